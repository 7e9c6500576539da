"""Shared by the ambient-occlusion tests (test infrastructure; tests/test_render_ao_cpu.py, test_render_ao_gpu.py): "what one pixel
computes" of include/rt355.h (rt_render_ao) restated in numpy float32, one operation per line in the header's order -- from
pick-style hits, the camera origin, the primary directions and the k tangent-space directions to the packed limited rays whose
rt_occluded answers a pixel's count sums -- and the primary hits of a triangle scene by the CPU alone."""
import numpy as np

from query_common import F, all_triangle_hits, bits, k_smallest, restate_triangle_hits


def ao_basis(n):
    """T and B of the header for normals n (m, 3) float32: s = (n.z >= 0) ? 1 : -1, a = -1 / (s + n.z), b = (n.x * n.y) * a,
    T = (1 + ((s * n.x) * n.x) * a, s * b, (-s) * n.x), B = (b, s + (n.y * n.y) * a, -n.y)."""
    n = np.asarray(n, F)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = np.where(nz >= F(0.0), F(1.0), F(-1.0)).astype(F)     # (-0 gives +1, NaN gives -1)
        a = F(-1.0) / (s + nz)
        b = (nx * ny) * a
        T = np.stack([F(1.0) + ((s * nx) * nx) * a, s * b, (-s) * nx], axis=1)
        B = np.stack([b, s + (ny * ny) * a, -ny], axis=1)
    return T.astype(F), B.astype(F)


def ao_rays(hits, o, d, dirs, tmin, radius):
    """hits: pick-style {"t", "prim", "normal"} of n pixels; o, d: (n, 3) camera origin and primary directions; dirs: (k, 3).
    -> the indices of the m pixels that hit, and their rays as (m, k, 8) float32 {origin, tmin, direction, radius}: origin
    p = o + t * d per component, direction (dirs[j].x * T + dirs[j].y * B) + dirs[j].z * n per component."""
    dirs = np.asarray(dirs, F).reshape(-1, 3)
    hit = np.nonzero(np.asarray(hits["prim"]) >= 0)[0]
    t = np.asarray(hits["t"], F)[hit]
    n = np.asarray(hits["normal"], F)[hit]
    oh, dh = np.asarray(o, F)[hit], np.asarray(d, F)[hit]
    with np.errstate(all="ignore"):
        p = oh + t[:, None] * dh
        T, B = ao_basis(n)
        rays = np.zeros((hit.size, dirs.shape[0], 8), F)
        rays[:, :, 0:3] = p[:, None, :]
        rays[:, :, 3] = F(tmin)
        rays[:, :, 7] = F(radius)
        for j in range(dirs.shape[0]):
            rays[:, j, 4:7] = (dirs[j, 0] * T + dirs[j, 1] * B) + dirs[j, 2] * n
    return hit, rays


def counts_from(n_pixels, hit, occluded, k):
    """The count plane, flat: `occluded` is the (m * k,) answers for ao_rays' rays in their order"""
    count = np.zeros(n_pixels, np.uint8)
    count[hit] = np.asarray(occluded).reshape(hit.size, k).sum(axis=1)
    return count


def ao_of(count, k):
    """The ao plane of a count plane: (float)(k - count) / (float)k in float32"""
    return ((F(k) - count.astype(F)) / F(k)).astype(F)


def cpu_primary_hits(oracle, buf, o, d):
    """pick-style hits of rays (o, d) against a triangle scene without the device: the nearest (t, instance, prim) of the float32
    brute force over every (triangle, instance) pair within (0.001, 9999), t checked against the oracle's walk bit for bit, and
    the shading normal restated."""
    n = o.shape[0]
    with np.errstate(all="ignore"):
        T, I, P, _ = k_smallest(n, 1, all_triangle_hits(buf, o, d), F(0.001), F(9999.0))
    t, inst, prim = T[:, 0], I[:, 0], P[:, 0]
    assert np.array_equal(bits(t), bits(oracle.trace_tri_rays(buf, o, d))), "the brute force and the oracle's walk disagree"
    normal = np.zeros((n, 3), F)
    hit = prim >= 0
    with np.errstate(all="ignore"):
        normal[hit] = restate_triangle_hits(buf, o[hit], d[hit], prim[hit], inst[hit])[3]
    return {"t": t, "prim": prim, "instance": inst, "normal": normal}


def cpu_occluded(oracle, buf, rays):
    """rt_occluded for limited rays (m, 8) with tmin = 0.001 by the oracle's nearest-hit walk: occluded iff it hits with
    t < radius (the walk's own tMin is 0.001; on builder-made trees the nearest hit within 9999 decides every shorter interval)."""
    assert np.all(rays[:, 3] == F(0.001))
    t = oracle.trace_tri_rays(buf, rays[:, 0:3], rays[:, 4:7])
    return (t > 0) & (t < rays[:, 7])
