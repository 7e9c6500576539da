"""Bounded and occlusion ray queries on the MI355X (include/rt355.h: RT_QUERY_LIMITS, rt_trace_rays_ex, rt_trace_rays_host_ex,
rt_occluded, rt_occluded_host), bit for bit: (0.001, 9999) against rt_trace_rays, tmax against the oracle's nearest hit, tmin
against a float32 brute force over every (triangle, instance) pair and a per-ray-limit copy of the oracle's sphere loop,
occlusion against the limited nearest query, in every triangle kernel form and on sphere scenes of every chunk count."""

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi, load_mesh
from compute_raytracer_amd.procedural import obj_floor
from helpers import tri_buffers, triangle_scene
from query_common import (brute_triangles, camera_rays, check_triangle_hits, pack, random_rays, restate_triangle_hits, same,
                          scene_box, trace_spheres)
from test_ray_query_gpu import make_renderer, sphere_scene_with_duplicates, tri_cases

pytestmark = pytest.mark.gpu
F = np.float32
L = abi.RT_QUERY_LIMITS


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def wide_lookup(make):
    """A lookup table of more than 65,536 entries (the scene's own plus unused padding): the walk that pushes u16 node indices."""
    def f():
        scene, mat = make()
        scene.static["tri_lookup"] = np.concatenate([np.asarray(scene.static["tri_lookup"], F), np.zeros(70000, F)])
        return scene, mat
    return f


def wide_nodes(make):
    """A node buffer of more than 65,536 entries (unused zero nodes after the BLAS trees): the walk with u32 stacks."""
    def f():
        scene, mat = make()
        scene.static["blas_nodes"] = np.concatenate([np.asarray(scene.static["blas_nodes"], F), np.zeros((70000, 8), F)])
        scene.blasNodesUsed = scene.static["blas_nodes"].shape[0]
        return scene, mat
    return f


# hand-made trees the reference's walk does not search exhaustively (a spine deeper than its twenty stack slots, leaves beside a
# spine whose boxes the tree does not nest): the brute-force comparison does not apply to them
NOT_EXHAUSTIVE = ("spine24", "leafy3", "leafy4")


def form_cases():
    """tri_cases() and the forms they leave out: pair records with four triangles per leaf (no P16), and the instance-staged and
    per-frame-buffer walks with unpacked u16 and with u32 stacks."""
    from helpers import leafy_scene
    cases = dict(tri_cases())
    inst3 = lambda: triangle_scene(seed=43, n_models=2)
    inst17 = lambda: triangle_scene(seed=57, n_models=16)
    cases.update({
        "leafy4": lambda: (leafy_scene(4), rt.Material.white()),
        "inst3_u16": wide_lookup(inst3), "inst17_u16": wide_lookup(inst17),
        "inst3_u32": wide_nodes(inst3), "inst17_u32": wide_nodes(inst17),
    })
    return cases


FORMS = form_cases()
SPHERES = [1, 37, 1024, 5000, "dup"]


def quad_stack(k, instanced):
    """k upward-facing 2 x 2 quads at heights 0, -1, .., -(k-1) around (0, ., -5): one mesh of k quads, or k instances of one."""
    if instanced:
        mesh = load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 1.0], alignBottom=False, scale=1.0))
        models = [dict(meshIndex=0, position=[0.0, -float(j), -5.0], eulers=[0, 0, 0]) for j in range(k)]
    else:
        v, f = [], []
        for j in range(k):
            y = -float(j)
            v += ["v -1 %g 6" % y, "v 1 %g 6" % y, "v 1 %g 4" % y, "v -1 %g 4" % y]
            b = 4 * j
            f.append("f %d/1/1 %d/2/1 %d/3/1 %d/4/1" % (b + 1, b + 2, b + 3, b + 4))
        text = "\n".join(v) + "\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 1 0\n" + "\n".join(f) + "\n"
        # (the quads wind like obj_floor's, facing up; the loader centres the mesh, the model moves layer 0 to height 0)
        mesh = load_mesh(text, dict(color=[1.0, 1.0, 1.0, 1.0], alignBottom=False, scale=1.0))
        models = [dict(meshIndex=0, position=[0.0, -0.5 * (k - 1), -5.0], eulers=[0, 0, 0])]
    scene = rt.SceneRaytracing().createScene([])
    scene.createTriangleScene([mesh], models)
    return scene, rt.Material.white()


# ---- rays and queries ---------------------------------------------------------------------------------------------------------
def host_ex(r, rays, flags):
    hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
    abi.check(r._lib.rt_trace_rays_host_ex(r._ctx, rays.ctypes.data, rays.shape[0], flags, hits.ctypes.data), r._ctx)
    return hits


def host_occ(r, rays, flags):
    occ = np.full(rays.shape[0], 7, np.uint8)
    abi.check(r._lib.rt_occluded_host(r._ctx, rays.ctypes.data, rays.shape[0], flags, occ.ctypes.data), r._ctx)
    return occ


def same_records(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def segment_rays(lo, hi, n, seed):
    """o = A, d = B - A between random points of the box: tmin 0.001, tmax 1 is the segment."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, (n, 3)).astype(F)
    b = rng.uniform(lo, hi, (n, 3)).astype(F)
    return a, (b - a).astype(F)


def check_occlusion(r, o, d, tmin, tmax):
    """occluded == (limited nearest prim >= 0), on the host and the device paths; returns the number occluded."""
    rays = pack(o, d, tmin, tmax)
    near = host_ex(r, rays, L)
    occ = host_occ(r, rays, L)
    assert np.all((occ == 0) | (occ == 1))
    assert np.array_equal(occ.astype(bool), near["prim"] >= 0), "occlusion differs from the nearest query on %d rays" % int(
        (occ.astype(bool) != (near["prim"] >= 0)).sum())
    assert np.array_equal(r.occluded(o, d, tmin, tmax), occ.astype(bool))
    return int(occ.sum())


def sphere_setup(n):
    scene = sphere_scene_with_duplicates() if n == "dup" else rt.synthetic_scene(n, 11)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    lo, hi = (sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)
    return scene, sp, lo, hi


def sphere_rays(scene, sp, lo, hi, seed):
    """Camera rays, incoherent rays, and rays from inside spheres (origins near their centres)."""
    rng = np.random.default_rng(seed)
    count = 1024 if sp.shape[0] > 1000 else 4000
    sets = [camera_rays(scene, 64, 40), random_rays(lo, hi, count, seed)]
    k = rng.integers(0, sp.shape[0], count // 4)
    o = (sp[k, 0:3] + rng.uniform(-0.3, 0.3, (k.size, 3)) * sp[k, 7:8]).astype(F)
    d = rng.normal(size=(k.size, 3)).astype(F)
    sets.append((o, d))
    return [(np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)) for a, b in sets]


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------
def check_identity(r, o, d, seed):
    rays = pack(o, d)
    base = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
    abi.check(r._lib.rt_trace_rays_host(r._ctx, rays.ctypes.data, rays.shape[0], base.ctypes.data), r._ctx)
    assert same_records(host_ex(r, rays, L), base)                    # (0.001, 9999) is rt_trace_rays
    rng = np.random.default_rng(seed)
    junk = rays.copy()
    junk[:, 3] = rng.normal(size=rays.shape[0]) * 100
    junk[:, 7] = rng.uniform(-1, 1, rays.shape[0])
    junk[::7, 3] = np.nan
    assert same_records(host_ex(r, junk, 0), base)                    # without the flag words 3 and 7 are ignored
    assert np.array_equal(host_occ(r, junk, 0).astype(bool), base["prim"] >= 0)
    return base


@pytest.mark.parametrize("name", list(FORMS))
def test_triangles_identity_and_tmax_against_the_oracle(oracle, name):
    scene, mat = FORMS[name]()
    W, H = (168, 106) if name == "ref" else (96, 60)
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        lo, hi = scene_box(buf, scene)
        o1, d1 = camera_rays(scene, W, H)
        o2, d2 = random_rays(lo, hi, 3000, 17)
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        base = check_identity(r, o, d, 5)
        t_ref = oracle.trace_tri_rays(buf, o, d)
        assert np.array_equal(base["prim"] >= 0, t_ref != F(-1.0))
        hit = t_ref != F(-1.0)
        assert hit.sum() > 100
        rng = np.random.default_rng(9)
        # tmax <= t*: a miss
        below = np.where(rng.random(o.shape[0]) < 0.3, t_ref, t_ref * rng.uniform(0.0, 1.0, o.shape[0]).astype(F))
        h = host_ex(r, pack(o[hit], d[hit], 0.001, below[hit]), L)
        assert np.all(h["prim"] == -1) and np.all(h["t"] == F(-1.0))
        # tmax >= t* (1 + 2^-8): exactly the oracle's hit (the full query's record); misses stay misses
        above = (t_ref * F(1.0 + 2.0 ** -8) * rng.uniform(1.0, 3.0, o.shape[0]).astype(F)).astype(F)
        above = np.where(hit, np.maximum(above, t_ref * F(1.0 + 2.0 ** -8)), rng.uniform(0.01, 50.0, o.shape[0]).astype(F))
        h = host_ex(r, pack(o, d, 0.001, above), L)
        assert same_records(h, base)
        assert same(h["t"][hit], t_ref[hit])
    finally:
        r.close()


@pytest.mark.parametrize("name", list(FORMS))
def test_triangles_tmin_against_the_brute_force_and_occlusion(oracle, name):
    scene, mat = FORMS[name]()
    W, H = (84, 53) if name == "ref" else (64, 40)
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        lo, hi = scene_box(buf, scene)
        o1, d1 = camera_rays(scene, W, H)
        o2, d2 = random_rays(lo, hi, 1200 if name == "ref" else 2000, 23)
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        first = host_ex(r, pack(o, d), 0)["t"]
        rng = np.random.default_rng(31)
        pick = rng.integers(0, 4, o.shape[0])
        tmin = np.select([pick == 0, pick == 1, pick == 2],
                         [np.maximum(first, F(0.0)), first * rng.uniform(0.5, 1.5, o.shape[0]).astype(F),
                          rng.uniform(0.0, 30.0, o.shape[0]).astype(F)], F(0.001)).astype(F)
        tmax = np.where(rng.random(o.shape[0]) < 0.5, F(9999.0), tmin + rng.uniform(0.5, 40.0, o.shape[0]).astype(F)).astype(F)
        h = host_ex(r, pack(o, d, tmin, tmax), L)
        hit = h["prim"] >= 0
        assert hit.sum() > 50 and (~hit).sum() > 50
        # every hit restates bit for bit and lies in (tmin, tmax)
        with np.errstate(all="ignore"):
            t, u, v, nrm = restate_triangle_hits(buf, o[hit], d[hit], h["prim"][hit], h["instance"][hit])
        assert same(t, h["t"][hit]) and same(u, h["u"][hit]) and same(v, h["v"][hit]) and same(nrm, h["normal"][hit])
        assert np.all(h["t"][hit] > tmin[hit]) and np.all(h["t"][hit] < tmax[hit])
        # the brute force accepts nothing nearer, and nothing at all where the walk missed
        with np.errstate(all="ignore"):
            best = np.where(hit, h["t"], F(np.inf)) if name in NOT_EXHAUSTIVE else brute_triangles(buf, o, d, tmin, tmax)
        below = hit & (best < h["t"])
        assert not below.any(), "the brute force finds nearer hits on %d rays" % int(below.sum())
        assert np.all(np.isinf(best[~hit])), "the walk misses %d rays the brute force hits" % int(np.isfinite(best[~hit]).sum())
        assert same(best[hit], h["t"][hit])
        # occlusion: the same rays and limits, the default limits, and segments
        assert check_occlusion(r, o, d, tmin, tmax) == int(hit.sum())
        check_occlusion(r, o, d, F(0.001), F(9999.0))
        a, s = segment_rays(lo, hi, 3000, 29)
        assert 0 < check_occlusion(r, a, s, F(0.001), F(1.0)) < a.shape[0]
    finally:
        r.close()


@pytest.mark.parametrize("instanced", [False, True])
def test_tmin_between_layers_selects_the_next_layer(instanced):
    k = 9
    scene, mat = quad_stack(k, instanced)
    r = make_renderer(scene, mat, 64, 40)
    try:
        buf = tri_buffers(scene, mat)
        rng = np.random.default_rng(3)
        n = 600
        o = np.stack([rng.uniform(-0.9, 0.9, n), np.full(n, 10.0), rng.uniform(-5.9, -4.1, n)], axis=1).astype(F)
        d = np.tile(np.array([0.0, -1.0, 0.0], F), (n, 1))
        j = rng.integers(0, k, n)
        tmin = (10.0 + j - rng.uniform(0.05, 0.95, n)).astype(F)            # between layer j-1 (t = 9 + j) and layer j (t = 10 + j)
        h = host_ex(r, pack(o, d, tmin, 9999.0), L)
        assert np.all(h["prim"] >= 0)
        y = o[:, 1] + h["t"] * d[:, 1]
        assert np.allclose(y, -j, atol=1e-4), "tmin selects the wrong layer on %d rays" % int((~np.isclose(y, -j, atol=1e-4)).sum())
        if instanced:
            assert np.array_equal(h["instance"], j)
        with np.errstate(all="ignore"):
            t, u, v, nrm = restate_triangle_hits(buf, o, d, h["prim"], h["instance"])
        assert same(t, h["t"]) and same(nrm, h["normal"])
        # beyond the last layer: a miss; a tmax between layers j and j+1 keeps layer j; every segment through a layer is occluded
        assert np.all(host_ex(r, pack(o, d, F(10.0 + k - 0.5), 9999.0), L)["prim"] == -1)
        h2 = host_ex(r, pack(o, d, tmin, (10.0 + j + 0.5).astype(F)), L)
        assert same_records(h2, h)
        assert np.all(host_occ(r, pack(o, d, tmin, (10.0 + j + 0.5).astype(F)), L) == 1)
        assert np.all(host_occ(r, pack(o, d, tmin, (10.0 + j - 0.01).astype(F)), L) == 0)
        assert check_occlusion(r, o, d * F(30.0), F(0.001), F(1.0)) == n             # segments through all k layers
    finally:
        r.close()


# ---- spheres ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SPHERES)
def test_spheres_limits_against_the_oracle_and_occlusion(oracle, n):
    scene, sp, lo, hi = sphere_setup(n)
    r = make_renderer(scene)
    try:
        rng = np.random.default_rng(41)
        hits = misses = behind = 0
        for o, d in sphere_rays(scene, sp, lo, hi, 43):
            base = check_identity(r, o, d, 7)
            m = o.shape[0]
            with np.errstate(all="ignore"):
                t_ref, idx_ref = trace_spheres(sp, o, d, F(0.001), F(9999.0))
            assert np.array_equal(base["prim"], np.where(idx_ref < 0, -1, idx_ref))
            first = np.where(idx_ref >= 0, t_ref, F(5.0)).astype(F)
            pick = rng.integers(0, 4, m)
            reach = F(2.0) * sp[:, 7].max() / np.sqrt((d * d).sum(axis=1))               # (a root behind the origin: up to a diameter)
            tmin = np.select([pick == 0, pick == 1, pick == 2], [first, -rng.uniform(0.0, 1.0, m).astype(F) * reach,
                             first * rng.uniform(0.5, 1.5, m).astype(F)], F(0.001)).astype(F)
            tmax = np.where(rng.random(m) < 0.5, F(9999.0), first * rng.uniform(0.5, 3.0, m).astype(F)).astype(F)
            tmax[::11] = first[::11]                                                    # tmax = t*: the nearest is excluded
            h = host_ex(r, pack(o, d, tmin, tmax), L)
            with np.errstate(all="ignore"):
                want_t, want_i = trace_spheres(sp, o, d, tmin, tmax)
            miss = want_i < 0
            assert np.array_equal(h["prim"], np.where(miss, -1, want_i).astype(np.int32))
            assert same(h["t"], np.where(miss, F(-1.0), want_t))
            hits, misses, behind = hits + int((~miss).sum()), misses + int(miss.sum()), behind + int((h["t"][~miss] < 0).sum())
            for i in np.nonzero(~miss)[0][:: max(1, int((~miss).sum()) // 100)]:
                ok, t, nrm = oracle.hit_sphere(o[i], d[i], sp[h["prim"][i]], tmin[i], tmax[i])
                assert ok and same(t, h["t"][i]) and same(nrm, h["normal"][i])
            if n == "dup":
                assert np.all(h["prim"][~miss] < sp.shape[0] // 2)                    # the lower index wins a tie
            assert check_occlusion(r, o, d, tmin, tmax) == int((~miss).sum())
        assert hits > 0 and misses > 0 and behind > 0                              # (behind: a negative tmin admits a root behind the origin)
        a, s = segment_rays(lo, hi, 2000, 47)
        check_occlusion(r, a, s, F(0.001), F(1.0))
    finally:
        r.close()


def test_crowded_spheres_stop_early_and_agree():
    """Hundreds of overlapping spheres: almost every ray is occluded within the first chunk, most workgroups stop staging; the
    lanes that search on (rays that slip through) still find exactly what the nearest query finds."""
    from helpers import crowded_spheres
    scene = rt.SceneRaytracing().createScene(crowded_spheres(3000, 8))
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    r = make_renderer(scene)
    try:
        o, d = camera_rays(scene, 96, 64)
        occ = check_occlusion(r, o, d, F(0.001), F(9999.0))
        assert occ > 0.5 * o.shape[0]
        rng = np.random.default_rng(5)
        a, s = segment_rays(sp[1:, 0:3].min(axis=0), sp[1:, 0:3].max(axis=0), 4000, 6)
        check_occlusion(r, a, s, F(0.001), F(1.0))
        tmin = rng.uniform(-2.0, 20.0, o.shape[0]).astype(F)
        check_occlusion(r, o, d, tmin, (tmin + rng.uniform(0.0, 3.0, o.shape[0])).astype(F))
    finally:
        r.close()


# ---- paths, pose, frames ------------------------------------------------------------------------------------------------------
def test_device_and_host_paths_agree_and_no_scene_is_refused():
    import torch
    scene, mat = triangle_scene(seed=91, n_models=4)
    W, H = 120, 80
    r = make_renderer(scene, mat, W, H)
    lib = r._lib
    try:
        o, d = camera_rays(scene, W, H, 2)
        rng = np.random.default_rng(1)
        rays = pack(o, d, rng.uniform(0.0, 8.0, o.shape[0]).astype(F), rng.uniform(4.0, 30.0, o.shape[0]).astype(F))
        host = host_ex(r, rays, L)
        occ = host_occ(r, rays, L)
        dev_rays = torch.from_numpy(rays).to("cuda:0")
        dev = r.trace_rays(dev_rays, limits=True)
        dev_occ = r.occluded(dev_rays)
        torch.cuda.synchronize()
        assert dev_occ.dtype == torch.uint8 and tuple(dev_occ.shape) == (o.shape[0],)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(-1), host.view(np.uint32))
        assert np.array_equal(dev_occ.cpu().numpy(), occ)
        # the numpy keywords
        res = r.trace_rays(o, d, tmin=rays[:, 3], tmax=rays[:, 7])
        assert np.array_equal(res["prim"], host["prim"]) and same(res["t"], host["t"])
        assert np.array_equal(r.occluded(o, d, rays[:, 3], rays[:, 7]), occ.astype(bool))
        assert r.occluded(o, d).dtype == bool
        # the raw device entry points, an `out` tensor, the context's stream
        out = torch.full((o.shape[0],), 9, dtype=torch.uint8, device="cuda:0")
        assert r.occluded(dev_rays, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), occ)
        hits = torch.zeros((o.shape[0], 8), dtype=torch.float32, device="cuda:0")
        abi.check(lib.rt_trace_rays_ex(r._ctx, dev_rays.data_ptr(), o.shape[0], L, hits.data_ptr(), None), r._ctx)
        torch.cuda.synchronize()
        assert np.array_equal(hits.cpu().numpy().view(np.uint32).reshape(-1), host.view(np.uint32))
        # n == 0, NULL pointers, unknown flags, misalignment
        for fn in (lib.rt_trace_rays_ex, lib.rt_occluded):
            assert fn(r._ctx, None, 0, L, None, None) == abi.RT_OK
            assert fn(r._ctx, None, 4, L, None, None) == abi.RT_ERR_INVALID_ARG
            assert fn(r._ctx, dev_rays.data_ptr(), 4, 2, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG
        for fn in (lib.rt_trace_rays_host_ex, lib.rt_occluded_host):
            assert fn(r._ctx, None, 0, 0, None) == abi.RT_OK
            assert fn(r._ctx, rays.ctypes.data, 4, 0, None) == abi.RT_ERR_INVALID_ARG
            assert fn(r._ctx, rays.ctypes.data, 4, 6, occ.ctypes.data) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_ex(r._ctx, dev_rays.data_ptr() + 4, 1, 0, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_occluded(r._ctx, dev_rays.data_ptr(), 1, 0, out.data_ptr() + 1, None) == abi.RT_OK   # no alignment needed
        # the messages whole -- each names its entry point and what it asks to be aligned -- and the order when two arguments are wrong
        err = lambda: lib.rt_last_error(r._ctx)
        for fn, name, nouns in ((lib.rt_trace_rays_ex, b"rt_trace_rays_ex", b"rays and hits"), (lib.rt_occluded, b"rt_occluded", b"rays")):
            assert fn(r._ctx, dev_rays.data_ptr() + 4, 1, L, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG
            assert err() == name + b": " + nouns + b" must be 16-byte aligned"
            assert fn(r._ctx, None, 4, L, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG and err() == name + b": NULL argument"
            assert fn(r._ctx, None, 4, 2, None, None) == abi.RT_ERR_INVALID_ARG and err() == name + b": unknown flag bits 0x2"   # flags first
            assert fn(r._ctx, None, 4, L, hits.data_ptr() + 4, None) == abi.RT_ERR_INVALID_ARG and err() == name + b": NULL argument"
        assert lib.rt_trace_rays_ex(r._ctx, dev_rays.data_ptr(), 1, 0, hits.data_ptr() + 4, None) == abi.RT_ERR_INVALID_ARG
        assert err() == b"rt_trace_rays_ex: rays and hits must be 16-byte aligned"
        for fn, name in ((lib.rt_trace_rays_host_ex, b"rt_trace_rays_host_ex"), (lib.rt_occluded_host, b"rt_occluded_host")):
            assert fn(r._ctx, None, 4, 0, occ.ctypes.data) == abi.RT_ERR_INVALID_ARG and err() == name + b": NULL argument"
            assert fn(r._ctx, None, 4, 6, None) == abi.RT_ERR_INVALID_ARG and err() == name + b": unknown flag bits 0x6"
        assert lib.rt_occluded_host(r._ctx, rays.ctypes.data + 4, 1, L, np.zeros(1, np.uint8).ctypes.data) == abi.RT_OK   # host memory: any address
        torch.cuda.synchronize()
    finally:
        r.close()
    bare = rt.RendererRaytracing(16, 16, rt.synthetic_scene(3, 1)).initialize()
    try:
        rays = pack(np.zeros((1, 3), F), np.array([[0.0, 0.0, -1.0]], F))
        hits = np.zeros(1, dtype=abi.HIT_DTYPE)
        occ = np.zeros(1, np.uint8)
        for flags in (0, L):
            assert bare._lib.rt_trace_rays_host_ex(bare._ctx, rays.ctypes.data, 1, flags, hits.ctypes.data) == abi.RT_ERR_STATE
            assert bare._lib.rt_occluded_host(bare._ctx, rays.ctypes.data, 1, flags, occ.ctypes.data) == abi.RT_ERR_STATE
            assert bare._lib.rt_last_error(bare._ctx) == b"rt_occluded_host: no scene has been written"
        assert bare._lib.rt_occluded_host(bare._ctx, rays.ctypes.data, 1, 2, occ.ctypes.data) == abi.RT_ERR_INVALID_ARG
    finally:
        bare.close()


@pytest.mark.parametrize("n_inst", [3, 17])
def test_occlusion_sees_the_pose_no_frame_has_carried(oracle, n_inst):
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    W, H = 120, 76
    r = make_renderer(scene, mat, W, H)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        scene.update(0.5)
        new = tri_buffers(scene, mat)
        o, d = camera_rays(scene, W, H)
        t_new, t_old = oracle.trace_tri_rays(new, o, d), oracle.trace_tri_rays(old, o, d)
        # segments that end just beyond the new pose's hit: occluded exactly where the new pose has one
        tmax = np.where(t_new > 0, t_new * F(1.0 + 2.0 ** -8), F(1.0)).astype(F)
        occ = r.occluded(o, d, F(0.001), tmax)
        assert np.array_equal(occ, t_new > 0)
        short = np.where(t_new > 0, t_new, F(1.0)).astype(F)                           # ... and ending at it: never occluded
        occ_short = r.occluded(o, d, F(0.001), short)
        assert not occ_short.any()
        old_answers = np.concatenate([(t_old > 0) & (t_old < tmax), (t_old > 0) & (t_old < short)])
        assert not np.array_equal(old_answers, np.concatenate([occ, occ_short]))    # the old pose would answer otherwise
        h = r.trace_rays(o, d, tmin=F(0.001), tmax=tmax)
        check_triangle_hits(oracle, new, o, d, h)
    finally:
        r.close()


def test_limited_queries_do_not_disturb_frames(oracle):
    import torch
    scene, mat = triangle_scene(seed=81, n_models=3)
    W, H = 160, 100
    r = make_renderer(scene, mat, W, H)
    try:
        ref, _, ref_rays = oracle.render_tri(scene.pack_params(2), tri_buffers(scene, mat), r.skyboxMaterial.faces, W, H)
        r.render()
        o, d = camera_rays(scene, W, H, 3)
        rays = pack(o, d, 0.5, 12.0)
        dev = torch.from_numpy(rays).to("cuda:0")
        frames = r.host_frames(4)
        want_h, want_o = host_ex(r, rays, L), host_occ(r, rays, L)

        def batch(query):
            for _ in range(4):
                r.enqueue()
            out = None
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    out = (r.trace_rays(dev, limits=True), r.occluded(dev))
            r.enqueue()
            for k in range(4):
                r.read_pixels_async(k, frames[k])
            r.wait()
            r.read_pixels_wait()
            if query:
                side.synchronize()
            return out

        batch(False)
        batch(False)
        s0 = r.stats()
        hits, occ = batch(True)
        s1 = r.stats()
        for f in frames + [r.read_pixels()]:
            assert np.array_equal(f, ref)
        assert s1["frames"] == s0["frames"] + 5 and s1["batch_frames"] == s0["batch_frames"]
        for k in ("rays", "kernel_id", "tri_form"):
            assert s1[k] == s0[k], k
        assert s1["rays"] == ref_rays
        before = r.stats()
        assert np.array_equal(hits.cpu().numpy().view(np.uint32).reshape(-1), want_h.view(np.uint32))
        assert np.array_equal(occ.cpu().numpy(), want_o)
        host_ex(r, rays, L)
        host_occ(r, rays, 0)
        assert r.stats() == before                                   # a query changes no statistic
    finally:
        r.close()
