"""Shared by the ray-query tests (test infrastructure; tests/test_ray_query_gpu.py, test_ray_limits_gpu.py, test_ray_multi_gpu.py,
test_query_lifecycle_gpu.py): float-bit comparison, the rays the queries are tried with, the triangle hit restated in float32, the
float32 brute forces over every (triangle, instance) pair and over every sphere, and check_all_queries -- every query family against
its reference for one scene state, bit for bit."""
import numpy as np

import shade_common
from compute_raytracer_amd import abi
from oracle import rt_oracle_np

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differ(a, b):
    """Elementwise: the float32 words differ as bits (the sign of zero and a NaN's payload included).  The comparisons below take
    another rule of the same shape through their `differ` argument (tests/tri_edge_common.py has one)."""
    return bits(a) != bits(b)


def same(a, b, differ=differ):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not differ(a, b).any()


_same = same                                            # (the comparisons below rebind `same` to their own rule)


# ---- rays --------------------------------------------------------------------------------------------------------------------
def camera_rays(scene, W, H, step=1):
    """The primary rays of a W x H frame (RK:76-86 in float32, the oracle's order), every `step`-th pixel."""
    p = scene.pack_params(2)
    cam, fw, rgt, up = p[0:3], p[4:7], p[8:11], p[12:15]
    ys, xs = np.mgrid[0:H:step, 0:W:step]
    xs = xs.reshape(-1); ys = ys.reshape(-1)
    hc = (xs.astype(F) - F(W) / F(2)) / F(W) * F(2)
    vc = (F(H) / F(2) - ys.astype(F)) / F(W) * F(2)
    d = np.stack([(fw[k] + hc * rgt[k]) + vc * up[k] for k in range(3)], axis=1).astype(F)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d / ln[:, None]
    return np.broadcast_to(cam, d.shape).astype(F), d.astype(F)


def random_rays(lo, hi, n, seed):
    """Incoherent rays: origins in the box grown by half its size on every side (inside and outside the scene), directions of
    lengths 0.05 .. 20 (not unit)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    o = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.05, 20.0, (n, 1))
    return o, d.astype(F)


def axis_rays(lo, hi, seed, per_axis=100):
    """Directions along the axes (the inverse direction is +-inf in two components)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (6 * per_axis, 3)).astype(F)
    d = np.zeros((6 * per_axis, 3), F)
    for k in range(6):
        d[k * per_axis:(k + 1) * per_axis, k // 2] = F(1.0 if k % 2 == 0 else -1.0) * F(0.5 + k)
    return o, d


def scene_box(buf, scene):
    """The top-level root's box, within 20 of the camera (the reference's floor spans millions)."""
    root, cam = buf["nodes"][0], scene.pack_params(2)[0:3]
    return np.maximum(root[0:3], cam - 20.0), np.minimum(root[4:7], cam + 20.0)


def pack(o, d, tmin=0.001, tmax=9999.0):
    rays = np.zeros((o.shape[0], 8), F)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = tmin, tmax
    return rays


# ---- the triangle hit restated in float32 --------------------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def mat_apply(m, v, w):
    """mat4 (column-major, m[4c + r]) * vec4(v, w), summed over columns left to right (RK:254-255)."""
    return np.stack([((m[:, r] * v[:, 0] + m[:, 4 + r] * v[:, 1]) + m[:, 8 + r] * v[:, 2]) + m[:, 12 + r] * F(w) for r in range(3)], axis=1)


def restate_triangle_hits(buf, o, d, prim, inst):
    """t, u, v (RK:354-379) of triangle `prim` in the object space of instance `inst`, and the shading normal (RK:381-382,
    RK:334-338): every operation a float32 operation, in the oracle's order."""
    m = np.asarray(buf["blas"], F).reshape(-1, 20)[inst]
    tri = np.asarray(buf["triangles"], F).reshape(-1, 40)[prim]
    oo, od = mat_apply(m, o, 1.0), mat_apply(m, d, 0.0)
    A, B, C = tri[:, 0:3], tri[:, 12:15], tri[:, 24:27]
    e1, e2 = B - A, C - A
    rce2 = cross(od, e2)
    det = dot(e1, rce2)
    s = oo - A
    u = dot(s, rce2)
    sce1 = cross(s, e1)
    v = dot(od, sce1)
    inv = F(1.0) / det
    t = inv * dot(e2, sce1)
    u = u * inv
    v = v * inv
    w = (F(1.0) - u) - v
    n = (w[:, None] * tri[:, 4:7] + u[:, None] * tri[:, 16:19]) + v[:, None] * tri[:, 28:31]
    tn = np.stack([((m[:, 4 * r + 0] * n[:, 0] + m[:, 4 * r + 1] * n[:, 1]) + m[:, 4 * r + 2] * n[:, 2]) + m[:, 4 * r + 3] * F(0.0)
                   for r in range(3)], axis=1)
    nrm = tn / np.sqrt(dot(tn, tn))[:, None]
    return t, u, v, nrm


def check_triangle_hits(oracle, buf, o, d, h, differ=differ):
    same = lambda a, b: _same(a, b, differ)
    t_ref = oracle.trace_tri_rays(buf, o, d)
    miss = h["prim"] < 0
    assert np.array_equal(miss, t_ref == F(-1.0)), "miss sets differ: %d vs %d" % (miss.sum(), (t_ref == -1).sum())
    assert same(h["t"], t_ref), "t differs from the oracle on %d rays" % int(differ(h["t"], t_ref).sum())
    assert np.all(h["instance"][miss] == -1) and np.all(h["u"][miss] == 0) and np.all(h["v"][miss] == 0)
    assert np.all(h["normal"][miss] == 0)
    hit = ~miss
    if hit.any():
        assert np.all(h["instance"][hit] >= 0) and np.all(h["prim"][hit] < len(buf["triangles"]))
        with np.errstate(all="ignore"):
            t, u, v, nrm = restate_triangle_hits(buf, o[hit], d[hit], h["prim"][hit], h["instance"][hit])
        assert same(t, h["t"][hit]) and same(u, h["u"][hit]) and same(v, h["v"][hit])
        assert same(nrm, h["normal"][hit])
    return int(hit.sum())


# ---- the box test and the triangle test, term by term (tests/tri_edge_common.py counts their edge cases) ---------------------------
def u32f(f):
    """WGSL u32(f32): truncating, saturating, NaN and negatives -> 0"""
    f = float(f)
    if not f > 0.0:
        return 0
    return 4294967295 if f >= 4294967040.0 else int(f)


def hit_aabb(lo, hi, o, inv, terms=False):
    """hitAABB (RK:395-410) in float32 for boxes lo / hi (3,) or (n, 3) and rays o, inv = 1 / d (n, 3): the entry distance, 99999
    on a miss.  fmin / fmax drop a NaN operand as C's fminf / fmaxf do.  terms: also the six slab products t1, t2."""
    t1 = (np.asarray(lo, F) - o) * inv                               # RK:397
    t2 = (np.asarray(hi, F) - o) * inv                               # RK:398
    lo3, hi3 = np.fmin(t1, t2), np.fmax(t1, t2)                      # RK:399-400
    t_min = np.fmax(np.fmax(lo3[..., 0], lo3[..., 1]), lo3[..., 2])  # RK:402
    t_max = np.fmin(np.fmin(hi3[..., 0], hi3[..., 1]), hi3[..., 2])  # RK:403
    dist = np.where((t_min > t_max) | (t_max < F(0.0)), F(99999.0), t_min).astype(F)   # RK:405-409
    return (dist, t1, t2) if terms else dist


def walk_leaves(nodes, root, o, d, limit, visit=None):
    """The leaves of the tree under node `root` a walk (RK:179-240, RK:271-330) can reach for rays o, d (n, 3): [(left, count,
    mask (n,))], mask = no box on the way down was missed or entered beyond `limit` (the value the running nearest hit starts
    from: it only falls).  The root's own box is not tested, as in the reference.  visit(child index, dist, t1, t2, mask) sees
    every box test.  Indices clamp to the last node; a buffer that is no tree is cut off after 4 n node visits."""
    nodes = np.asarray(nodes, F).reshape(-1, 8)
    last = nodes.shape[0] - 1
    inv = F(1.0) / d
    out, todo, budget = [], [(min(int(root), last), np.ones(o.shape[0], bool))], 4 * nodes.shape[0] + 4
    while todo and budget > 0:
        budget -= 1
        i, mask = todo.pop()
        left, count = u32f(nodes[i, 3]), u32f(nodes[i, 7])
        if count:
            out.append((left, count, mask))
            continue
        for c in (left, (left + 1) & 0xFFFFFFFF):
            c = min(c, last)
            dist, t1, t2 = hit_aabb(nodes[c, 0:3], nodes[c, 4:7], o, inv, terms=True)
            if visit is not None:
                visit(c, dist, t1, t2, mask)
            m = mask & ~(dist > limit)
            if m.any():
                todo.append((c, m))
    return out


def reach(buf, o, d, limit, visit=None):
    """{instance record: (slots, mask (n, len(slots)))}: the lookup slots whose leaf the two-level walk can reach per ray, by
    walk_leaves over the top-level tree and then over each instance's tree in its object space.  visit(instance record or None
    for the top level, direction there (n, 3), dist, t1, t2, mask) sees every box test a ray can come to."""
    nodes = np.asarray(buf["nodes"], F).reshape(-1, 8)
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    look = np.asarray(buf["blas_lookup"], F)
    n, n_slots = o.shape[0], len(buf["tri_lookup"])
    limit = np.broadcast_to(np.asarray(limit, F), (n,))
    per_inst = {}
    top = None if visit is None else (lambda c, dist, t1, t2, m: visit(None, d, dist, t1, t2, m))
    for left, count, mask in walk_leaves(nodes, 0, o, d, limit, top):
        for k in range(min(count, len(look))):
            bi = min(u32f(look[min(left + k, len(look) - 1)]), blas.shape[0] - 1)
            per_inst[bi] = per_inst.get(bi, np.zeros(n, bool)) | mask
    out = {}
    for bi, mask in per_inst.items():
        m = np.broadcast_to(blas[bi], (n, 20))
        oo, od = mat_apply(m, o, 1.0), mat_apply(m, d, 0.0)
        got = {}
        low = None if visit is None else (lambda c, dist, t1, t2, lm, bi=bi, od=od, mask=mask: visit(bi, od, dist, t1, t2, lm & mask))
        for left, count, lm in walk_leaves(nodes, u32f(blas[bi, 16]), oo, od, limit, low):
            for k in range(min(count, 4 * n_slots)):
                s = min(left + k, n_slots - 1)
                got[s] = got.get(s, np.zeros(n, bool)) | (lm & mask)
        slots = np.array(sorted(got), np.int64)
        out[bi] = (slots, np.stack([got[s] for s in slots], axis=1) if slots.size else np.zeros((n, 0), bool))
    return out


def triangle_terms(m, tris, o, d):
    """hitTriangle's terms (RK:354-379) for n rays against P triangles (P, 40) in the object space of instance record m (20,), each
    (n, P) float32 in the oracle's order: det, u, v (before the division), tnum = dot(edge2, sCrossEdge1), t, and `ok`, the
    tests of RK:359-372 passed -- written as the shader's rejections, so a NaN passes where it passes there."""
    n = o.shape[0]
    mm = np.broadcast_to(np.asarray(m, F), (n, 20))
    oo, od = mat_apply(mm, o, 1.0), mat_apply(mm, d, 0.0)
    A, B, C = tris[:, 0:3], tris[:, 12:15], tris[:, 24:27]
    e1, e2 = (B - A)[None], (C - A)[None]
    shape = (n,) + e2.shape[1:]
    odc = np.broadcast_to(od[:, None, :], shape)
    rce2 = cross(odc, np.broadcast_to(e2, shape))
    det = dot(e1, rce2)
    s = oo[:, None, :] - A[None]
    u = dot(s, rce2)
    sce1 = cross(s, np.broadcast_to(e1, shape))
    v = dot(odc, sce1)
    tnum = dot(np.broadcast_to(e2, shape), sce1)
    t = (F(1.0) / det) * tnum
    ok = ~(det < F(0.00001)) & ~((u < 0) | (u > det)) & ~((v < 0) | (u + v > det))
    return dict(det=det, u=u, v=v, tnum=tnum, t=t, ok=ok, oo=oo, od=od)


# ---- triangles: the float32 brute force ---------------------------------------------------------------------------------------
def blas_slots(buf, root):
    """The lookup slots of the leaves under node `root` (RK:246-332 reaches no others)."""
    nodes = np.asarray(buf["nodes"], F)
    n_lookup = len(buf["tri_lookup"])
    out, todo = [], [int(root)]
    while todo:
        i = min(todo.pop(), nodes.shape[0] - 1)
        left, count = int(nodes[i, 3]), int(nodes[i, 7])
        if count == 0:
            todo += [left, left + 1]
        else:
            out += [min(left + k, n_lookup - 1) for k in range(count)]
    return np.unique(np.asarray(out, np.int64))


def brute_triangles(buf, o, d, tmin, tmax, boxes=False):
    """The smallest t that hit_triangle (RK:344-381) accepts within (tmin, tmax) over every (triangle, instance) pair, in the
    same float32 operations; +inf where none does.  boxes: only the pairs whose leaf the walk can reach (reach(): a ray that lies
    in the plane of a box face with a zero direction component there misses that box in the reference, whatever is inside)."""
    if boxes:
        n = o.shape[0]
        tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
        lookup = np.asarray(buf["tri_lookup"], F)
        lo_t = np.broadcast_to(np.asarray(tmin, F), (n,))
        hi_t = np.broadcast_to(np.asarray(tmax, F), (n,))
        best = np.full(n, np.inf, F)
        for bi, (slots, mask) in reach(buf, o, d, hi_t).items():
            if not slots.size:
                continue
            prims = np.array([min(u32f(lookup[s]), tris.shape[0] - 1) for s in slots], np.int64)
            q = triangle_terms(np.asarray(buf["blas"], F).reshape(-1, 20)[bi], tris[prims], o, d)
            ok = q["ok"] & mask & (q["t"] > lo_t[:, None]) & (q["t"] < hi_t[:, None])
            best = np.minimum(best, np.where(ok, q["t"], np.inf).min(axis=1).astype(F))
        return best
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    lookup = np.asarray(buf["tri_lookup"], F)
    n = o.shape[0]
    best = np.full(n, np.inf, F)
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    for bi in np.unique(np.asarray(buf["blas_lookup"], np.int64).clip(0, blas.shape[0] - 1)):
        m = np.broadcast_to(blas[bi], (n, 20))
        oo, od = mat_apply(m, o, 1.0), mat_apply(m, d, 0.0)
        prims = np.minimum(lookup[blas_slots(buf, blas[bi, 16])].astype(np.int64), tris.shape[0] - 1)
        A, B, C = tris[prims, 0:3], tris[prims, 12:15], tris[prims, 24:27]
        e1, e2 = (B - A)[None], (C - A)[None]
        for s0 in range(0, n, 256):
            sl = slice(s0, s0 + 256)
            odc, ooc = od[sl, None, :], oo[sl, None, :]
            rce2 = cross(np.broadcast_to(odc, (odc.shape[0],) + e2.shape[1:]), np.broadcast_to(e2, (odc.shape[0],) + e2.shape[1:]))
            det = dot(e1, rce2)
            s = ooc - A[None]
            u = dot(s, rce2)
            sce1 = cross(s, np.broadcast_to(e1, s.shape))
            v = dot(np.broadcast_to(odc, s.shape), sce1)
            t = (F(1.0) / det) * dot(np.broadcast_to(e2, s.shape), sce1)
            ok = ~(det < F(0.00001)) & ~((u < 0) | (u > det)) & ~((v < 0) | (u + v > det))
            ok &= (t > tmin[sl, None]) & (t < tmax[sl, None])
            cand = np.where(ok, t, np.inf).min(axis=1)
            best[sl] = np.minimum(best[sl], cand)
    return best


def all_triangle_hits(buf, o, d, boxes=False):
    """Every (ray, t, instance, prim) that passes hit_triangle's tests (RK:344-379) over every (triangle, instance) pair, in the
    same float32 operations as brute_triangles; the limits are applied by k_smallest.  boxes: as in brute_triangles, with the
    reference's 9999 as the limit."""
    if boxes:
        tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
        lookup = np.asarray(buf["tri_lookup"], F)
        out = [(np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, np.int64), np.zeros(0, np.int64))]
        for bi, (slots, mask) in reach(buf, o, d, F(9999.0)).items():
            if not slots.size:
                continue
            prim_of = np.array([min(u32f(lookup[s]), tris.shape[0] - 1) for s in slots], np.int64)
            prims = np.unique(prim_of)
            pm = np.stack([mask[:, prim_of == p].any(axis=1) for p in prims], axis=1)
            q = triangle_terms(np.asarray(buf["blas"], F).reshape(-1, 20)[bi], tris[prims], o, d)
            ray, tri = np.nonzero(q["ok"] & pm)
            out.append((ray, q["t"][ray, tri], np.full(ray.size, bi), prims[tri]))
        return tuple(np.concatenate(c) for c in zip(*out))
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    lookup = np.asarray(buf["tri_lookup"], F)
    n = o.shape[0]
    out = []
    for bi in np.unique(np.asarray(buf["blas_lookup"], np.int64).clip(0, blas.shape[0] - 1)):
        m = np.broadcast_to(blas[bi], (n, 20))
        oo, od = mat_apply(m, o, 1.0), mat_apply(m, d, 0.0)
        prims = np.unique(np.minimum(lookup[blas_slots(buf, blas[bi, 16])].astype(np.int64), tris.shape[0] - 1))
        A, B, C = tris[prims, 0:3], tris[prims, 12:15], tris[prims, 24:27]
        e1, e2 = (B - A)[None], (C - A)[None]
        for s0 in range(0, n, 256):
            odc, ooc = od[s0:s0 + 256, None, :], oo[s0:s0 + 256, None, :]
            shape = (odc.shape[0],) + e2.shape[1:]
            rce2 = cross(np.broadcast_to(odc, shape), np.broadcast_to(e2, shape))
            det = dot(e1, rce2)
            s = ooc - A[None]
            u = dot(s, rce2)
            sce1 = cross(s, np.broadcast_to(e1, s.shape))
            v = dot(np.broadcast_to(odc, s.shape), sce1)
            t = (F(1.0) / det) * dot(np.broadcast_to(e2, s.shape), sce1)
            ok = ~(det < F(0.00001)) & ~((u < 0) | (u > det)) & ~((v < 0) | (u + v > det))
            ray, tri = np.nonzero(ok)
            out.append((ray + s0, t[ray, tri], np.full(ray.size, bi), prims[tri]))
    return tuple(np.concatenate(c) for c in zip(*out))


def k_smallest(n, k, cand, tmin, tmax):
    """Per ray the k smallest (t, instance, prim) among `cand` with tmin < t < tmax: (n, k) t / instance / prim (-1 where there
    are fewer), and the number of accepted hits per ray before the cut."""
    ray, t, inst, prim = cand
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    keep = (t > tmin[ray]) & (t < tmax[ray])
    ray, t, inst, prim = ray[keep], t[keep], inst[keep], prim[keep]
    order = np.lexsort((prim, inst, t, ray))
    ray, t, inst, prim = ray[order], t[order], inst[order], prim[order]
    total = np.bincount(ray, minlength=n)
    rank = np.arange(ray.size) - (np.cumsum(total) - total)[ray]
    cut = rank < k
    T, I, P = np.full((n, k), -1.0, F), np.full((n, k), -1, np.int32), np.full((n, k), -1, np.int32)
    T[ray[cut], rank[cut]], I[ray[cut], rank[cut]], P[ray[cut], rank[cut]] = t[cut], inst[cut], prim[cut]
    return T, I, P, total


# ---- spheres: rt_oracle_np._trace with per-ray limits, and every sphere's near root ---------------------------------------------
def trace_spheres(sp, o, d, tmin, tmax):
    """RK:311-322 over the spheres with hitSphere (HK:307-331) in float32, tMin = tmin, the running nearest starting at tmax."""
    n = o.shape[0]
    ox, oy, oz, dx, dy, dz = (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])
    def _dot(ax, ay, az, bx, by, bz):
        return (ax * bx + ay * by) + az * bz
    nearest = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,))
    idx = np.full(n, -1, np.int64)
    a = _dot(dx, dy, dz, dx, dy, dz)
    for i in range(sp.shape[0]):
        cx, cy, cz, radius = sp[i, 0], sp[i, 1], sp[i, 2], sp[i, 7]
        ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
        b = F(2.0) * _dot(dx, dy, dz, ocx, ocy, ocz)
        c = _dot(ocx, ocy, ocz, ocx, ocy, ocz) - radius * radius
        disc = b * b - F(4.0) * a * c
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / (F(2.0) * a)
            hit = (disc > 0) & (t > tmin) & (t < nearest)
        nearest = np.where(hit, t, nearest)
        idx = np.where(hit, i, idx)
    return nearest, idx


def brute_spheres(sp, o, d, tmin, tmax, k):
    """trace_spheres' per-sphere t (HK:308-317) in float32; accepted: disc > 0 and tmin < t < tmax; the k smallest (t, index)."""
    n = o.shape[0]
    ox, oy, oz, dx, dy, dz = (c[:, None] for c in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    def _dot(ax, ay, az, bx, by, bz):
        return (ax * bx + ay * by) + az * bz
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,))[:, None]
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))[:, None]
    a = _dot(dx, dy, dz, dx, dy, dz)
    cx, cy, cz, radius = sp[None, :, 0], sp[None, :, 1], sp[None, :, 2], sp[None, :, 7]
    ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
    b = F(2.0) * _dot(dx, dy, dz, ocx, ocy, ocz)
    c = _dot(ocx, ocy, ocz, ocx, ocy, ocz) - radius * radius
    disc = b * b - F(4.0) * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-b - np.sqrt(disc)) / (F(2.0) * a)
        hit = (disc > 0) & (t > tmin) & (t < tmax)
    key = np.where(hit, t, F(np.inf))
    idx = np.argsort(key, axis=1, kind="stable")[:, :k]            # (stable: the lower index first on equal t)
    if idx.shape[1] < k:
        idx = np.concatenate([idx, np.zeros((n, k - idx.shape[1]), idx.dtype)], axis=1)
    rows = np.arange(n)[:, None]
    found = hit[rows, idx] & (np.arange(k)[None, :] < sp.shape[0])
    return np.where(found, t[rows, idx], F(-1.0)).astype(F), np.where(found, idx, -1).astype(np.int32)


# ---- multi-hit records ----------------------------------------------------------------------------------------------------------
def host_multi(r, rays, flags, k):
    """rt_trace_rays_multi_host into a buffer of junk: (n, k) records, every one of them written."""
    hits = np.zeros((rays.shape[0], k), dtype=abi.HIT_DTYPE)
    hits.view(np.uint8)[...] = 0x5A
    abi.check(r._lib.rt_trace_rays_multi_host(r._ctx, rays.ctypes.data, rays.shape[0], flags, k, hits.ctypes.data), r._ctx)
    return hits


def check_order(h, tmin, tmax):
    """Strictly ascending (t, instance, prim) -- hence distinct -- and tmin < t < tmax."""
    filled = h["prim"] >= 0
    a, b = h[:, :-1], h[:, 1:]
    both = filled[:, 1:]
    before = (a["t"] < b["t"]) | ((a["t"] == b["t"]) & ((a["instance"] < b["instance"]) |
                                                      ((a["instance"] == b["instance"]) & (a["prim"] < b["prim"]))))
    assert np.all(before[both]), "records out of order or repeated on %d rays" % int((~before & both).any(axis=1).sum())
    lo = np.broadcast_to(np.asarray(tmin, F).reshape(-1, 1), h.shape)
    hi = np.broadcast_to(np.asarray(tmax, F).reshape(-1, 1), h.shape)
    assert np.all(h["t"][filled] > lo[filled]) and np.all(h["t"][filled] < hi[filled])


# ---- every query family against its reference, for one scene state ---------------------------------------------------------------
MISS = np.zeros(1, dtype=abi.HIT_DTYPE)
MISS["t"], MISS["prim"], MISS["instance"] = -1.0, -1, -1


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _limits(first, seed):
    """Per-ray (tmin, tmax) from the oracle's unrestricted first hit `first` (-1: none): about a third of the rays get a tmin at or
    just beyond that hit (the hit itself is then excluded: t > tmin), the rest the reference's 0.001; about half a finite tmax on
    either side of the hit, the rest the reference's 9999."""
    rng = np.random.default_rng(seed)
    n = first.shape[0]
    hit = first > 0
    base = np.where(hit, first, F(5.0)).astype(F)
    pick = rng.integers(0, 6, n)
    beyond = np.where(pick == 0, base, (base * F(1.0 + 2.0 ** -10)).astype(F))
    tmin = np.where(pick < 2, beyond, F(0.001)).astype(F)
    tmax = np.where(rng.random(n) < 0.5, (base * rng.uniform(0.5, 3.0, n).astype(F)).astype(F), F(9999.0)).astype(F)
    return tmin, tmax


def _check_sphere_nearest(oracle, sp, o, d, h, tmin, tmax, ref=None):
    """The sphere comparison of test_spheres_against_the_oracle, under per-ray limits: prim and t against the oracle's loop
    (`ref`: its (nearest, index) where the caller has them), the rest of the record, and a sample of the hits against
    oracle.hit_sphere (the normal)."""
    with np.errstate(all="ignore"):
        nearest, idx = trace_spheres(sp, o, d, tmin, tmax) if ref is None else ref
    miss = idx < 0
    assert np.array_equal(h["prim"], np.where(miss, -1, idx).astype(np.int32)), "prim differs from the oracle on %d rays" % int(
        (h["prim"] != np.where(miss, -1, idx)).sum())
    assert same(h["t"], np.where(miss, F(-1.0), nearest)), "t differs from the oracle on %d rays" % int(
        (bits(h["t"]) != bits(np.where(miss, F(-1.0), nearest))).sum())
    assert np.all(h["instance"] == -1) and np.all(h["u"] == 0) and np.all(h["v"] == 0) and np.all(h["normal"][miss] == 0)
    hit = np.nonzero(~miss)[0]
    lo, hi = np.broadcast_to(np.asarray(tmin, F), idx.shape), np.broadcast_to(np.asarray(tmax, F), idx.shape)
    for i in hit[:: max(1, hit.size // 100)]:
        ok, t, nrm = oracle.hit_sphere(o[i], d[i], sp[h["prim"][i]], lo[i], hi[i])
        assert ok and same(t, h["t"][i]) and same(nrm, h["normal"][i])
    return int(hit.size)


def check_all_queries(oracle, r, state, rays, differ=differ, boxes=False):
    """Every query family of renderer `r` against the scene state the host holds now, bit for bit.  state: {"tri": the triangle
    buffers (tri_buffers(scene, mat))} or {"spheres": the (n, 8) records}, plus "params" (scene.pack_params of the renderer's
    maxBounces) and "faces" (the sky's); rays: (origins, directions), each (n, 3).  The shaded query and pick take the camera rays
    of the renderer's own frame (a shaded ray stands for a pixel only with the direction the frame itself forms).  Returns the
    number of `rays` that hit.  differ: the rule float words are compared by (bits unless given); boxes: the brute forces count
    only what the walk's box tests let it reach (brute_triangles)."""
    same = lambda a, b: _same(a, b, differ)
    o, d = (np.ascontiguousarray(a, F) for a in rays)
    n = o.shape[0]
    params = np.asarray(state["params"], F)
    W, H = r.width, r.height
    tri = "tri" in state
    buf = state.get("tri")
    sp = None if tri else np.asarray(state["spheres"], F).reshape(-1, 8)

    # trace_rays (the first call also carries the host's state to the context: recalculateScene)
    near = r.trace_rays(o, d)
    if tri:
        hits = check_triangle_hits(oracle, buf, o, d, near, differ)
        first = oracle.trace_tri_rays(buf, o, d)
    else:
        with np.errstate(all="ignore"):
            nearest, idx = rt_oracle_np._trace(sp, o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])
        first = np.where(idx < 0, F(-1.0), nearest).astype(F)
        hits = _check_sphere_nearest(oracle, sp, o, d, near, F(0.001), F(9999.0), ref=(nearest, idx))

    # trace_rays with limits against the float32 brute force; occluded == the limited query reports a hit
    tmin, tmax = _limits(first, 5)
    lim = r.trace_rays(o, d, tmin=tmin, tmax=tmax)
    found = lim["prim"] >= 0
    if tri:
        with np.errstate(all="ignore"):
            best = brute_triangles(buf, o, d, tmin, tmax, boxes)
            t, u, v, nrm = restate_triangle_hits(buf, o[found], d[found], lim["prim"][found], lim["instance"][found])
        assert np.array_equal(found, np.isfinite(best)), "the limited query and the brute force disagree on %d rays" % int(
            (found != np.isfinite(best)).sum())
        assert same(lim["t"], np.where(found, best, F(-1.0))), "limited t differs from the brute force on %d rays" % int(
            differ(lim["t"], np.where(found, best, F(-1.0))).sum())
        assert same(t, lim["t"][found]) and same(u, lim["u"][found]) and same(v, lim["v"][found]) and same(nrm, lim["normal"][found])
        assert np.all(lim["instance"][~found] == -1) and np.all(lim["u"][~found] == 0) and np.all(lim["v"][~found] == 0)
        assert np.all(lim["normal"][~found] == 0) and np.all(lim["instance"][found] >= 0)
    else:
        _check_sphere_nearest(oracle, sp, o, d, lim, tmin, tmax)
    assert np.all(lim["t"][found] > tmin[found]) and np.all(lim["t"][found] < tmax[found])
    occ = r.occluded(o, d, tmin, tmax)
    assert occ.dtype == bool and np.array_equal(occ, found), "occlusion differs from the limited query on %d rays" % int((occ != found).sum())

    # trace_rays_multi, k = 3 and 6 (the K = 4 and K = 8 lists below capacity): the brute force's k smallest, hit 0 the nearest query
    if tri:
        with np.errstate(all="ignore"):
            cand = all_triangle_hits(buf, o, d, boxes)
    for k in (3, 6):
        h = host_multi(r, pack(o, d), 0, k)
        filled = h["prim"] >= 0
        assert np.array_equal(filled, np.arange(k)[None, :] < filled.sum(axis=1)[:, None]), "a miss record precedes a hit"
        assert np.array_equal(_words(h[~filled]), _words(np.broadcast_to(MISS, (int((~filled).sum()),)))), "an unused place is not the miss record"
        check_order(h, F(0.001), F(9999.0))
        if tri:
            with np.errstate(all="ignore"):
                T, I, P, _ = k_smallest(n, k, cand, F(0.001), F(9999.0))
                ray, j = np.nonzero(filled)
                g = h[ray, j]
                t, u, v, nrm = restate_triangle_hits(buf, o[ray], d[ray], g["prim"], g["instance"])
            assert same(t, g["t"]) and same(u, g["u"]) and same(v, g["v"]) and same(nrm, g["normal"])
        else:
            if sp.shape[0]:
                with np.errstate(all="ignore"):
                    T, P = brute_spheres(sp, o, d, F(0.001), F(9999.0), k)
            else:                                                   # no sphere: every place is the miss record
                T, P = np.full((n, k), -1.0, F), np.full((n, k), -1, np.int32)
            I = np.full((n, k), -1, np.int32)
            assert np.all(h["u"] == 0) and np.all(h["v"] == 0)
            assert np.array_equal(h["prim"][:, 0], near["prim"])            # (the lowest index wins a tie in both)
        bad = (h["prim"] != P) | (h["instance"] != I) | differ(h["t"], T)
        assert not bad.any(), "k = %d: the walk and the brute force differ on %d rays, first %s" % (
            k, int(bad.any(axis=1).sum()), np.nonzero(bad.any(axis=1))[0][:5])
        assert same(h["t"][:, 0], near["t"]) and np.array_equal(h["prim"][:, 0] >= 0, near["prim"] >= 0)

    # shade_rays with compose: every camera ray of the frame against the oracle's float frame (the skipped share is zero)
    oc, dc = shade_common.camera_rays(params, W, H)
    if tri:
        ref_rgb = oracle.render_tri(params, buf, state["faces"], W, H, want_float=True)[1]
    else:
        ref_rgb = oracle.render(params, sp, state["faces"], W, H, want_float=True)[1]
    got = r.shade_rays(oc, dc, compose=True)
    diff = differ(got[:, 0:3], ref_rgb.reshape(-1, 3)).any(axis=-1)
    assert not diff.any(), "%d of %d shaded camera rays differ from the oracle's float frame" % (int(diff.sum()), W * H)
    if not tri and sp.shape[0] == 0:                                # the empty scene: the sky along the ray as given, dist 0
        sky = shade_common.OracleRays(oracle, params, sp, state["faces"]).sky(dc[::7])
        assert same(r.shade_rays(oc[::7], dc[::7])[:, 0:3], F(params[20]) * sky) and np.all(got[:, 3] == 0)

    # pick: every 7th pixel in both directions
    ys, xs = np.mgrid[0:H:7, 0:W:7]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    p = r.pick(xs, ys)
    dirs = np.stack([oracle.ray_dir(params, W, H, int(x), int(y)) for x, y in zip(xs, ys)])
    orig = np.broadcast_to(params[0:3], dirs.shape).astype(F)
    if tri:
        check_triangle_hits(oracle, buf, orig, dirs, p, differ)
    else:
        _check_sphere_nearest(oracle, sp, orig, dirs, p, F(0.001), F(9999.0))
    return hits
