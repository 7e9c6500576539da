"""Shared by the closest-point tests (test infrastructure; tests/test_closest_cpu.py, tests/test_closest_gpu.py): the definition of
include/rt355.h: rt_closest_points restated in numpy -- vectorised over the points, looped over every (instance, slot) pair, every
sum written out in the order of csrc/rt_closest.h (no `@`, no np.dot) --, rt_closest_points_model through the C ABI, the points
and radii the queries are tried with, and the scene variants."""
import ctypes

import numpy as np

from compute_raytracer_amd import abi
from compute_raytracer_amd.instances import invert_mat4
from query_common import blas_slots, u32f

F = np.float32
D = np.float64
ALL = 0xFFFFFFFF
RADII = (np.inf, 0.75, 0.0, -1.0, np.nan)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_records(a, b):
    """every field of two (n,) CLOSEST_DTYPE arrays, bit for bit -> the indices that differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape
    return np.nonzero((words(a).reshape(a.shape[0], -1) != words(b).reshape(b.shape[0], -1)).any(axis=1))[0]


def assert_same(got, want, what=""):
    bad = same_records(got, want)
    assert bad.size == 0, "%s: %d of %d records differ, first %d: got %s, want %s" % (
        what, bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])


# ---- the definition ----
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def leaf(p, A, B, C):
    """item 3: p (3 x (n,) float32 columns), A, B, C (3 float32 scalars each) -> float32 dist2, u, v, point (3 columns)"""
    q = [p[k].astype(D) for k in range(3)]
    a, b, c = ([D(X[k]) for k in range(3)] for X in (A, B, C))
    ab = [b[k] - a[k] for k in range(3)]
    ac = [c[k] - a[k] for k in range(3)]
    ap = [q[k] - a[k] for k in range(3)]
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = [q[k] - b[k] for k in range(3)]
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = [q[k] - c[k] for k in range(3)]
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    # interior
    denom = 1.0 / ((va + vb) + vc)
    u, v = vb * denom, vc * denom
    s = [(a[k] + ab[k] * u) + ac[k] * v for k in range(3)]
    # edge BC
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    u, v = np.where(m, 1.0 - w, u), np.where(m, w, v)
    s = [np.where(m, b[k] + w * (c[k] - b[k]), s[k]) for k in range(3)]
    # edge AC
    w = d2 / (d2 - d6)
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    u, v = np.where(m, zero, u), np.where(m, w, v)
    s = [np.where(m, a[k] + w * ac[k], s[k]) for k in range(3)]
    # vertex C
    m = (d6 >= 0) & (d5 <= d6)
    u, v = np.where(m, zero, u), np.where(m, one, v)
    s = [np.where(m, c[k], s[k]) for k in range(3)]
    # edge AB
    w = d1 / (d1 - d3)
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    u, v = np.where(m, w, u), np.where(m, zero, v)
    s = [np.where(m, a[k] + w * ab[k], s[k]) for k in range(3)]
    # vertex B
    m = (d3 >= 0) & (d4 <= d3)
    u, v = np.where(m, one, u), np.where(m, zero, v)
    s = [np.where(m, b[k], s[k]) for k in range(3)]
    # vertex A
    m = (d1 <= 0) & (d2 <= 0)
    u, v = np.where(m, zero, u), np.where(m, zero, v)
    s = [np.where(m, a[k], s[k]) for k in range(3)]
    e = [q[k] - s[k] for k in range(3)]
    return dot(e, e).astype(F), u.astype(F), v.astype(F), [s[k].astype(F) for k in range(3)]


def forward_matrices(buf):
    """item 2: Fm of every BLAS record, (n_blas, 16) float32"""
    return invert_mat4(np.asarray(buf["blas"], F).reshape(-1, 20)[:, 0:16])


def world_corners(buf):
    """{bi: (slots, prims, (S, 3 corners, 3) float32 world corners)} for every instance a top-level leaf names"""
    nodes = np.asarray(buf["nodes"], F).reshape(-1, 8)
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    look = np.asarray(buf["blas_lookup"], F).reshape(-1)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    tl = np.asarray(buf["tri_lookup"], F).reshape(-1)
    Fm = forward_matrices(buf).astype(D)
    named, todo = set(), [0]
    while todo:
        i = min(todo.pop(), nodes.shape[0] - 1)
        left, count = u32f(nodes[i, 3]), u32f(nodes[i, 7])
        if count == 0:
            todo += [left, left + 1]
        else:
            named |= {min(u32f(look[min(left + k, look.shape[0] - 1)]), blas.shape[0] - 1) for k in range(count)}
    out = {}
    for bi in sorted(named):
        slots = blas_slots(buf, u32f(blas[bi, 16]))
        prims = np.array([min(u32f(tl[s]), tris.shape[0] - 1) for s in slots], np.int64)
        obj = np.stack([tris[prims, 0:3], tris[prims, 12:15], tris[prims, 24:27]], axis=1).astype(D)      # (S, 3, 3)
        x, y, z = obj[..., 0], obj[..., 1], obj[..., 2]
        m = Fm[bi]
        w = np.stack([((m[k] * x + m[4 + k] * y) + m[8 + k] * z) + m[12 + k] for k in range(3)], axis=-1).astype(F)
        out[bi] = (slots, prims, w)
    return out


def brute(buf, points, masks=None, ray_mask=ALL):
    """items 1-5 over every pair: points (n, 4) float32 {x, y, z, radius} -> (n,) CLOSEST_DTYPE"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    n = pts.shape[0]
    p = [pts[:, k] for k in range(3)]
    radius = pts[:, 3]
    with np.errstate(all="ignore"):
        live = radius >= 0
        best = (radius * radius).astype(F)
    binst = np.full(n, 2 ** 31 - 1, np.int64)
    bprim = np.full(n, 2 ** 31 - 1, np.int64)
    out = np.zeros(n, dtype=abi.CLOSEST_DTYPE)
    out["dist2"], out["prim"], out["instance"] = -1.0, -1, -1
    masks = np.zeros(0, np.uint32) if masks is None else np.asarray(masks, np.uint32)
    with np.errstate(all="ignore"):
        for bi, (slots, prims, w) in world_corners(buf).items():
            mask = int(masks[bi]) if bi < masks.shape[0] else ALL
            if (mask & int(ray_mask)) == 0:
                continue
            for j in range(slots.shape[0]):
                d2, u, v, s = leaf(p, w[j, 0], w[j, 1], w[j, 2])
                prim = int(prims[j])
                take = live & ((d2 < best) | ((d2 == best) & ((bi < binst) | ((bi == binst) & (prim < bprim)))))
                if not take.any():
                    continue
                best = np.where(take, d2, best)
                binst = np.where(take, bi, binst)
                bprim = np.where(take, prim, bprim)
                out["dist2"][take], out["u"][take], out["v"][take] = d2[take], u[take], v[take]
                out["prim"][take], out["instance"][take] = prim, bi
                for k in range(3):
                    out["point"][take, k] = s[k][take]
    return out


def n_pairs(buf):
    return sum(slots.shape[0] for slots, _, _ in world_corners(buf).values())


# ---- rt_closest_points_model ----
def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def model(buf, points, masks=None, ray_mask=ALL, junk=True):
    """-> (status, (n,) CLOSEST_DTYPE, candidate tests); the output starts as junk, so every record must be written"""
    L = abi.load()
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    arr = {k: np.ascontiguousarray(buf[k], F) for k in ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")}
    shape = dict(triangles=40, tri_lookup=1, nodes=8, blas=20, blas_lookup=1)
    out = np.zeros(pts.shape[0], dtype=abi.CLOSEST_DTYPE)
    if junk:
        out.view(np.uint8)[...] = 0x5A
    m = None if masks is None else np.ascontiguousarray(masks, np.uint32)
    tests = ctypes.c_uint64(0xFFFF)
    rc = L.rt_closest_points_model(_ptr(pts), pts.shape[0], *[x for k in ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")
                                                              for x in (_ptr(arr[k]), arr[k].size // shape[k])],
                                   _ptr(m), 0 if m is None else m.shape[0], int(ray_mask), _ptr(out), ctypes.byref(tests))
    return rc, out, int(tests.value)


# ---- points ----
def scene_box(buf):
    """the box of every world corner, clipped to +-20 (the floor reaches further than the points need to)"""
    allw = np.concatenate([w.reshape(-1, 3) for _, _, w in world_corners(buf).values()]).astype(D)
    return np.maximum(allw.min(axis=0), -20.0), np.minimum(allw.max(axis=0), 20.0)


def make_points(buf, n, seed):
    """(n, 3) float32: uniform in the scene box grown by half; every fifth point exactly on a world corner of a random triangle; every
    tenth on the float32 midpoint of an edge of a random triangle (an edge two triangles of a mesh share)"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(buf)
    ext = hi - lo
    pts = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3)).astype(F)
    wc = world_corners(buf)
    keys = sorted(wc)
    for i in range(0, n, 5):
        _, _, w = wc[keys[int(rng.integers(len(keys)))]]
        pts[i] = w[int(rng.integers(w.shape[0])), int(rng.integers(3))]
    for i in range(3, n, 10):
        _, _, w = wc[keys[int(rng.integers(len(keys)))]]
        t, k = w[int(rng.integers(w.shape[0]))], int(rng.integers(3))
        pts[i] = ((t[k].astype(D) + t[(k + 1) % 3].astype(D)) * 0.5).astype(F)
    return pts


def with_radius(pts, radius):
    out = np.zeros((pts.shape[0], 4), F)
    out[:, 0:3] = pts
    out[:, 3] = radius
    return out


def mixed_radii(pts, seed):
    """every radius of RADII in turn, and a few drawn between 0 and 3"""
    rng = np.random.default_rng(seed)
    r = np.array([RADII[(i + i // 5) % len(RADII)] for i in range(pts.shape[0])], F)     # (a corner point takes each in turn too)
    pick = rng.random(pts.shape[0]) < 0.3
    r[pick] = rng.uniform(0.0, 3.0, int(pick.sum())).astype(F)
    return with_radius(pts, r)


# ---- scene variants ----
def shear_records(buf, which=(1, 3)):
    """buf with the FORWARD matrices of two instances given a non-uniform scale and a shear; their records are the inverses"""
    out = dict(buf)
    blas = np.array(buf["blas"], F).reshape(-1, 20).copy()
    fwd = invert_mat4(blas[:, 0:16]).astype(D).reshape(-1, 4, 4)          # [col][row]
    for j, bi in enumerate(which):
        lin = np.array([[1.4, 0.0, 0.0], [0.35, 0.6, 0.0], [-0.2, 0.45, 1.1 + 0.3 * j]])      # lin[col][row]: scale + shear
        m = fwd[bi].copy()
        m[0:3, 0:3] = np.stack([sum(lin[c][r] * fwd[bi][r, 0:3] for r in range(3)) for c in range(3)])
        blas[bi, 0:16] = invert_mat4(m.reshape(1, 16).astype(F))[0]
    out["blas"] = blas
    return out


def twin_scene():
    """a triangle scene whose instances 1 and 3 are the same mesh at the same place: identical BLAS records"""
    import compute_raytracer_amd as rt
    from compute_raytracer_amd.procedural import obj_floor, obj_uv_sphere
    meshes = [rt.load_mesh(obj_uv_sphere(6, 8, 1.0), dict(color=[0.9, 0.5, 0.3, 0.6], alignBottom=True, scale=1.0)),
              rt.load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 0.8], alignBottom=False, scale=12))]
    same = dict(meshIndex=0, position=[1.5, 0.0, -5.0], eulers=[0, 40.0, 0])
    models = [dict(meshIndex=0, position=[-2.0, 0.0, -6.0], eulers=[0, 10.0, 0]), dict(same),
              dict(meshIndex=1, position=[0, 0, -5], eulers=[0, 0, 0]), dict(same)]
    scene = rt.SceneRaytracing().createScene([]).createTriangleScene(meshes, models)
    return scene, rt.Material.white()
