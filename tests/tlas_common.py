"""Shared by the device-top-level-build tests (test infrastructure; tests/test_build_tlas_cpu.py, tests/test_build_tlas_gpu.py):
rt_build_tlas_host through the C ABI, an independent numpy restatement of what it must compute (instances.invert_mat4 and
world_boxes, the pad, and a short SAH over primitives written from the rule list at the top of csrc/rt_blas_build.h), synthetic
instance sets, the scenes of the no-lost-hit test and the rays they are tried with."""
import ctypes

import numpy as np

from compute_raytracer_amd import abi
from compute_raytracer_amd.instances import invert_mat4, world_boxes
from refit_common import F, FP, U32, u32f

HUGE = F(1e30)
PAD = F(2.0 ** -16)
SIZES_CPU = (1, 2, 3, 16, 17, 65, 300)
SIZES_GPU = (1, 2, 3, 16, 17, 64, 65, 257, 300)      # the per-frame path's edge at 16 / 17, the wave's at 64 / 65, kBuildShort's at 256 / 257


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- rt_build_tlas_host ----
SENTINEL = F(-7.5)


def build_host(models, roots, nodes, node_cap):
    """rt_build_tlas_host -> (status, tlas (node_cap, 8), blas (n, 20), lookup (n,), info dict); the outputs start as SENTINEL"""
    L = abi.load()
    m = np.ascontiguousarray(models, F).reshape(-1, 16)
    r = np.ascontiguousarray(roots, np.uint32).reshape(-1)
    nd = np.ascontiguousarray(nodes, F).reshape(-1, 8)
    n = r.shape[0]
    tlas, blas, lookup = np.full((max(node_cap, 1), 8), SENTINEL, F), np.full((max(n, 1), 20), SENTINEL, F), np.full(max(n, 1), SENTINEL, F)
    info = abi.RtTlasInfo(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    rc = L.rt_build_tlas_host(m.ctypes.data_as(FP), r.ctypes.data_as(U32), n, nd.ctypes.data_as(FP), nd.shape[0], tlas.ctypes.data_as(FP),
                              blas.ctypes.data_as(FP), lookup.ctypes.data_as(FP), int(node_cap), ctypes.byref(info))
    return rc, tlas[:node_cap], blas[:n], lookup[:n], info_dict(info)


def info_dict(info):
    return dict(nodes_used=int(info.nodes_used), depth=int(info.depth), leaves=int(info.leaves), max_leaf=int(info.max_leaf))


def untouched(*arrays):
    return all((bits(a) == bits(SENTINEL)).all() for a in arrays)


# ---- the restatement ----
def numpy_records(models, roots):
    m = np.ascontiguousarray(models, F).reshape(-1, 16)
    rec = np.zeros((m.shape[0], 20), F)
    rec[:, 0:16] = invert_mat4(m)
    rec[:, 16] = np.asarray(roots, np.float64).astype(F)
    return rec


def numpy_prims(models, roots, nodes):
    """(lo, hi, centre), each (n, 3) float32: the padded world boxes"""
    rec = np.asarray(nodes, F).reshape(-1, 8)[np.asarray(roots, np.int64)]
    lo, hi, _ = world_boxes(np.asarray(models, F).reshape(-1, 16), rec[:, 0:3], rec[:, 4:7])
    lo, hi = lo.astype(F), hi.astype(F)
    m = np.maximum(np.abs(lo).max(axis=1), np.abs(hi).max(axis=1)).astype(F)
    pad = (m * PAD).astype(F)
    lo, hi = (lo - pad[:, None]).astype(F), (hi + pad[:, None]).astype(F)
    return lo, hi, ((lo + hi).astype(F) * F(0.5)).astype(F)


def _area(lo, hi):
    e = [float(F(hi[a]) - F(lo[a])) for a in range(3)]
    return 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])


def _side(lo, hi, ids):
    if len(ids) == 0:
        return np.full(3, HUGE, F), np.full(3, -HUGE, F)
    return np.minimum(lo[ids].min(axis=0), HUGE).astype(F), np.maximum(hi[ids].max(axis=0), -HUGE).astype(F)


def numpy_sah(lo, hi, cen):
    """The rules at the top of rt_blas_build.h over primitives {lo, hi, cen}: nine planes per axis at tenths of the node's box
    (float64), a primitive goes left when its centroid is below the plane, cost = areaL nL + areaR nR, the first strict minimum in
    (axis, plane) order below 1e30; a leaf when fewer than two, when staying is cheaper, when a side would be empty or when no
    cost is below 1e30; a stable partition; children numbered in preorder, the left subtree first.
    -> ((used, 8) float32 nodes rooted at 0, (n,) order, info dict)"""
    n = lo.shape[0]
    order = np.arange(n, dtype=np.int64)
    blo, bhi = _side(lo, hi, order)
    nodes = [[blo, 0, bhi, n]]                      # [lo, first, hi, count] until a split rewrites first / count
    depth_of = {0: 0}
    todo = [0]
    info = dict(nodes_used=0, depth=0, leaves=0, max_leaf=0)
    while todo:
        i = todo.pop()
        nlo, first, nhi, count = nodes[i]
        info["depth"] = max(info["depth"], depth_of[i])
        run = order[first:first + count].copy()
        best, choice = 1e30, None
        if count >= 2:
            for axis in range(3):
                c = cen[run, axis].astype(np.float64)
                for s in range(1, 10):
                    f = s / 10.0
                    plane = float(nlo[axis]) * (1.0 - f) + float(nhi[axis]) * f
                    left = c < plane
                    l, r = run[left], run[~left]
                    llo, lhi = _side(lo, hi, l)
                    rlo, rhi = _side(lo, hi, r)
                    cost = (0.0 + _area(llo, lhi) * float(len(l))) + _area(rlo, rhi) * float(len(r))
                    if cost < best:
                        best, choice = cost, (left, (llo, lhi), (rlo, rhi))
        leaf = choice is None or _area(nlo, nhi) * float(count) < best or choice[0].sum() in (0, count)
        if leaf:
            info["leaves"] += 1
            info["max_leaf"] = max(info["max_leaf"], count)
            continue
        left, (llo, lhi), (rlo, rhi) = choice
        n_left = int(left.sum())
        order[first:first + count] = np.concatenate([run[left], run[~left]])
        child = len(nodes)
        nodes[i] = [nlo, child, nhi, 0]
        nodes.append([llo, first, lhi, n_left])
        nodes.append([rlo, first + n_left, rhi, count - n_left])
        depth_of[child] = depth_of[child + 1] = depth_of[i] + 1
        todo += [child + 1, child]
    out = np.zeros((len(nodes), 8), F)
    for i, (nlo, first, nhi, count) in enumerate(nodes):
        out[i, 0:3], out[i, 3], out[i, 4:7], out[i, 7] = nlo, first, nhi, count
    info["nodes_used"] = len(nodes)
    return out, order, info


def numpy_tlas(models, roots, nodes, node_cap):
    """what rt_build_tlas_host must store -> (tlas (node_cap, 8), blas, lookup, info)"""
    lo, hi, cen = numpy_prims(models, roots, nodes)
    tree, order, info = numpy_sah(lo, hi, cen)
    tlas = np.zeros((node_cap, 8), F)
    tlas[:tree.shape[0]] = tree
    return tlas, numpy_records(models, roots), order.astype(F), info


# ---- synthetic instance sets: K root records behind node_cap top-level nodes, n instances of them ----
def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def synthetic(n, seed, kinds=5, spread=12.0):
    """-> (models (n, 16), roots (n,), nodes, node_cap): rotations about any axis with scales 0.3 .. 2.5 and translations within
    `spread`; every seventh matrix has a projective bottom row (w != 1 at the corners)"""
    rng = np.random.default_rng(seed)
    node_cap = 2 * n - 1
    nodes = np.zeros((node_cap + kinds, 8), F)
    c = rng.uniform(-1.0, 1.0, (kinds, 3))
    e = rng.uniform(0.0, 1.5, (kinds, 3))
    e[0, 1] = 0.0                                                        # a flat one: zero height
    nodes[node_cap:, 0:3], nodes[node_cap:, 4:7] = c - e, c + e
    nodes[node_cap:, 3], nodes[node_cap:, 7] = 0.0, 2.0
    models = np.zeros((n, 4, 4))
    for i in range(n):
        models[i, :3, :3] = rotation(rng) * rng.uniform(0.3, 2.5)
        models[i, :3, 3] = rng.uniform(-spread, spread, 3)
        models[i, 3, 3] = 1.0
        if i % 7 == 6:
            models[i, 3, :3] = rng.uniform(-0.01, 0.01, 3)
    models = models.transpose(0, 2, 1).reshape(n, 16).astype(F)          # column-major
    roots = (node_cap + rng.integers(0, kinds, n)).astype(np.uint32)
    return models, roots, nodes, node_cap


def translations(xs, half=0.5):
    """cubes of half-width `half` at the given x: (models, roots, nodes, node_cap) with one root record {-half .. half}"""
    n = len(xs)
    node_cap = 2 * n - 1
    nodes = np.zeros((node_cap + 1, 8), F)
    nodes[node_cap, 0:3], nodes[node_cap, 4:7], nodes[node_cap, 7] = -half, half, 1.0
    models = np.zeros((n, 16), F)
    models[:, [0, 5, 10, 15]] = 1.0
    models[:, 12] = np.asarray(xs, np.float64).astype(F)
    return models, np.full(n, node_cap, np.uint32), nodes, node_cap


SPINE_HALF = 2.0 ** -50


def spine_xs(n=23):
    """x = 11^(i - 12), i = 0 .. n - 1, for cubes of half-width SPINE_HALF: each split peels the farthest one off
    (tests/test_build_tlas_cpu.py confirms it).  UNIT boxes at these x do not make a spine: the six nearest the origin overlap
    and stay one leaf (17 levels); and cubes at 11^i alone cost more than the builder's 1e30 bound and stay one leaf of all."""
    return [11.0 ** (i - 12) for i in range(n)]


# ---- walking a built top level ----
def walk(tlas):
    """-> [(leaf node, [ancestors .. leaf], first, count)] from node 0, checking every node is reached once"""
    tlas = np.asarray(tlas, F).reshape(-1, 8)
    out, seen, todo = [], set(), [(0, [0])]
    while todo:
        i, path = todo.pop()
        assert 0 <= i < tlas.shape[0] and i not in seen, "node %d reached twice or beyond the buffer" % i
        seen.add(i)
        left, count = u32f(tlas[i, 3]), u32f(tlas[i, 7])
        if count:
            out.append((i, path, left, count))
        else:
            todo += [(left + 1, path + [left + 1]), (left, path + [left])]
    return out, seen


def check_well_formed(tlas, lookup, n, used):
    leaves, seen = walk(tlas[:used])
    assert seen == set(range(used))
    cover = np.zeros(n, np.int64)
    for _, _, first, count in leaves:
        assert first + count <= n
        cover[first:first + count] += 1
    assert (cover == 1).all()
    assert np.array_equal(np.sort(np.asarray(lookup, F)), np.arange(n, dtype=F))
    assert not bits(tlas[used:]).any()


# ---- triangle scenes: the arguments of a build, and the buffers with the built top level in place of the reference's ----
def scene_args(scene, buf):
    """(models, roots, nodes, node_cap) of a createTriangleScene scene whose node buffer is buf["nodes"]"""
    roots = np.array([scene.meshes[k].root_node for k in scene.instances.mesh_index], np.uint32)
    return scene.instances.matrices(), roots, np.asarray(buf["nodes"], F), scene.tlasNodesMax


def with_top_level(buf, tlas, blas, lookup):
    out = dict(buf)
    nodes = np.array(buf["nodes"], F).copy()
    nodes[:tlas.shape[0]] = tlas
    out["nodes"], out["blas"], out["blas_lookup"] = nodes, np.asarray(blas, F), np.asarray(lookup, F)
    return out


def tight_buffers(scene, buf):
    """buf with the host model's top level -> (buffers, info)"""
    models, roots, nodes, cap = scene_args(scene, buf)
    rc, tlas, blas, lookup, info = build_host(models, roots, nodes, cap)
    assert rc == abi.RT_OK
    return with_top_level(buf, tlas, blas, lookup), info


def box_rays(lo, hi, lo_scene, hi_scene, n, seed):
    """n rays from random origins aimed at points ON the padded instance boxes (lo, hi: (M, 3)): a third at points of a face, a
    third at points of an edge, a third at corners"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, lo.shape[0], n)
    u = rng.random((n, 3))
    fixed = rng.integers(0, 2, (n, 3)).astype(np.float64)             # which bound a pinned axis takes
    kind = np.arange(n) % 3                                              # 0: a face (one axis pinned), 1: an edge (two), 2: a corner
    axis = rng.integers(0, 3, n)
    pinned = np.zeros((n, 3), bool)
    for a in range(3):
        pinned[:, a] = np.where(kind == 0, axis == a, np.where(kind == 1, axis != a, True))
    w = np.where(pinned, fixed, u)
    p = lo[k].astype(np.float64) * (1.0 - w) + hi[k].astype(np.float64) * w
    ext = np.asarray(hi_scene, np.float64) - np.asarray(lo_scene, np.float64)
    o = rng.uniform(np.asarray(lo_scene) - 0.5 * ext, np.asarray(hi_scene) + 0.5 * ext, (n, 3))
    return o.astype(F), (p - o).astype(F)
