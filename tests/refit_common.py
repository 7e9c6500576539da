"""Shared by the deforming-mesh tests (test infrastructure; tests/test_refit_tri_cpu.py, tests/test_refit_tri_gpu.py):
rt_refit_plan through the C ABI, the refit restated in numpy float32, the two deformations, and hand-made bad trees."""
import ctypes

import numpy as np

from compute_raytracer_amd import abi

F = np.float32
FP = ctypes.POINTER(ctypes.c_float)
U32 = ctypes.POINTER(ctypes.c_uint32)
HUGE = F(1e30)                                       # acceleration/bvh.py: fit's starting values


def u32f(f):
    """WGSL u32(f32): truncating, saturating, NaN -> 0"""
    f = float(f)
    if not f > 0.0:
        return 0
    return 4294967295 if f >= 4294967040.0 else int(f)


def refit_plan(nodes, n_tri_lookup, roots, cap=None):
    """rt_refit_plan -> (status, n_plan, (n_plan, 3) uint32 triples {node, first_slot, n_slots}); cap: room offered (None: enough)"""
    L = abi.load()
    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 8)
    roots = np.ascontiguousarray(roots, np.uint32).reshape(-1)
    cap = nodes.shape[0] if cap is None else cap
    plan = np.full((max(cap, 1), 3), 0xFFFFFFFF, np.uint32)
    n = ctypes.c_uint32(12345)
    rc = L.rt_refit_plan(nodes.ctypes.data_as(FP), nodes.shape[0], int(n_tri_lookup), roots.ctypes.data_as(U32), roots.shape[0],
                         plan.ctypes.data_as(U32), cap, ctypes.byref(n))
    return rc, n.value, (plan[:n.value].copy() if rc == abi.RT_OK else plan[:0])


def corners_by_slot(triangles, tri_lookup):
    """(slots, 3 corners, 3) float32: what the library's corner array holds (rt_triangles.hip: tri_corners)"""
    tris = np.asarray(triangles, F).reshape(-1, 40)
    idx = np.array([min(u32f(v), tris.shape[0] - 1) for v in np.asarray(tri_lookup, F)], np.int64)
    return np.stack([tris[idx, 0:3], tris[idx, 12:15], tris[idx, 24:27]], axis=1)


def numpy_refit(nodes, triangles, tri_lookup, plan):
    """The node buffer with the box of every planned node recomputed: per axis np.fmin / np.fmax (a NaN corner is skipped) over
    the three float32 corners of every slot of the node's run, from +-float32(1e30).  Words 3 and 7 and every other node are
    the input's."""
    out = np.array(nodes, F).reshape(-1, 8).copy()
    c = corners_by_slot(triangles, tri_lookup)
    for node, first, n in np.asarray(plan, np.int64):
        run = c[first:first + n].reshape(-1, 3)
        out[node, 0:3] = np.fmin.reduce(run, axis=0, initial=HUGE)
        out[node, 4:7] = np.fmax.reduce(run, axis=0, initial=-HUGE)
    return out


def tree_by_hand(nodes, root):
    """An independent walk (recursion over Python sets): {node: set of lookup slots of the leaves below it} under `root`"""
    nodes = np.asarray(nodes, F).reshape(-1, 8)
    out = {}
    todo = [(root, False)]
    while todo:
        i, done = todo.pop()
        left, count = u32f(nodes[i, 3]), u32f(nodes[i, 7])
        if count:
            out[i] = set(range(left, left + count))
        elif done:
            out[i] = out[left] | out[left + 1]
        else:
            assert i not in out
            todo += [(i, True), (left, False), (left + 1, False)]
    return out


# ---- the scene of the pixel tests: frames of 64 x 48, a few hundred triangles ----
W, H, B = 64, 48, 2


def view_scene(n_models=3):
    """helpers.triangle_scene: two tessellated spheres (96 and 176 triangles) instanced n_models times, and a floor"""
    from helpers import triangle_scene
    return triangle_scene(seed=40, n_models=n_models)


# ---- the two deformations, applied to the vertices of one mesh in numpy float32 ----
CORNER_COLS = (slice(0, 3), slice(12, 15), slice(24, 27))


def deform(triangles, first, count, kind, phase=0.0):
    """(T, 40) float32 records with the corners of triangles [first, first + count) moved: "grow" scales the mesh by 1.5 about its
    centroid and adds a sine displacement -- it leaves its old boxes --, "shrink" scales it by 0.6 -- it stays inside them.  A
    vertex shared by several triangles moves to the same place in each."""
    t = np.array(triangles, F).reshape(-1, 40).copy()
    v = np.stack([t[first:first + count, c] for c in CORNER_COLS], axis=1)            # (count, 3, 3)
    c = v.reshape(-1, 3).mean(axis=0, dtype=np.float64).astype(F)
    if kind == "grow":
        w = c + F(1.5) * (v - c) + F(0.15) * np.sin(F(3.0) * v[..., [1, 2, 0]] + F(phase)).astype(F)
    elif kind == "shrink":
        w = c + F(0.6) * (v - c)
    else:
        raise ValueError(kind)
    w = w.astype(F)
    for k, cols in enumerate(CORNER_COLS):
        t[first:first + count, cols] = w[:, k]
    return t


def mesh_ranges(scene):
    """[(root node, first triangle, triangle count)] per mesh of a scene made by createTriangleScene"""
    return [(m.root_node, m.lookup_offset, m.soup.count) for m in scene.meshes]


# ---- hand-made trees: node buffers of (n, 8) float32 with a lookup table of LOOKUP slots ----
LOOKUP = 5


def _nodes(rows):
    n = np.zeros((len(rows), 8), F)
    for i, (left, count) in enumerate(rows):
        n[i] = [-1, -1, -1, left, 1, 1, 1, count]
    return n


def good_tree():
    """0: inner (1, 2); 1: leaf slots [0, 2); 2: inner (3, 4); 3: leaf [2, 3); 4: leaf [3, 5)"""
    return _nodes([(1, 0), (0, 2), (3, 0), (2, 1), (3, 2)])


def bad_trees():
    """name -> (nodes, roots, expected status)"""
    inv, uns = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_UNSUPPORTED
    cases = {}
    t = good_tree(); t[2, 3] = 4                       # children 4 and 5: 5 is beyond the buffer
    cases["child beyond the buffer"] = (t, [0], inv)
    t = good_tree(); t[2, 3] = 4294967295.0            # left + 1 wraps in 32 bits
    cases["child index saturates"] = (t, [0], inv)
    t = good_tree(); t[4, 7] = 3                       # slots [3, 6) of 5
    cases["leaf run beyond the lookup table"] = (t, [0], inv)
    cases["node shared by two parents"] = (_nodes([(1, 0), (3, 0), (3, 0), (0, 2), (2, 3)]), [0], inv)
    t = good_tree(); t[2, 3] = 0                       # node 2's children are 0 and 1: back to the root
    cases["cycle"] = (t, [0], inv)
    cases["two roots sharing a subtree"] = (good_tree(), [0, 2], inv)
    cases["root beyond the buffer"] = (good_tree(), [5], inv)
    cases["right run before the left with a gap"] = (_nodes([(1, 0), (3, 2), (0, 2)]), [0], uns)
    return cases
