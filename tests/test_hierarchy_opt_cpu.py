"""The reinsertion pass over the sphere hierarchy (rt_bvh_build.h: Builder::optimise; DESIGN.md 4.0 "Structure"), without a
GPU.  rt_build_hierarchy_ex builds the tree with a chosen number of passes (0: the top-down tree as built) and reports the
top-down node count and the cost of both trees.  Conditions, on the scenes of tests/test_hierarchy_cpu.py and on degenerate
inputs: the optimised tree keeps every invariant the walk relies on (check_tree), never has more nodes than the top-down
tree of the same input (the kernel form follows the node count; the pass in fact keeps the count), never costs more by its own objective -- the sum over
inner nodes of R^2 x children, recomputed here from the emitted records --, and is deterministic."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.scene_raytracing import synthetic_spheres

from helpers import FILTER_SCALE, LEAF, _members_f64, build_hierarchy, check_tree


def records(spheres):
    return np.ascontiguousarray(rt.SceneRaytracing().createScene(spheres).pack_spheres(), dtype=np.float32).reshape(-1, 8)


def build_ex(rec, passes):
    n = rec.shape[0]
    cap = 2 * n + 64
    out, link, nodes = np.zeros((cap, 4), np.float32), np.zeros(cap, np.uint32), ctypes.c_uint32(0)
    info = (ctypes.c_double * 4)()
    fp = ctypes.POINTER(ctypes.c_float)
    abi.check(abi.load().rt_build_hierarchy_ex(rec.ctypes.data_as(fp), n, out.ctypes.data_as(fp), link.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                               cap, ctypes.byref(nodes), passes, info))
    m = nodes.value
    return out[: m + 1].copy(), link[: m + 1].copy(), m, list(info)


def tree_cost(rec, out, link, m):
    """sum over inner nodes of R^2 x children, R the radius of the members about the centre the record stores (what bound()
    multiplies by sigma; taken from the members because the record's k loses R^2 against |C|^2 far from the origin)"""
    c, r = _members_f64(rec)
    cost = 0.0
    for i in range(m):
        if link[i] & LEAF:
            continue
        C = out[i, 0:3].astype(np.float64) / FILTER_SCALE
        kids, j, end = 0, i + 1, int(link[i]) // 4
        while j < end:
            kids += 1
            j = j + 1 if link[j] & LEAF else int(link[j]) // 4
        assert 2 <= kids <= 4
        members = link[i + 1: end][(link[i + 1: end] & LEAF) != 0] & 0x7FFFFFFF
        R = (np.linalg.norm(c[members] - C, axis=1) + r[members]).max()
        cost += R * R * kids
    return cost


def scenes():
    yield from (("baseline-%d" % n, synthetic_spheres(n, seed)) for n, seed in [(2, 1), (5, 2), (9, 3), (64, 357), (1024, 358), (4096, 360)])
    yield "coincident", [rt.Sphere([0, 1, -6], 1.0, [1, 0, 0])] * 7
    yield "coincident-200", [rt.Sphere([0, 1, -6], 1.0, [1, 0, 0])] * 200
    yield "nested", [rt.Sphere([0, 1, -6], 0.1 * 2 ** k, [0, 1, 0]) for k in range(9)]
    yield "collinear", [rt.Sphere([i * 0.5, 0, 0], 0.2, [0, 0, 1]) for i in range(37)]
    yield "collinear-growing", [rt.Sphere([1.3 ** i, 0, 0], 0.05 * 1.3 ** i, [0, 0, 1]) for i in range(60)]
    yield "points", [rt.Sphere([0, 0, 0], 0.0, [0, 0, 1]), rt.Sphere([1, 0, 0], 0.0, [0, 0, 1]), rt.Sphere([5, 5, 5], 1e-3, [1, 1, 1])]
    rng = np.random.default_rng(4)
    yield "huge-and-tiny", [rt.Sphere([0, -50, 0], 50.0, [1, 1, 1])] + [rt.Sphere(rng.normal(size=3), 1e-3, [1, 1, 1]) for _ in range(150)]
    for n in range(2, 10):
        yield "n-%d" % n, [rt.Sphere(rng.uniform(-3, 3, 3), float(rng.uniform(0.1, 0.6)), [1, 1, 1]) for _ in range(n)]
    for seed in range(12):
        rng = np.random.default_rng(seed)
        scale = 10 ** rng.uniform(-2, 4)
        off = rng.choice([0.0, 1e3, 1e5]) * rng.normal(size=3)
        n = int(rng.choice([6, 33, 300, 1500]))
        spheres = [rt.Sphere(off + rng.normal(size=3) * scale, scale * 10 ** rng.uniform(-3, -0.5), [1, 1, 1]) for _ in range(n)]
        if seed % 2:
            spheres.append(rt.Sphere(off + np.array([0, -60 * scale, 0]), 55 * scale, [1, 1, 1]))
        yield "random-%d" % seed, spheres


SCENES = list(scenes())


@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_optimised_tree_keeps_the_invariants_the_node_count_and_its_own_objective(name):
    rec = records(dict(SCENES)[name])
    out0, link0, m0, info0 = build_ex(rec, 0)
    assert info0[0] == m0 and info0[1] == 0                        # no passes: the top-down tree, no moves
    check_tree(rec, out0, link0, m0)
    for passes in sorted({1, 2, abi_passes(), 5}):
        out, link, m, info = build_ex(rec, passes)
        check_tree(rec, out, link, m)
        assert m <= m0 and info[0] == m0, (passes, m, m0)           # never more nodes than the top-down tree
        assert m <= max(1.6 * rec.shape[0], rec.shape[0] + 1)
        assert info[2] == info0[2] and info[3] <= info[2]           # the build's own figures ...
        assert abs(info[3] - tree_cost(rec, out, link, m)) <= 1e-9 * info[3] + 1e-300
        c0, c = tree_cost(rec, out0, link0, m0), tree_cost(rec, out, link, m)
        assert c <= c0 * (1.0 + 1e-9), (passes, c, c0)              # ... and the same recomputed from the emitted tree
        again = build_ex(rec, passes)
        assert np.array_equal(out, again[0]) and np.array_equal(link, again[1]) and info == again[3]
    d_out, d_link, d_m = build_hierarchy(rec)                       # the default entry point: the library's pass count
    ex = build_ex(rec, abi_passes())
    assert d_m == ex[2] and np.array_equal(d_out, ex[0]) and np.array_equal(d_link, ex[1])


def abi_passes():
    """RT355_HIERARCHY_PASSES of include/rt355.h"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt355.h")).read()
    return int(re.search(r"#define\s+RT355_HIERARCHY_PASSES\s+(\d+)u", text).group(1))


def test_the_pass_finds_something_on_the_baseline_scenes():
    """not a measurement, a guard against a pass that silently does nothing: on C3's and C5's spheres it moves subtrees and lowers
    the cost"""
    for n, seed in [(1024, 358), (4096, 360)]:
        info = build_ex(records(synthetic_spheres(n, seed)), abi_passes())[3]
        assert info[1] > 0 and info[3] < info[2]


def test_non_finite_records_keep_the_top_down_tree():
    rec = records(synthetic_spheres(50, 3))
    rec[7, 0] = np.inf
    rec[11, 7] = np.inf
    a, b = build_ex(rec, 0), build_ex(rec, 3)
    assert b[3][1] == 0 and a[2] == b[2] and np.array_equal(a[1], b[1])
