"""The host model of the device BLAS build (include/rt355.h: rt_build_blas_host; csrc/rt_blas_build.h -- the inline arithmetic the
kernels of rt_build.hip call, run serially) against the host builder (acceleration/bvh.py: build_tree): nodes bit for bit, `used`
equal, the lookup equal once every leaf's run is sorted -- build_tree's two-pointer sweep and the model's stable partition differ
only in the order inside a leaf.  Then the calling contract: ranges, errors, capacity, non-finite corners; and the "full" node
layout of createTriangleScene.  No GPU."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.acceleration.bvh import build_tree
from build_common import (MESHES, MIXED_COUNTS, bits, build_host, canonical, check_rows_are_build_tree, check_well_formed, grid_records,
                          level_widths, mesh_and_tree, mesh_rows, mixed_scene, mixed_trees, perturbed_grid_records, random_records,
                          ranges_array, soup_of)
from helpers import random_sky, tri_buffers
from refit_common import B, F, FP, H, U32, W, deform, view_scene


@pytest.mark.parametrize("name", list(MESHES))
def test_the_model_is_build_tree(name):
    records, tree = mesh_and_tree(name)
    T, root, first = records.shape[0], 5, 3                        # the tree sits behind five nodes and three foreign slots
    nodes = np.full((root + 2 * T + 1, 8), 7.5, F)
    lookup = np.concatenate([np.full(first, 9.0, F), np.arange(T, dtype=F), np.full(2, 9.0, F)])
    rows = [(root, 2 * T - 1 if T > 1 else 1, first, T)]
    rc, nd, lk, used = build_host(records, lookup, nodes, rows)
    assert rc == abi.RT_OK and int(used[0]) == tree.used
    assert np.array_equal(bits(nd[root:root + tree.used]), bits(tree.nodes(root, first)))
    untouched = np.r_[0:root, root + tree.used:nodes.shape[0]]
    assert np.array_equal(bits(nd[untouched]), bits(nodes[untouched]))
    want = lookup.copy()
    want[first:first + T] = tree.order.astype(F)
    assert np.array_equal(canonical(lk, nd, root), canonical(want, nd, root))
    check_well_formed(nd, lk, rows[0], int(used[0]), lookup)
    if name in ("grid", "duplicates"):                             # the input condition that makes the canonical form necessary
        assert not np.array_equal(lk, want)
    if name == "grid":
        assert tree.used == 287 and 2 * T - 1 == 575
    if name == "duplicates":
        assert tree.used == 1 and np.array_equal(lk, lookup)     # one leaf of 40, in the order the slots had
    rc, nd2, lk2, used2 = build_host(records, lk, nd, rows)        # a second call changes no byte
    assert rc == abi.RT_OK and np.array_equal(bits(nd2), bits(nd)) and np.array_equal(bits(lk2), bits(lk)) and used2[0] == used[0]


def test_the_skew_mesh_is_deep_and_t1000_is_wide():
    """Input conditions of the device tests (tests/test_build_blas_gpu.py).  `skew`: a long chain of narrow levels -- one host
    read-back, one count_up, rank_down and emit launch per level.  `T1000`: a level wider than 256 nodes with more than 256 splits
    -- the scan's carry across its 256-node chunks already runs there and needs no further case."""
    records, tree = mesh_and_tree("skew")
    widths = level_widths(tree.nodes(0, 0), 0)
    assert sum(widths) == tree.used and len(widths) >= 30
    assert sum(1 for w in widths if w <= 4) >= len(widths) - 4
    records, tree = mesh_and_tree("T1000")
    widths = level_widths(tree.nodes(0, 0), 0)
    assert sum(widths) == tree.used
    assert any(a > 256 and b > 512 for a, b in zip(widths, widths[1:]))


def test_run_lengths_at_the_edges_of_the_partitions():
    """the input condition of T64 .. T513: their roots split (the partition of a run of exactly that length runs), and the two
    sides of the comparison with kBuildShort = 256 are both there"""
    for name, T in (("T64", 64), ("T128", 128), ("T256", 256), ("T257", 257), ("T512", 512), ("T513", 513)):
        records, tree = mesh_and_tree(name)
        assert records.shape[0] == T and tree.count[0] == 0 and tree.used > 1, name


def test_the_mixed_scene_is_build_tree_per_mesh():
    """The scene of the device's call-shape test, through the model alone: all seven ranges in one call, in mesh order and reversed,
    equal build_tree per mesh; the unused capacity of every range and the top-level nodes stay untouched.  Then the model after a
    deformation of mesh 0, and the input condition that its tree is another one."""
    scene, mat = mixed_scene(), rt.Material.white()
    buf = tri_buffers(scene, mat)
    rows, trees = mesh_rows(scene), mixed_trees()
    assert [r[3] for r in rows] == list(MIXED_COUNTS) and [r[1] for r in rows] == [max(2 * T - 1, 1) for T in MIXED_COUNTS]
    assert np.array_equal(buf["tri_lookup"], np.arange(sum(MIXED_COUNTS), dtype=F))
    assert sum(T > 256 for T in MIXED_COUNTS[:4]) == 2 and MIXED_COUNTS[2] == 1 and trees[6].used == 1      # long, short, single, long | ..., a leaf
    assert all(t.used > 1 for t, T in zip(trees[:6], MIXED_COUNTS) if T > 1)
    rc, nd, lk, used = build_host(buf["triangles"], buf["tri_lookup"], buf["nodes"], rows)
    assert rc == abi.RT_OK and used.tolist() == [t.used for t in trees]
    check_rows_are_build_tree(nd, lk, buf["nodes"], buf["tri_lookup"], rows, trees)
    assert any(t.used < r[1] for t, r in zip(trees, rows))                                                  # there is unused capacity
    rc, nd2, lk2, used2 = build_host(buf["triangles"], buf["tri_lookup"], buf["nodes"], rows[::-1])
    assert rc == abi.RT_OK and used2.tolist() == used.tolist()[::-1]
    assert np.array_equal(bits(nd2), bits(nd)) and np.array_equal(bits(lk2), bits(lk))
    rc, nd3, lk3, used3 = build_host(buf["triangles"], buf["tri_lookup"], buf["nodes"], [rows[3], rows[0]])
    assert rc == abi.RT_OK and used3.tolist() == [trees[3].used, trees[0].used]
    check_rows_are_build_tree(nd3, lk3, buf["nodes"], buf["tri_lookup"], rows, trees, built=[3, 0])
    root, cap, first, n = rows[0]
    tris = deform(buf["triangles"], first, n, "grow")
    moved = build_tree(soup_of(tris[first:first + n]))
    assert moved.used != trees[0].used or not np.array_equal(bits(moved.nodes(root, first)[:, [3, 7]]), bits(trees[0].nodes(root, first)[:, [3, 7]]))
    rc, nd4, lk4, used4 = build_host(tris, lk, nd, [rows[0]])
    assert rc == abi.RT_OK and used4.tolist() == [moved.used]
    check_rows_are_build_tree(nd4, lk4, nd, lk, rows, [moved] + trees[1:], built=[0])


def two_meshes():
    a, b = mesh_and_tree("T65"), mesh_and_tree("grid")
    tris = np.concatenate([a[0], b[0]])
    lookup = np.arange(tris.shape[0], dtype=F)
    rows = [(2, 129, 0, 65), (2 + 129 + 10, 575, 65, 288)]         # a gap of ten nodes between the ranges
    nodes = np.full((rows[1][0] + 575, 8), -3.25, F)
    return tris, lookup, nodes, rows, (a[1], b[1])


def test_two_ranges_and_the_gap_between_them():
    tris, lookup, nodes, rows, trees = two_meshes()
    rc, nd, lk, used = build_host(tris, lookup, nodes, rows[::-1])         # any order
    assert rc == abi.RT_OK and used.tolist() == [trees[1].used, trees[0].used]
    touched = np.zeros(nodes.shape[0], bool)
    for (root, cap, first, n), tree, tri_base in zip(rows, trees, (0, 65)):
        assert np.array_equal(bits(nd[root:root + tree.used]), bits(tree.nodes(root, first)))
        touched[root:root + tree.used] = True
        want = lookup.copy()
        want[first:first + n] = (tree.order + tri_base).astype(F)
        assert np.array_equal(canonical(lk, nd, root)[first:first + n], canonical(want, nd, root)[first:first + n])
    assert np.array_equal(bits(nd[~touched]), bits(nodes[~touched]))       # the gap, and the grid's unused 288 nodes


def test_every_refusal_leaves_the_arrays_alone():
    tris, lookup, nodes, rows, trees = two_meshes()
    n_nodes, n_slots = nodes.shape[0], lookup.shape[0]
    root, cap, first, n = rows[0]
    inv = abi.RT_ERR_INVALID_ARG
    bad = {"no slots": [(root, cap, first, 0)], "no nodes": [(root, 0, first, n)],
           "beyond the nodes": [(n_nodes - 3, 4, first, n)], "node sum wraps": [(0xFFFFFFFF, 2, first, n)],
           "beyond the slots": [(root, cap, n_slots - 1, 2)], "slot sum wraps": [(root, cap, 0xFFFFFFFF, 2)],
           "overlap in nodes": [rows[0], (root + cap - 1, 20, rows[1][2], rows[1][3])],
           "overlap in slots": [rows[0], (rows[1][0], rows[1][1], first + n - 1, 5)],
           "the same range twice": [rows[0], rows[0]], "node 0": [(0, root + cap, first, n)]}
    for name, r in bad.items():
        rc, nd, lk, used = build_host(tris, lookup, nodes, r)
        assert rc == inv, name
        assert np.array_equal(bits(nd), bits(nodes)) and np.array_equal(bits(lk), bits(lookup)), name
    # capacity: reported with used[] set for every range, nothing stored; one node more and it fits
    short = [(root, trees[0].used - 1, first, n), rows[1]]
    rc, nd, lk, used = build_host(tris, lookup, nodes, short)
    assert rc == abi.RT_ERR_CAPACITY and used.tolist() == [trees[0].used, trees[1].used]
    assert np.array_equal(bits(nd), bits(nodes)) and np.array_equal(bits(lk), bits(lookup))
    rc, nd, lk, used = build_host(tris, lookup, nodes, [(root, trees[0].used, first, n), rows[1]])
    assert rc == abi.RT_OK and used.tolist() == [trees[0].used, trees[1].used]
    # the argument checks, in their order
    L = abi.load()
    t, lk, nd = np.ascontiguousarray(tris, F), lookup.copy(), nodes.copy()
    r = ranges_array(rows)
    args = (t.ctypes.data_as(FP), t.shape[0], lk.ctypes.data_as(FP), n_slots, nd.ctypes.data_as(FP), n_nodes)
    assert L.rt_build_blas_host(*args, None, 1, None) == inv
    assert L.rt_build_blas_host(None, 0, lk.ctypes.data_as(FP), n_slots, nd.ctypes.data_as(FP), n_nodes, None, 1, None) == inv
    assert L.rt_build_blas_host(None, 0, lk.ctypes.data_as(FP), n_slots, nd.ctypes.data_as(FP), n_nodes,
                                r.ctypes.data_as(ctypes.POINTER(abi.RtBlasRange)), 2, None) == abi.RT_ERR_STATE
    assert L.rt_build_blas_host(*args, None, 0, None) == abi.RT_OK
    assert L.rt_build_blas_host(*args, r.ctypes.data_as(ctypes.POINTER(abi.RtBlasRange)), 2, None) == abi.RT_OK      # used may be NULL


def test_the_perturbed_grid_needs_more_nodes_than_the_flat_one():
    """the input condition of the capacity test on the device (tests/test_build_blas_gpu.py)"""
    assert build_tree(soup_of(perturbed_grid_records())).used > build_tree(soup_of(grid_records())).used == 287


def test_triangle_indices_are_clamped_as_tri_corners_clamps_them():
    records = random_records(20, 5)
    lookup = np.arange(20, dtype=F)
    lookup[[3, 7, 11]] = [500.0, np.nan, -4.0]                     # -> the last triangle, triangle 0, triangle 0
    rc, nd, lk, used = build_host(records, lookup, np.zeros((40, 8), F), [(1, 39, 0, 20)])
    assert rc == abi.RT_OK
    seen = records[[19 if i == 3 else 0 if i in (7, 11) else i for i in range(20)]]
    tree = build_tree(soup_of(seen))
    assert int(used[0]) == tree.used and np.array_equal(bits(nd[1:1 + tree.used]), bits(tree.nodes(1, 0)))
    check_well_formed(nd, lk, (1, 39, 0, 20), int(used[0]), lookup)        # the words themselves are carried, not rewritten


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_non_finite_corners_leave_a_well_formed_tree(seed):
    records = random_records(257, 70 + seed).copy()
    rng = np.random.default_rng(seed)
    odd = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F)
    for t in rng.choice(257, 40 * seed, replace=False):
        records[t, 12 * int(rng.integers(3)) + int(rng.integers(3))] = odd[int(rng.integers(len(odd)))]
    lookup = np.arange(257, dtype=F)
    row = (1, 513, 0, 257)
    rc, nd, lk, used = build_host(records, lookup, np.zeros((514, 8), F), [row])
    assert rc == abi.RT_OK
    check_well_formed(nd, lk, row, int(used[0]), lookup)


def packed_as_the_parent_commit_packed(scene):
    """createTriangleScene's arrays as it made them before node_capacity existed: trees back to back"""
    at, nodes, parts, look = 0, 0, [], []
    for m in scene.meshes:
        parts.append(m.tree.nodes(scene.tlasNodesMax + nodes, at))
        look.append((m.tree.order + at).astype(np.float64))
        at += m.soup.count
        nodes += m.tree.used
    return np.concatenate(parts), np.concatenate(look).astype(F)


def test_the_full_layout_renders_the_tight_layouts_frame(oracle):
    tight, mat = view_scene()
    nodes, lookup = packed_as_the_parent_commit_packed(tight)
    assert np.array_equal(bits(tight.static["blas_nodes"]), bits(nodes)) and np.array_equal(bits(tight.static["tri_lookup"]), bits(lookup))
    assert tight.blasNodesUsed == nodes.shape[0]
    full, _ = view_scene()
    full.createTriangleScene(full.meshes, full.instances, node_capacity="full")
    assert [m.root_node for m in full.meshes] == [tight.tlasNodesMax + k for k in np.cumsum([0] + [max(2 * m.soup.count - 1, m.tree.used) for m in full.meshes[:-1]])]
    assert full.blasNodesUsed == sum(2 * m.soup.count - 1 for m in full.meshes) > tight.blasNodesUsed
    gaps = np.ones(full.blasNodesUsed, bool)
    for m in full.meshes:
        at = m.root_node - full.tlasNodesMax
        gaps[at:at + m.tree.used] = False
        assert np.array_equal(bits(full.static["blas_nodes"][at:at + m.tree.used]), bits(m.tree.nodes(m.root_node, m.lookup_offset)))
    assert gaps.any() and not full.static["blas_nodes"][gaps].view(np.uint32).any()
    assert np.array_equal(bits(full.static["tri_lookup"]), bits(tight.static["tri_lookup"]))
    sky = random_sky(40)
    a = oracle.render_tri(tight.pack_params(B), tri_buffers(tight, mat), sky.faces, W, H)[0]
    b = oracle.render_tri(full.pack_params(B), tri_buffers(full, mat), sky.faces, W, H)[0]
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        rt.SceneRaytracing().createTriangleScene(tight.meshes, tight.instances, node_capacity="loose")
