"""Device BLAS builds on the MI355X (include/rt355.h: rt_build_blas, rt_read_tri_lookup): the node buffer and the lookup table the
device leaves against the host model (rt_build_blas_host: the same inline arithmetic, run serially) byte for byte, against the
host builder (acceleration/bvh.py: build_tree) bit for bit in the nodes and up to the order inside a leaf in the lookup, and every
frame form and query family against the CPU oracle on exactly the buffers the scene object then holds.  No tolerance anywhere.

Frames are 64 x 48.  T = 65 and 257 are one past a wave and one past a 256-lane chunk of the partition, T = 1000 gives several
chunks at the top and some 13 levels of many short nodes."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.acceleration.bvh import build_tree
from compute_raytracer_amd.scene_raytracing import TriMesh
from build_common import (bits, build_host, canonical, check_well_formed, grid_records, mesh_and_tree, one_leaf_tree,
                          perturbed_grid_records, random_records, ranges_array, soup_of)
from helpers import deepen_top_level, diff_stats, random_sky, tri_buffers
from query_common import camera_rays, check_all_queries, check_triangle_hits, random_rays, scene_box
from refit_common import B, F, FP, H, U32, W, deform, mesh_ranges, numpy_refit, refit_plan, view_scene
from test_gbuffer_gpu import hits_of
from test_refit_tri_gpu import CASES, all_roots, frames_in_flight, make, oracle_frame
from test_render_samples_cpu import resolve_np
from test_render_samples_gpu import check as check_samples

pytestmark = pytest.mark.gpu

RANGE = ctypes.POINTER(abi.RtBlasRange)


def single_mesh_scene(records, node_capacity="full", tree=None):
    """one mesh, one instance in front of the camera; tree None: the dummy one-leaf tree"""
    soup = soup_of(records)
    mesh = TriMesh(soup, tree if tree is not None else one_leaf_tree(soup))
    models = [dict(meshIndex=0, position=[0.0, 0.5, -6.0], eulers=[20, 30, 0])]
    return rt.SceneRaytracing().createScene([]).createTriangleScene([mesh], models, node_capacity=node_capacity)


def full_view_scene(n_models=3):
    scene, mat = view_scene(n_models)
    return scene.createTriangleScene(scene.meshes, scene.instances, node_capacity="full"), mat


def mesh_rows(scene):
    """the ranges rebuild() passes: (root_node, node_cap, first_slot, n_slots) per mesh"""
    ends = [m.root_node for m in scene.meshes[1:]] + [scene.node_buffer_length()]
    return [(m.root_node, e - m.root_node, m.lookup_offset, m.soup.count) for m, e in zip(scene.meshes, ends)]


@pytest.mark.parametrize("name", ["T1", "T2", "T65", "T257", "T1000", "grid", "duplicates"])
def test_device_build_is_the_model_and_the_builder(name):
    records, tree = mesh_and_tree(name)
    scene = single_mesh_scene(records)
    mat = rt.Material.white()
    r = make(scene, mat, random_sky(41))
    try:
        r.recalculateScene()
        before = tri_buffers(scene, mat)
        rows = mesh_rows(scene)
        assert rows[0][1] == max(2 * records.shape[0] - 1, 1)
        used = r.rebuild()
        got_nodes, got_lookup = r.read_nodes(), r.read_tri_lookup()
        rc, want_nodes, want_lookup, want_used = build_host(before["triangles"], before["tri_lookup"], before["nodes"], rows)
        assert rc == abi.RT_OK and used == [int(want_used[0])] == [tree.used]
        bad = np.nonzero((bits(got_nodes) != bits(want_nodes)).any(axis=1))[0]
        assert bad.size == 0, "nodes %s differ from the model" % bad[:8]
        assert np.array_equal(bits(got_lookup), bits(want_lookup))
        root = rows[0][0]
        assert np.array_equal(bits(got_nodes[root:root + tree.used]), bits(tree.nodes(root, 0)))
        assert np.array_equal(bits(got_nodes[root + tree.used:]), bits(before["nodes"][root + tree.used:]))
        assert np.array_equal(canonical(got_lookup, got_nodes, root), canonical(tree.order.astype(F), got_nodes, root))
        assert np.array_equal(bits(scene.static["blas_nodes"]), bits(got_nodes[scene.tlasNodesMax:]))
        assert np.array_equal(bits(scene.static["tri_lookup"]), bits(got_lookup))
        assert r.rebuild() == used                       # a second build changes no byte
        assert np.array_equal(bits(r.read_nodes()), bits(got_nodes)) and np.array_equal(bits(r.read_tri_lookup()), bits(got_lookup))
    finally:
        r.close()


@pytest.mark.parametrize("case", ["tiny", "node_buffer", "deep"])
def test_rebuilt_deformed_mesh_nodes_and_frames(oracle, case):
    """update_triangles + rebuild(): the node bytes against build_tree of the deformed soup, an awaited frame, three frames in
    flight and an awaited one behind them -- through the pair records (variant 0: rebuilt exactly once), through the node buffer
    alone (variant 6), and in the twenty-slot form, where BLAS nodes live in the head copy that frames carry."""
    n_models, deepen, variant, form = CASES[case]
    scene, mat = full_view_scene(n_models)
    sky = random_sky(42)
    if deepen:
        deepen_top_level(scene, min(deepen, (scene.tlasNodesMax - len(scene.frame["tlas_nodes"])) // 2))
    r = make(scene, mat, sky, variant)
    try:
        r.render()
        assert np.array_equal(r.read_pixels(), oracle_frame(oracle, scene, mat, sky))
        assert r.stats()["tri_form"] == form
        rebuilds = r.stats()["pair_rebuilds"]
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        tris = deform(old["triangles"], first, count, "grow")
        tree = build_tree(soup_of(tris[first:first + count]))
        # the input condition, on the oracle alone: a refit of the old topology is NOT what the builder makes of the new pose
        rc, _, plan = refit_plan(old["nodes"], len(old["tri_lookup"]), all_roots(scene))
        assert rc == abi.RT_OK
        refitted = numpy_refit(old["nodes"], tris, old["tri_lookup"], plan)
        want = old["nodes"].copy()
        want[root:root + tree.used] = tree.nodes(root, first)
        assert tree.used <= mesh_rows(scene)[1][1] and not np.array_equal(bits(refitted), bits(want))
        r.update_triangles(first, tris[first:first + count])
        used = r.rebuild()
        assert used[1] == tree.used
        got, lookup = r.read_nodes(), r.read_tri_lookup()
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, "nodes %s differ from build_tree (the other meshes' must not change a bit)" % bad[:8]
        want_lookup = old["tri_lookup"].copy()
        want_lookup[first:first + count] = (tree.order + first).astype(F)
        for m_root, _, _, _ in mesh_rows(scene):
            assert np.array_equal(canonical(lookup, got, m_root), canonical(want_lookup, got, m_root))
        packed = scene.to_packed()
        assert np.array_equal(bits(packed["triangles"]), bits(tris))
        assert np.array_equal(bits(packed["blas_nodes"]), bits(got[scene.tlasNodesMax:]))
        assert np.array_equal(bits(packed["tri_lookup"]), bits(lookup))
        fresh = oracle_frame(oracle, scene, mat, sky)
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, fresh), diff_stats(img, fresh)
        assert r.stats()["tri_form"] == form
        for f, img in enumerate(frames_in_flight(r)):
            assert np.array_equal(img, fresh), (f, diff_stats(img, fresh))
        r.render()
        assert np.array_equal(r.read_pixels(), fresh)
        assert r.stats()["pair_rebuilds"] == (0 if variant == 6 else rebuilds + 1)
        r.refit()                                        # the builder's boxes are the refit's: no byte moves
        assert np.array_equal(bits(r.read_nodes()), bits(got))
        r.render()
        assert np.array_equal(r.read_pixels(), fresh)
    finally:
        r.close()


def test_rebuilt_deformed_mesh_queries(oracle):
    """every query family, a 2 x 2 supersampled frame and a geometry frame on the rebuilt scene"""
    scene, mat = full_view_scene()
    sky = random_sky(43)
    r = make(scene, mat, sky)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        tris = deform(old["triangles"], first, count, "grow")
        r.update_triangles(first, tris[first:first + count])
        r.rebuild()
        buf = tri_buffers(scene, mat)
        assert np.array_equal(bits(buf["nodes"]), bits(r.read_nodes()))
        params = np.asarray(scene.pack_params(B), F)
        state = dict(tri=buf, params=params, faces=sky.faces)
        lo, hi = scene_box(buf, scene)
        sets = [camera_rays(scene, W, H, 2), random_rays(lo, hi, 400, 9)]
        rays = (np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
        assert check_all_queries(oracle, r, state, rays) > 100
        big = oracle.render_tri(params, buf, sky.faces, 2 * W, 2 * H, want_float=True)[1]
        img, flt = r.render_samples(2, float_out=True)
        check_samples(img, flt, resolve_np(big, 2), "2 x 2 after a rebuild")
        o, d = camera_rays(scene, W, H)
        assert check_triangle_hits(oracle, buf, o, d, hits_of(r.render_gbuffer())) > 100
    finally:
        r.close()


def test_a_tree_beyond_its_capacity_changes_nothing(oracle):
    """The flat grid's tree has two-triangle leaves (287 nodes); its vertices perturbed, the builder wants more.  Laid out tight:
    RT_ERR_CAPACITY with the needed count, and nodes, lookup and the next frame are what they were.  Laid out "full": it fits."""
    flat, moved = grid_records(), perturbed_grid_records()
    need = build_tree(soup_of(moved)).used
    assert need > 287
    mat, sky = rt.Material.white(), random_sky(44)
    for capacity in ("tight", "full"):
        scene = single_mesh_scene(flat, capacity, tree=build_tree(soup_of(flat)))
        r = make(scene, mat, sky)
        try:
            r.render()
            r.update_triangles(0, moved)
            r.render()
            before_img, before_nodes, before_lookup = r.read_pixels(), r.read_nodes(), r.read_tri_lookup()
            assert np.array_equal(before_img, oracle_frame(oracle, scene, mat, sky))
            rebuilds = r.stats()["pair_rebuilds"]
            if capacity == "tight":
                with pytest.raises(abi.RtError) as e:
                    r.rebuild()
                assert e.value.code == abi.RT_ERR_CAPACITY and ("needs %d nodes" % need) in str(e.value) and "has 287" in str(e.value)
                assert np.array_equal(bits(r.read_nodes()), bits(before_nodes)) and np.array_equal(bits(r.read_tri_lookup()), bits(before_lookup))
                r.render()
                assert np.array_equal(r.read_pixels(), before_img) and r.stats()["pair_rebuilds"] == rebuilds
            else:
                assert r.rebuild() == [need]
                r.render()
                img, ref = r.read_pixels(), oracle_frame(oracle, scene, mat, sky)
                assert np.array_equal(img, ref), diff_stats(img, ref)
        finally:
            r.close()


def test_the_error_list_through_the_context(oracle):
    scene, mat = full_view_scene()
    sky = random_sky(45)
    r = make(scene, mat, sky)
    L = r._lib
    try:
        r.render()
        ref = oracle_frame(oracle, scene, mat, sky)
        n_nodes, n_slots = scene.node_buffer_length(), scene.triangleCount
        good = mesh_rows(scene)
        before_nodes, before_lookup = r.read_nodes(), r.read_tri_lookup()
        used = np.zeros(4, np.uint32)

        def call(rows, ctx=r._ctx, null=False):
            a = ranges_array(rows)
            return L.rt_build_blas(ctx, None if null else a.ctypes.data_as(RANGE), len(rows), used.ctypes.data_as(U32))
        assert call(good[:1], ctx=None) == abi.RT_ERR_INVALID_ARG
        assert L.rt_build_blas(r._ctx, None, 1, None) == abi.RT_ERR_INVALID_ARG
        assert L.rt_build_blas(r._ctx, None, 0, None) == abi.RT_OK
        root, cap, first, n = good[0]
        bad = {"no slots": [(root, cap, first, 0)], "no nodes": [(root, 0, first, n)],
               "beyond the nodes": [(root, n_nodes - root + 1, first, n)], "node sum wraps": [(0xFFFFFFFF, 2, first, n)],
               "beyond the slots": [(root, cap, n_slots - 1, 2)], "slot sum wraps": [(root, cap, 0xFFFFFFFF, 2)],
               "overlap in nodes": [good[0], (root + cap - 1, 2, good[1][2], good[1][3])],
               "overlap in slots": [good[0], (good[1][0], good[1][1], first + n - 1, 2)],
               "the same range twice": [good[0], good[0]], "node 0": [(0, root + cap, first, n)]}
        for name, rows in bad.items():
            assert call(rows) == abi.RT_ERR_INVALID_ARG, name
        assert call([(root, cap - 2, first, n)]) == abi.RT_ERR_CAPACITY and used[0] == cap
        assert L.rt_read_tri_lookup(None, 0, 1, before_lookup.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_tri_lookup(r._ctx, 0, 1, None) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_tri_lookup(r._ctx, n_slots, 1, before_lookup.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_tri_lookup(r._ctx, 0xFFFFFFFF, 2, before_lookup.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_tri_lookup(r._ctx, n_slots, 0, None) == abi.RT_OK
        assert np.array_equal(bits(r.read_nodes()), bits(before_nodes)) and np.array_equal(bits(r.read_tri_lookup()), bits(before_lookup))
        r.render()
        assert np.array_equal(r.read_pixels(), ref) and r.stats()["pair_rebuilds"] == 1
    finally:
        r.close()


def test_a_sphere_scene_is_a_state_error():
    scene = rt.synthetic_scene(5, 3)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(None)
    try:
        r.recalculateScene()
        a = ranges_array([(1, 3, 0, 2)])
        assert r._lib.rt_build_blas(r._ctx, a.ctypes.data_as(RANGE), 1, None) == abi.RT_ERR_STATE
        assert r._lib.rt_build_blas(r._ctx, a.ctypes.data_as(RANGE), 0, None) == abi.RT_ERR_STATE
    finally:
        r.close()


def test_non_finite_corners_leave_a_well_formed_tree():
    """NaN and infinite corners: the call returns, every slot is in exactly one leaf of a well-formed tree, a frame renders"""
    records = random_records(257, 77).copy()
    rng = np.random.default_rng(78)
    odd = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F)
    for t in rng.choice(257, 60, replace=False):
        records[t, 12 * int(rng.integers(3)) + int(rng.integers(3))] = odd[int(rng.integers(len(odd)))]
    scene = single_mesh_scene(records)
    mat = rt.Material.white()
    r = make(scene, mat, random_sky(46))
    try:
        r.recalculateScene()
        before = r.read_tri_lookup()
        used = r.rebuild()
        check_well_formed(r.read_nodes(), r.read_tri_lookup(), mesh_rows(scene)[0], used[0], before)
        r.render()
        assert r.read_pixels().shape == (H, W, 4)
    finally:
        r.close()
