"""Device BLAS builds on the MI355X (include/rt355.h: rt_build_blas, rt_read_tri_lookup): the node buffer and the lookup table the
device leaves against the host model (rt_build_blas_host: the same inline arithmetic, run serially) byte for byte, against the
host builder (acceleration/bvh.py: build_tree) bit for bit in the nodes and up to the order inside a leaf in the lookup, and every
frame form and query family against the CPU oracle on exactly the buffers the scene object then holds.  No tolerance anywhere.

Frames are 64 x 48.  T = 64, 128, 256 and 512 are whole-chunk runs of the wave's and the block's partition, 65, 257 and 513 one
past them; 256 against 257 is the comparison with kBuildShort that build_price and build_split each make on their own.  T = 1000
gives several chunks at the top and some 13 levels of many short nodes (the scan's carry), `skew` more than 30 levels of two or
four nodes.  The mixed scene (tests/build_common.py: mixed_scene) puts long, short and one-triangle runs into one block of four
nodes; its tests keep the expected bytes as host arrays that only the model advances through a sequence of calls in one context.
The input conditions are asserted without a GPU in tests/test_build_blas_cpu.py or at the head of the test that needs them."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.acceleration.bvh import build_tree
from compute_raytracer_amd.scene_raytracing import TriMesh
from build_common import (MIXED_COUNTS, bits, build_host, canonical, check_well_formed, grid_records, mesh_and_tree, mesh_rows, mixed_scene,
                          one_leaf_tree, perturbed_grid_records, random_records, ranges_array, soup_of)
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


def two_mesh_scene(pairs, node_capacity):
    """two meshes given as (records, tree) with their trees, side by side in front of the camera"""
    meshes = [TriMesh(soup_of(rec), tree) for rec, tree in pairs]
    models = [dict(meshIndex=k, position=[-3.0 + 6.0 * k, 0.5, -8.0], eulers=[20, 30, 0]) for k in range(2)]
    return rt.SceneRaytracing().createScene([]).createTriangleScene(meshes, models, node_capacity=node_capacity)


# ---- the expected state as cumulative host arrays: started from the scene's packed buffers, advanced by the model alone, never
# ---- read back from the device -- one wrong byte stays wrong in every later comparison
def host_state(scene, mat):
    buf = tri_buffers(scene, mat)
    return dict(triangles=np.array(buf["triangles"], F).copy(), nodes=np.array(buf["nodes"], F).copy(), lookup=np.array(buf["tri_lookup"], F).copy())


def advance(state, rows):
    """rt_build_blas_host of `rows` on the state -> the model's used[], in the order of the call"""
    rc, state["nodes"], state["lookup"], used = build_host(state["triangles"], state["lookup"], state["nodes"], rows)
    assert rc == abi.RT_OK
    return [int(u) for u in used]


def same_as_model(r, state, what):
    """the WHOLE node buffer and the WHOLE lookup table of the device against the state, bit for bit -> (nodes, lookup) read"""
    got_nodes, got_lookup = r.read_nodes(), r.read_tri_lookup()
    assert got_nodes.shape == state["nodes"].shape and got_lookup.shape == state["lookup"].shape
    bad = np.nonzero((bits(got_nodes) != bits(state["nodes"])).any(axis=1))[0]
    assert bad.size == 0, "%s: nodes %s (%d in all) differ from the model" % (what, bad[:8], bad.size)
    bad = np.nonzero(bits(got_lookup) != bits(state["lookup"]))[0]
    assert bad.size == 0, "%s: lookup slots %s (%d in all) differ from the model" % (what, bad[:8], bad.size)
    return got_nodes, got_lookup


def scene_holds(scene, state, what):
    """scene.to_packed() describes the device: the state's bytes"""
    packed = scene.to_packed()
    assert np.array_equal(bits(packed["triangles"]), bits(state["triangles"])), what
    assert np.array_equal(bits(packed["blas_nodes"]), bits(state["nodes"][scene.tlasNodesMax:])), what
    assert np.array_equal(bits(packed["tri_lookup"]), bits(state["lookup"])), what


@pytest.mark.parametrize("name", ["T1", "T2", "T3", "T64", "T65", "T128", "T256", "T257", "T512", "T513", "T1000", "grid", "duplicates", "skew"])
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
        host = tri_buffers(scene, mat)
        assert np.array_equal(bits(before), bits(host["tri_lookup"]))
        used = r.rebuild()
        check_well_formed(r.read_nodes(), r.read_tri_lookup(), mesh_rows(scene)[0], used[0], before)
        # the device and the model call the same inline functions: the same bytes here too
        rc, want_nodes, want_lookup, want_used = build_host(host["triangles"], host["tri_lookup"], host["nodes"], mesh_rows(scene))
        assert rc == abi.RT_OK and used == want_used.tolist()
        same_as_model(r, dict(nodes=want_nodes, lookup=want_lookup), "non-finite corners")
        r.render()
        assert r.read_pixels().shape == (H, W, 4)
    finally:
        r.close()


def test_triangle_indices_are_clamped_as_tri_corners_clamps_them():
    """The device twin of the model's test (tests/test_build_blas_cpu.py): lookup words beyond the triangles, NaN and negative are
    read as tri_corners reads them -- the last triangle, triangle 0, triangle 0 -- and carried into the new table as the bit
    patterns they were, not re-derived from the index they stood for."""
    records = random_records(20, 5)
    scene = single_mesh_scene(records)
    words = np.array(scene.static["tri_lookup"], F).copy()
    words[[3, 7, 11]] = [500.0, np.nan, -4.0]
    scene.static["tri_lookup"] = words                   # before the upload: recalculateScene writes the packed table
    mat = rt.Material.white()
    r = make(scene, mat, random_sky(47))
    try:
        r.recalculateScene()
        host = tri_buffers(scene, mat)
        assert np.array_equal(bits(r.read_tri_lookup()), bits(words))
        rows = mesh_rows(scene)
        used = r.rebuild()
        rc, want_nodes, want_lookup, want_used = build_host(host["triangles"], words, host["nodes"], rows)
        assert rc == abi.RT_OK and used == want_used.tolist()
        got_nodes, got_lookup = same_as_model(r, dict(nodes=want_nodes, lookup=want_lookup), "odd lookup words")
        seen = records[[19 if i == 3 else 0 if i in (7, 11) else i for i in range(20)]]
        tree = build_tree(soup_of(seen))
        root = rows[0][0]
        assert used == [tree.used] and np.array_equal(bits(got_nodes[root:root + tree.used]), bits(tree.nodes(root, 0)))
        assert np.array_equal(np.sort(bits(got_lookup)), np.sort(bits(words)))
        for w in words[[3, 7, 11]]:
            assert (bits(got_lookup) == bits(w)).sum() == 1
    finally:
        r.close()


def moved_only(before, state, rows, built):
    """between two states of the model, only the node ranges and the slots of the meshes `built` may differ"""
    node_free, slot_free = np.zeros(len(state["nodes"]), bool), np.zeros(len(state["lookup"]), bool)
    for k in built:
        root, cap, first, n = rows[k]
        node_free[root:root + cap] = True
        slot_free[first:first + n] = True
    assert np.array_equal(bits(before["nodes"][~node_free]), bits(state["nodes"][~node_free]))
    assert np.array_equal(bits(before["lookup"][~slot_free]), bits(state["lookup"][~slot_free]))


def copy_of(state):
    return {k: v.copy() for k, v in state.items()}


def test_call_shapes_on_the_mixed_scene(oracle):
    """Seven meshes of 300, 65, 1, 600, 2, 257 and 40 triangles: long, short and one-triangle runs share the blocks of four nodes
    of a level.  One context goes through a one-triangle call, two long roots in descending order, all seven (the scratch
    grows), the seven reversed through the C ABI with used = NULL, and a smaller call after the larger one on a deformed mesh.
    After every step the whole node buffer and the whole lookup table are the model's (tests/test_build_blas_cpu.py pins the
    model to build_tree on this scene), kept as host arrays that only the model advances; then a frame and every query family."""
    scene, mat = mixed_scene(), rt.Material.white()
    sky = random_sky(48)
    r = make(scene, mat, sky)
    try:
        r.recalculateScene()
        state, rows = host_state(scene, mat), mesh_rows(scene)
        assert [row[3] for row in rows] == list(MIXED_COUNTS)
        same_as_model(r, state, "the upload")
        # a. one triangle, the smallest scratch
        before = copy_of(state)
        assert r.rebuild([2]) == advance(state, [rows[2]]) == [1]
        moved_only(before, state, rows, [2])
        same_as_model(r, state, "a: rebuild([2])")
        # b. two long roots, descending: used[] follows the call
        before = copy_of(state)
        used = r.rebuild([3, 0])
        assert used == advance(state, [rows[3], rows[0]]) and used[0] != used[1]
        moved_only(before, state, rows, [3, 0])
        same_as_model(r, state, "b: rebuild([3, 0])")
        # c. all seven: the scratch grows
        assert r.rebuild() == advance(state, rows)
        same_as_model(r, state, "c: rebuild()")
        scene_holds(scene, state, "c")
        # d. the same ranges reversed, through the C ABI, used = NULL: no byte changes
        before = copy_of(state)
        a = ranges_array(rows[::-1])
        assert r._lib.rt_build_blas(r._ctx, a.ctypes.data_as(RANGE), len(rows), None) == abi.RT_OK
        advance(state, rows[::-1])
        assert np.array_equal(bits(before["nodes"]), bits(state["nodes"])) and np.array_equal(bits(before["lookup"]), bits(state["lookup"]))
        same_as_model(r, state, "d: reversed, used = NULL")
        # e. a smaller call after the larger one: mesh 0 deformed and rebuilt alone
        root, cap, first, n = rows[0]
        state["triangles"] = deform(state["triangles"], first, n, "grow")
        r.update_triangles(first, state["triangles"][first:first + n])
        before = copy_of(state)
        assert r.rebuild([0]) == advance(state, [rows[0]])
        # the input condition, on the model alone: another tree, not the old one with new boxes
        assert not np.array_equal(bits(before["nodes"][root:root + cap, [3, 7]]), bits(state["nodes"][root:root + cap, [3, 7]]))
        moved_only(before, state, rows, [0])
        same_as_model(r, state, "e: rebuild([0]) of the deformed mesh")
        scene_holds(scene, state, "e")
        # f. a frame and every query family on exactly these buffers
        buf = tri_buffers(scene, mat)
        assert np.array_equal(bits(buf["nodes"]), bits(state["nodes"])) and np.array_equal(bits(buf["tri_lookup"]), bits(state["lookup"]))
        o, d = camera_rays(scene, W, H)
        assert int((oracle.trace_tri_rays(buf, o, d) > 0).sum()) >= 100
        ref = oracle_frame(oracle, scene, mat, sky, buf)
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, ref), diff_stats(img, ref)
        params = np.asarray(scene.pack_params(B), F)
        lo, hi = scene_box(buf, scene)
        sets = [camera_rays(scene, W, H, 2), random_rays(lo, hi, 400, 9)]
        rays = (np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
        assert check_all_queries(oracle, r, dict(tri=buf, params=params, faces=sky.faces), rays) > 100
    finally:
        r.close()


def plan_of(nodes, n_lookup, roots):
    rc, _, plan = refit_plan(nodes, n_lookup, roots)
    assert rc == abi.RT_OK
    return plan


@pytest.mark.parametrize("cached", ["every root", "one root"])
def test_a_refit_plan_cached_before_a_rebuild_is_dropped(oracle, cached):
    """refit() caches its plan -- the runs of the tree it walked.  A rebuild makes another tree: the next refit must walk again
    (rt_build_blas bumps the context's topology generation), or the old tree's runs are applied to the new tree's nodes.
    "every root": the plan of the builder's trees, mesh 1 rebuilt in a grown pose, then refitted in a second pose.  "one root":
    the plan of mesh 1 alone, then a rebuild of the deformed mesh 0 -- a call that does not touch that plan's tree."""
    scene, mat = full_view_scene()
    sky = random_sky(49)
    r = make(scene, mat, sky)
    try:
        r.render()
        state, rows = host_state(scene, mat), mesh_rows(scene)
        original = copy_of(state)
        (root0, first0, n0), (root1, first1, n1) = mesh_ranges(scene)[0:2]
        roots = all_roots(scene) if cached == "every root" else [root1]
        r.refit(None if cached == "every root" else roots)             # caches a plan of the builder's trees; no byte moves
        same_as_model(r, state, "the first refit")
        state["triangles"] = deform(state["triangles"], first1, n1, "grow")
        r.update_triangles(first1, state["triangles"][first1:first1 + n1])
        if cached == "every root":
            assert r.rebuild() == advance(state, rows)
        else:
            state["triangles"] = deform(state["triangles"], first0, n0, "grow")
            r.update_triangles(first0, state["triangles"][first0:first0 + n0])
            assert r.rebuild([0]) == advance(state, [rows[0]])
            assert not np.array_equal(bits(original["nodes"][:, [3, 7]]), bits(state["nodes"][:, [3, 7]]))
        same_as_model(r, state, "the rebuild")
        state["triangles"] = deform(state["triangles"], first1, n1, "shrink")
        r.update_triangles(first1, state["triangles"][first1:first1 + n1])
        want = numpy_refit(state["nodes"], state["triangles"], state["lookup"], plan_of(state["nodes"], len(state["lookup"]), roots))
        if cached == "every root":
            # the input condition, on the host alone: the plan of the ORIGINAL trees over the rebuilt nodes gives other bytes
            stale = numpy_refit(state["nodes"], state["triangles"], state["lookup"], plan_of(original["nodes"], len(original["lookup"]), roots))
            assert not np.array_equal(bits(stale), bits(want))
        r.refit(None if cached == "every root" else roots)
        state["nodes"] = want
        same_as_model(r, state, "the refit after the rebuild")
        scene_holds(scene, state, "after the refit")
        ref = oracle_frame(oracle, scene, mat, sky)
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, ref), diff_stats(img, ref)
    finally:
        r.close()


def test_capacity_with_several_ranges_changes_nothing(oracle):
    """Three ranges of the mixed scene, the middle one a node short: RT_ERR_CAPACITY, used[] filled for all three, the message
    names range 1, and nodes, lookup, the next frame and the pair records are what they were.  Two ranges short: the first is
    named."""
    scene, mat = mixed_scene(), rt.Material.white()
    sky = random_sky(50)
    r = make(scene, mat, sky)
    L = r._lib
    try:
        r.render()
        state, rows = host_state(scene, mat), mesh_rows(scene)
        all_used = r.rebuild()
        assert all_used == advance(state, rows)
        r.render()
        before_img, rebuilds = r.read_pixels(), r.stats()["pair_rebuilds"]
        assert np.array_equal(before_img, oracle_frame(oracle, scene, mat, sky))
        want = [all_used[1], all_used[3], all_used[5]]
        for short, named in (((1,), 1), ((0, 2), 0)):
            three = [rows[1], rows[3], rows[5]]
            for k in short:
                three[k] = (three[k][0], want[k] - 1, three[k][2], three[k][3])
            a, used = ranges_array(three), np.full(3, 0xFFFFFFFF, np.uint32)
            assert L.rt_build_blas(r._ctx, a.ctypes.data_as(RANGE), 3, used.ctypes.data_as(U32)) == abi.RT_ERR_CAPACITY
            msg = L.rt_last_error(r._ctx).decode()
            assert used.tolist() == want
            assert ("range %d needs %d nodes, its node_cap is %d" % (named, want[named], want[named] - 1)) in msg, msg
            rc, nd, lk, model_used = build_host(state["triangles"], state["lookup"], state["nodes"], three)
            assert rc == abi.RT_ERR_CAPACITY and model_used.tolist() == want
            assert np.array_equal(bits(nd), bits(state["nodes"])) and np.array_equal(bits(lk), bits(state["lookup"]))
            same_as_model(r, state, "after the refusal")
            r.render()
            assert np.array_equal(r.read_pixels(), before_img) and r.stats()["pair_rebuilds"] == rebuilds
    finally:
        r.close()


def test_a_tight_layout_names_the_mesh_that_does_not_fit(oracle):
    """Two meshes laid out tight, the second the flat grid with its vertices perturbed: rebuild() names mesh 1 -- the index into
    scene.meshes, wherever it stands in the call -- and nothing changes; the mesh that fits is still rebuilt on its own."""
    small, small_tree = mesh_and_tree("T65")
    flat, moved = grid_records(), perturbed_grid_records()
    need = build_tree(soup_of(moved)).used
    assert need > 287
    scene, mat = two_mesh_scene([(small, small_tree), (flat, build_tree(soup_of(flat)))], "tight"), rt.Material.white()
    sky = random_sky(51)
    r = make(scene, mat, sky)
    try:
        r.render()
        r.update_triangles(65, moved)
        r.render()
        state, rows = host_state(scene, mat), mesh_rows(scene)
        assert rows[0][1] == small_tree.used and rows[1][1] == 287
        before_img, rebuilds = r.read_pixels(), r.stats()["pair_rebuilds"]
        assert np.array_equal(before_img, oracle_frame(oracle, scene, mat, sky))
        for meshes in (None, [1, 0], [1]):
            with pytest.raises(abi.RtError) as e:
                r.rebuild(meshes)
            assert e.value.code == abi.RT_ERR_CAPACITY and ("mesh 1 needs %d nodes, has 287" % need) in str(e.value), str(e.value)
            assert "mesh 0" not in str(e.value)
            same_as_model(r, state, "after the refusal of %s" % (meshes,))
            r.render()
            assert np.array_equal(r.read_pixels(), before_img) and r.stats()["pair_rebuilds"] == rebuilds
        assert r.rebuild([0]) == advance(state, [rows[0]]) == [small_tree.used]
        same_as_model(r, state, "rebuild([0])")
        r.render()
        assert np.array_equal(r.read_pixels(), before_img)
    finally:
        r.close()


def test_frames_in_flight_across_a_rebuild(oracle):
    """update_triangles, a query (the corner array is valid), three frames enqueued and not waited for, then rebuild() -- it
    drains them -- and only then the wait: the three are the oracle's on the buffers before the rebuild (new triangles, old nodes,
    old lookup), the next awaited frame the oracle's on the rebuilt ones.  A missing drain would show here only as a race: a pass
    is necessary, not sufficient."""
    scene, mat = full_view_scene()
    sky = random_sky(52)
    r = make(scene, mat, sky)
    try:
        r.render()
        state, rows = host_state(scene, mat), mesh_rows(scene)
        root, first, count = mesh_ranges(scene)[1]
        state["triangles"] = deform(state["triangles"], first, count, "grow")
        r.update_triangles(first, state["triangles"][first:first + count])
        buf = tri_buffers(scene, mat)
        assert np.array_equal(bits(buf["triangles"]), bits(state["triangles"])) and np.array_equal(bits(buf["nodes"]), bits(state["nodes"]))
        o, d = camera_rays(scene, W, H, 4)
        assert check_triangle_hits(oracle, buf, o, d, r.trace_rays(o, d)) > 10
        old_img = oracle_frame(oracle, scene, mat, sky, buf)
        host = r.host_frames(3)
        for f in range(3):
            r.enqueue()
            r.read_pixels_async(0, host[f])
        assert r.rebuild() == advance(state, rows)
        r.wait()
        r.read_pixels_wait()
        new_img = oracle_frame(oracle, scene, mat, sky)
        assert int((old_img != new_img).any(axis=-1).sum()) > 20          # the input condition: the old tree's stale boxes show
        for f in range(3):
            assert np.array_equal(host[f].reshape(H, W, 4), old_img), (f, diff_stats(host[f].reshape(H, W, 4), old_img))
        same_as_model(r, state, "the rebuild behind the frames")
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, new_img), diff_stats(img, new_img)
    finally:
        r.close()
