"""Deforming meshes on the MI355X (include/rt355.h: rt_update_triangles, rt_refit_blas, rt_read_nodes): vertices moved in numpy
float32, written over a part of the triangle buffer, the bottom-level trees refitted on the device -- and then the node buffer
against the numpy restatement of the refit (tests/refit_common.py: numpy_refit) bit for bit, and every frame form and query family
against the CPU oracle on exactly the buffers the scene object then holds, byte for byte.  No tolerance anywhere.

Frames are 64 x 48, meshes 96 and 176 triangles.  That the pixel checks can fail is shown without a GPU
(tests/test_refit_tri_cpu.py: test_the_deformations_can_show_a_stale_box) and asserted again here on the oracle alone."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import deepen_top_level, diff_stats, random_sky, tri_buffers
from query_common import camera_rays, check_all_queries, check_triangle_hits, random_rays, scene_box
from refit_common import (B, F, FP, H, LOOKUP, U32, W, bad_trees, deform, mesh_ranges, numpy_refit, refit_plan, u32f, view_scene)
from test_gbuffer_gpu import hits_of
from test_refit_tri_cpu import one_triangle_scene
from test_render_samples_cpu import resolve_np
from test_render_samples_gpu import check as check_samples

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def make(scene, mat, sky, variant=0):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky, mat)
    r.set_variant(variant)
    return r


def oracle_frame(oracle, scene, mat, sky, buf=None):
    return oracle.render_tri(scene.pack_params(B), buf if buf is not None else tri_buffers(scene, mat), sky.faces, W, H)[0]


def all_roots(scene):
    return sorted(set(u32f(rec[16]) for rec in np.asarray(scene.pack_blas(), F).reshape(-1, 20)))


def expect_nodes(buf, tris, roots):
    """the whole node buffer after a refit of `roots` over the triangles `tris`: numpy_refit over rt_refit_plan's runs"""
    rc, _, plan = refit_plan(buf["nodes"], len(buf["tri_lookup"]), roots)
    assert rc == abi.RT_OK
    return numpy_refit(buf["nodes"], tris, buf["tri_lookup"], plan), plan


def frames_in_flight(r, n=3):
    host = r.host_frames(n)
    for f in range(n):
        r.enqueue()
        r.read_pixels_async(0, host[f])
    r.wait()
    r.read_pixels_wait()
    return [h.reshape(H, W, 4) for h in host]


CASES = {"tiny": (3, 0, 0, 1), "node_buffer": (3, 0, 6, 0), "deep": (11, 7, 0, 0)}      # n_models, extra top-level levels, variant, tri_form (the small forms walk pair records)


@pytest.mark.parametrize("kind", ["grow", "shrink"])
@pytest.mark.parametrize("case", list(CASES))
def test_deformed_mesh_nodes_and_frames(oracle, case, kind):
    """update_triangles + refit of every root: the node bytes, an awaited frame and three frames in flight -- through the pair
    records (variant 0), through the node buffer alone (variant 6), and in the twenty-slot form, whose frames bring a version of
    the per-frame buffers up to date from the host's copy of the buffer's head (the BLAS nodes below node 31 live there too)."""
    n_models, deepen, variant, form = CASES[case]
    scene, mat = view_scene(n_models)
    sky = random_sky(31)
    if deepen:
        deepen_top_level(scene, min(deepen, (scene.tlasNodesMax - len(scene.frame["tlas_nodes"])) // 2))
    r = make(scene, mat, sky, variant)
    try:
        r.render()
        assert np.array_equal(r.read_pixels(), oracle_frame(oracle, scene, mat, sky))
        assert r.stats()["tri_form"] == form
        rebuilds = r.stats()["pair_rebuilds"]
        assert rebuilds == (0 if variant == 6 else 1)
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        tris = deform(old["triangles"], first, count, kind)
        want, plan = expect_nodes(old, tris, all_roots(scene))
        assert plan.shape[0] == scene.blasNodesUsed
        stale = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=tris))
        fresh = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=tris, nodes=want))
        if kind == "grow":                          # the input condition of the pixel checks: a stale box shows
            assert int((stale != fresh).any(axis=-1).sum()) > 20
        r.update_triangles(first, tris[first:first + count])
        r.refit()
        got = r.read_nodes()
        assert got.shape == want.shape
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, "nodes %s differ from the numpy refit" % bad[:8]
        assert np.array_equal(bits(got[:, [3, 7]]), bits(old["nodes"][:, [3, 7]]))
        untouched = np.setdiff1d(np.arange(got.shape[0]), plan[:, 0])
        assert np.array_equal(bits(got[untouched]), bits(old["nodes"][untouched]))
        # the scene object describes the device: to_packed() feeds the oracle directly
        packed = scene.to_packed()
        assert np.array_equal(bits(packed["triangles"]), bits(tris))
        assert np.array_equal(bits(packed["blas_nodes"]), bits(want[scene.tlasNodesMax:]))
        assert np.array_equal(bits(tri_buffers(scene, mat)["nodes"]), bits(want))
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, fresh), diff_stats(img, fresh)
        assert r.stats()["tri_form"] == form
        for f, img in enumerate(frames_in_flight(r)):
            assert np.array_equal(img, fresh), (f, diff_stats(img, fresh))
        r.render()                                  # and an awaited one behind them
        assert np.array_equal(r.read_pixels(), fresh)
        assert r.stats()["pair_rebuilds"] == rebuilds
    finally:
        r.close()


@pytest.mark.parametrize("kind", ["grow", "shrink"])
def test_deformed_mesh_queries(oracle, kind):
    """Every query family (tests/query_common.py: check_all_queries -- the shaded query with compose among them), a 2 x 2
    supersampled frame and a geometry frame on the refitted scene, and the rebuild count of the pair records."""
    scene, mat = view_scene()
    sky = random_sky(32)
    r = make(scene, mat, sky)
    try:
        r.render()
        rebuilds = r.stats()["pair_rebuilds"]
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        tris = deform(old["triangles"], first, count, kind)
        r.update_triangles(first, tris[first:first + count])
        r.refit()
        buf = tri_buffers(scene, mat)
        assert np.array_equal(bits(buf["nodes"]), bits(expect_nodes(old, tris, all_roots(scene))[0]))
        params = np.asarray(scene.pack_params(B), F)
        state = dict(tri=buf, params=params, faces=sky.faces)
        lo, hi = scene_box(buf, scene)
        sets = [camera_rays(scene, W, H, 2), random_rays(lo, hi, 400, 9)]
        rays = (np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
        assert check_all_queries(oracle, r, state, rays) > 100
        big = oracle.render_tri(params, buf, sky.faces, 2 * W, 2 * H, want_float=True)[1]
        img, flt = r.render_samples(2, float_out=True)
        check_samples(img, flt, resolve_np(big, 2), "2 x 2 after a refit")
        o, d = camera_rays(scene, W, H)
        assert check_triangle_hits(oracle, buf, o, d, hits_of(r.render_gbuffer())) > 100
        assert r.stats()["pair_rebuilds"] == rebuilds
    finally:
        r.close()


def test_selective_refit_honours_a_stale_box(oracle):
    """Two meshes move, one root is refitted: the other tree keeps its bytes and the frame is the oracle's on exactly those buffers
    -- the stale boxes cut the grown mesh, and nothing fixes that silently.  Then the second root."""
    scene, mat = view_scene()
    sky = random_sky(33)
    r = make(scene, mat, sky)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        (root0, first0, count0), (root1, first1, count1) = mesh_ranges(scene)[0:2]
        tris = deform(deform(old["triangles"], first0, count0, "grow"), first1, count1, "grow", phase=1.0)
        half, plan0 = expect_nodes(old, tris, [root0])
        full, _ = expect_nodes(old, tris, [root0, root1])
        img_half = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=tris, nodes=half))
        img_full = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=tris, nodes=full))
        assert int((img_half != img_full).any(axis=-1).sum()) > 20          # the input condition: the stale tree shows
        r.update_triangles(first0, tris[first0:first0 + count0])
        r.update_triangles(first1, tris[first1:first1 + count1])
        r.refit([root0])
        got = r.read_nodes()
        assert np.array_equal(bits(got), bits(half))
        other = np.setdiff1d(np.arange(got.shape[0]), plan0[:, 0])
        assert np.array_equal(bits(got[other]), bits(old["nodes"][other]))
        assert np.array_equal(bits(tri_buffers(scene, mat)["nodes"]), bits(half))
        r.render()
        assert np.array_equal(r.read_pixels(), img_half), diff_stats(r.read_pixels(), img_half)
        r.refit([root1, root1])                     # a root named twice is refitted once
        assert np.array_equal(bits(r.read_nodes()), bits(full))
        r.render()
        assert np.array_equal(r.read_pixels(), img_full), diff_stats(r.read_pixels(), img_full)
        assert r.stats()["pair_rebuilds"] == 1
    finally:
        r.close()


@pytest.mark.parametrize("builder", ["procedural", "one triangle"])
def test_refit_without_a_vertex_change_is_the_identity(oracle, builder):
    """The builders' boxes are the float32 min / max of the corners: the device gives them back bit for bit -- also before any
    frame (no pair records yet), and for a root that is a leaf."""
    scene, mat = view_scene() if builder == "procedural" else (one_triangle_scene(), rt.Material.white())
    sky = random_sky(34)
    r = make(scene, mat, sky)
    try:
        before = tri_buffers(scene, mat)["nodes"].copy()
        r.refit()                                   # before the first frame
        assert np.array_equal(bits(r.read_nodes()), bits(before))
        r.render()
        ref = oracle_frame(oracle, scene, mat, sky)
        assert np.array_equal(r.read_pixels(), ref)
        r.refit()
        r.refit(all_roots(scene))                   # the cached plan again
        assert np.array_equal(bits(r.read_nodes()), bits(before))
        assert np.array_equal(bits(scene.static["blas_nodes"]), bits(before[scene.tlasNodesMax:]))
        r.render()
        assert np.array_equal(r.read_pixels(), ref) and r.stats()["pair_rebuilds"] == 1
        if builder == "one triangle":               # the leaf root moves: its box follows
            root, first, count = mesh_ranges(scene)[0]
            assert count == 1
            old = tri_buffers(scene, mat)
            tris = deform(old["triangles"], first, count, "grow")
            want, _ = expect_nodes(old, tris, all_roots(scene))
            r.update_triangles(first, tris[first:first + 1])
            r.refit()
            assert np.array_equal(bits(r.read_nodes()), bits(want)) and not np.array_equal(bits(want), bits(before))
            r.render()
            assert np.array_equal(r.read_pixels(), oracle_frame(oracle, scene, mat, sky))
    finally:
        r.close()


def test_frames_in_flight_keep_the_old_scene(oracle):
    """Three frames enqueued, then update_triangles + refit (they drain), then a frame: the first three are the old scene's bytes."""
    scene, mat = view_scene()
    sky = random_sky(35)
    r = make(scene, mat, sky)
    try:
        r.render()
        old_img = oracle_frame(oracle, scene, mat, sky)
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        tris = deform(old["triangles"], first, count, "grow")
        host = r.host_frames(4)
        for f in range(3):
            r.enqueue()
            r.read_pixels_async(0, host[f])
        r.update_triangles(first, tris[first:first + count])
        r.refit()
        r.enqueue()
        r.read_pixels_async(0, host[3])
        r.wait()
        r.read_pixels_wait()
        new_img = oracle_frame(oracle, scene, mat, sky)
        assert int((old_img != new_img).any(axis=-1).sum()) > 20
        for f in range(3):
            assert np.array_equal(host[f].reshape(H, W, 4), old_img), f
        assert np.array_equal(host[3].reshape(H, W, 4), new_img)
    finally:
        r.close()


def test_an_animation_loop_of_eight_steps(oracle):
    """Per step one pose change (rt_write_blas travels with the frame) and one deformation through update_triangles + refit: every
    frame is the oracle's, instance_uploads keeps counting, and the pair records are never rebuilt after the first frame."""
    scene, mat = view_scene()
    sky = random_sky(36)
    r = make(scene, mat, sky)
    try:
        r.render()
        rebuilds, uploads = r.stats()["pair_rebuilds"], r.stats()["instance_uploads"]
        assert rebuilds == 1
        base = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        for step in range(8):
            scene.update(0.2)
            tris = deform(base["triangles"], first, count, "grow" if step % 2 == 0 else "shrink", phase=0.7 * step)
            want, _ = expect_nodes(base, tris, all_roots(scene))
            r.update_triangles(first, tris[first:first + count])
            r.refit()
            r.render()
            buf = tri_buffers(scene, mat)
            assert np.array_equal(bits(buf["nodes"][scene.tlasNodesMax:]), bits(want[scene.tlasNodesMax:])), step
            ref = oracle_frame(oracle, scene, mat, sky, buf)
            assert np.array_equal(r.read_pixels(), ref), (step, diff_stats(r.read_pixels(), ref))
            st = r.stats()
            assert st["instance_uploads"] == uploads + step + 1 and st["pair_rebuilds"] == rebuilds, (step, st)
    finally:
        r.close()


def rebase(nodes, node_base, slot_base):
    out = np.array(nodes, F).copy()
    for row in out:
        if u32f(row[7]) == 0:
            if row[3] < 1e6:
                row[3] += node_base
        else:
            row[3] += slot_base
    return out


def test_error_paths_change_nothing(oracle):
    """The bad trees of tests/test_refit_tri_cpu.py, written behind the scene's own nodes (no instance names them, so frames do not
    see them) and refitted by their root: the documented status, and afterwards the node buffer and a frame are what they were."""
    scene, mat = view_scene()
    sky = random_sky(37)
    r = make(scene, mat, sky)
    L = r._lib
    try:
        r.render()
        ref = oracle_frame(oracle, scene, mat, sky)
        assert np.array_equal(r.read_pixels(), ref)
        n_scene, n_lookup = scene.node_buffer_length(), len(scene.pack_tri_lookup())
        cases = sorted(bad_trees().items(), key=lambda kv: kv[1][0].shape[0])            # the node count never shrinks: small first
        total = n_scene
        for name, (tree, roots, want) in cases:
            t = np.ascontiguousarray(rebase(tree, n_scene, n_lookup - LOOKUP))
            abi.check(L.rt_write_nodes(r._ctx, 32 * n_scene, t.ctypes.data_as(FP), t.shape[0]), r._ctx)
            total = max(total, n_scene + t.shape[0])
            r.render()
            assert np.array_equal(r.read_pixels(), ref), name
            before, rebuilds = r.read_nodes(0, total), r.stats()["pair_rebuilds"]
            with pytest.raises(abi.RtError) as e:
                r.refit([n_scene + k for k in roots])
            assert e.value.code == want, (name, e.value)
            assert np.array_equal(bits(r.read_nodes(0, total)), bits(before)), name
            r.render()
            assert np.array_equal(r.read_pixels(), ref) and r.stats()["pair_rebuilds"] == rebuilds, name
        # the scene's own trees: a root named together with one of its children, and a partial write beyond the triangles
        root = mesh_ranges(scene)[0][0]
        child = u32f(tri_buffers(scene, mat)["nodes"][root, 3])
        before = r.read_nodes()
        with pytest.raises(abi.RtError) as e:
            r.refit([root, child])
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        rec = np.zeros((2, 40), F)
        with pytest.raises(abi.RtError) as e:
            r.update_triangles(scene.triangleCount - 1, rec)
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        assert L.rt_update_triangles(r._ctx, 0xFFFFFFFF, 2, rec.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG       # the sum in 64 bits
        assert L.rt_update_triangles(r._ctx, scene.triangleCount, 0, None) == abi.RT_OK
        assert L.rt_update_triangles(r._ctx, 0, 1, None) == abi.RT_ERR_INVALID_ARG
        assert L.rt_update_triangles(None, 0, 1, rec.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG
        assert L.rt_refit_blas(None, None, 0) == abi.RT_ERR_INVALID_ARG
        assert L.rt_refit_blas(r._ctx, None, 1) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_nodes(r._ctx, 0, 1, None) == abi.RT_ERR_INVALID_ARG
        assert L.rt_read_nodes(r._ctx, scene.node_buffer_length() + 64, 1, before.ctypes.data_as(FP)) == abi.RT_ERR_INVALID_ARG
        assert np.array_equal(bits(r.read_nodes()), bits(before))
        r.render()
        assert np.array_equal(r.read_pixels(), ref)
    finally:
        r.close()


def test_a_sphere_scene_is_a_state_error():
    scene = rt.synthetic_scene(5, 3)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(None)
    try:
        r.recalculateScene()
        rec = np.zeros((1, 40), F)
        assert r._lib.rt_update_triangles(r._ctx, 0, 1, rec.ctypes.data_as(FP)) == abi.RT_ERR_STATE
        assert r._lib.rt_refit_blas(r._ctx, None, 0) == abi.RT_ERR_STATE
        root = np.zeros(1, np.uint32)
        assert r._lib.rt_refit_blas(r._ctx, root.ctypes.data_as(U32), 1) == abi.RT_ERR_STATE
    finally:
        r.close()
