"""Closest-point queries on the MI355X (include/rt355.h: rt_closest_points, rt_closest_points_host): the kernel against the numpy brute
force over every (instance, slot) pair (tests/closest_common.py: the definition restated), bit for bit on every field -- with the
instance data travelling with the call (up to sixteen instances) and read from the per-frame buffers (more), under the reference's
placeholder top level and a built one, under sheared records written per frame, at the edges of a wave and a workgroup, from host
and from device memory, after every kind of scene change, under masks, on coincident instances, and refused on a sphere scene.
No tolerance anywhere.  Frames are 96 x 64."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from closest_common import ALL, F, assert_same, brute, make_points, mixed_radii, shear_records, twin_scene, with_radius
from helpers import obj_floor, random_sky, tri_buffers, triangle_scene
from refit_common import deform, mesh_ranges

pytestmark = pytest.mark.gpu

W, H, B = 96, 64, 2


def make(scene, mat, sky=None):
    return rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky if sky is not None else random_sky(71), mat)


def host_query(r, points):
    """rt_closest_points_host on the context's state as it is (no host write precedes it) into a buffer of junk"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    out = np.zeros(pts.shape[0], dtype=abi.CLOSEST_DTYPE)
    out.view(np.uint8)[...] = 0x5A
    abi.check(r._lib.rt_closest_points_host(r._ctx, pts.ctypes.data, pts.shape[0], out.ctypes.data), r._ctx)
    return out


def records_of(tensor):
    a = np.ascontiguousarray(tensor.cpu().numpy())
    return a.view(abi.CLOSEST_DTYPE).reshape(a.shape[0])


def as_records(res):
    """the dict of RendererRaytracing.closest_points as (n,) CLOSEST_DTYPE"""
    out = np.zeros(res["dist2"].shape[0], dtype=abi.CLOSEST_DTYPE)
    for f in ("dist2", "u", "v", "prim", "instance", "point"):
        out[f] = res[f]
    return out


def check_state(r, buf, n, seed, what, masks=None, ray_mask=ALL):
    """the host form against the brute force on `buf`, an infinite radius and the mixed ones"""
    pts = make_points(buf, n, seed)
    for points in (with_radius(pts, np.inf), mixed_radii(pts, seed + 1)):
        got = host_query(r, points)
        assert_same(got, brute(buf, points, masks, ray_mask), what)
    return pts


# ---- 1. the scenes ----
def test_six_instances_travel_with_the_call():
    scene, mat = triangle_scene(seed=3, n_models=5)
    r = make(scene, mat)
    try:
        r.recalculateScene()                                  # no frame ever: the instance data is in the call's arguments
        buf = tri_buffers(scene, mat)
        pts = check_state(r, buf, 1500, 31, "seed 3")
        res = r.closest_points(pts, radius=np.inf)           # the wrapper: the same records, dist and mesh beside them
        want = brute(buf, with_radius(pts, np.inf))
        assert_same(as_records(res), want, "RendererRaytracing.closest_points")
        assert np.array_equal(res["dist"], np.sqrt(want["dist2"])) and np.array_equal(res["mesh"], np.asarray(scene.instances.mesh_index)[want["instance"]])
        far = r.closest_points(pts[:7] + F(500.0), radius=1.0)
        assert (far["dist"] == -1).all() and (far["dist2"] == -1).all() and (far["mesh"] == -1).all() and (far["prim"] == -1).all()
        r.render()                                            # a frame builds the relinked pair records: the query does not read them
        check_state(r, buf, 300, 33, "seed 3 after a frame")
        # masks: the winner's instance hidden (word 18 of the records in the arguments), and a ray mask that sees nothing
        winner = int(np.bincount(want["instance"], minlength=6).argmax())
        masks = np.full(6, 0x6, np.uint32)
        masks[winner] = 0x1
        r.set_instance_masks(masks)
        r.set_query_masks(nearest=0x4, occlusion=0x1)        # (the occlusion mask is not the one that counts)
        check_state(r, buf, 400, 35, "the winner hidden", masks, 0x4)
        r.set_query_masks(nearest=0)
        got = host_query(r, with_radius(pts[:100], np.inf))
        assert (got["prim"] == -1).all() and (got["dist2"] == -1).all() and not got["point"].any()
    finally:
        r.close()


def test_sheared_records_written_per_frame():
    scene, mat = triangle_scene(seed=3, n_models=5)
    r = make(scene, mat)
    try:
        r.render()
        sheared = shear_records(tri_buffers(scene, mat))
        scene.frame = dict(scene.frame, blas=np.asarray(sheared["blas"], F).copy())
        r.recalculateScene()                                  # rt_write_blas of six records: kept on the host, carried by the call
        buf = tri_buffers(scene, mat)
        assert np.array_equal(np.asarray(buf["blas"], F).view(np.uint32), np.asarray(sheared["blas"], F).view(np.uint32))
        check_state(r, buf, 1500, 37, "sheared records")
    finally:
        r.close()


def test_twenty_one_instances_read_the_per_frame_buffers():
    scene, mat = triangle_scene(seed=4, n_models=20)
    r = make(scene, mat)
    try:
        r.recalculateScene()
        buf = tri_buffers(scene, mat)
        pts = check_state(r, buf, 700, 41, "21 instances, the reference's top level")
        info = r.build_top_level()
        assert info["nodes_used"] > 1
        built = tri_buffers(scene, mat)
        assert not np.array_equal(np.asarray(built["nodes"]), np.asarray(buf["nodes"]))
        check_state(r, built, 700, 41, "21 instances, a built top level")
        masks = np.full(21, 0x3, np.uint32)
        masks[[2, 5, 20]] = 0x8                               # the device table: two meshes and the floor hidden
        r.set_instance_masks(masks)
        r.set_query_masks(nearest=0x1)
        check_state(r, built, 300, 43, "21 instances, masked", masks, 0x1)
    finally:
        r.close()


def test_a_scene_inside_the_head_of_the_node_buffer():
    """Three instances of a two-triangle floor: five top-level nodes and one bottom-level node, all below node 31 -- such node
    writes stay in the host copy that calls carry, so the bottom-level node too is current only in the staged head."""
    floor = rt.load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 0.8], alignBottom=False, scale=3))
    models = [dict(meshIndex=0, position=[-4.0 + 4.0 * k, 0.5 * k, -6.0], eulers=[0, 25.0 * k, 0]) for k in range(3)]
    scene = rt.SceneRaytracing().createScene([]).createTriangleScene([floor], models)
    assert scene.node_buffer_length() == 6
    mat = rt.Material.white()
    r = make(scene, mat)
    try:
        r.recalculateScene()
        check_state(r, tri_buffers(scene, mat), 500, 47, "a node buffer inside the head")
        r.build_top_level()
        check_state(r, tri_buffers(scene, mat), 500, 47, "a node buffer inside the head, a built top level")
    finally:
        r.close()


# ---- 2. the edges of a wave and of a workgroup; host memory and device memory ----
def test_wave_edges_and_both_forms():
    import torch
    scene, mat = triangle_scene(seed=3, n_models=5)
    r = make(scene, mat)
    try:
        r.recalculateScene()
        buf = tri_buffers(scene, mat)
        points = mixed_radii(make_points(buf, 257, 45), 46)
        want = brute(buf, points)
        side = torch.cuda.Stream()
        for n in (1, 63, 64, 65, 255, 257):
            got = host_query(r, points[:n])
            assert_same(got, want[:n], "n = %d, host memory" % n)
            dev = torch.from_numpy(points[:n].copy()).to("cuda:0")
            out = torch.full((n + 1, 8), 7.0, dtype=torch.float32, device="cuda:0")
            if n == 65:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                # a stream of the caller's
                    back = r.closest_points(dev, out=out[:n])
                side.synchronize()
            else:
                back = r.closest_points(dev, out=out[:n])    # torch's default stream
                torch.cuda.synchronize()
            assert back.data_ptr() == out.data_ptr()
            assert got.tobytes() == records_of(out[:n]).tobytes(), "n = %d: the two forms differ" % n
            assert (out[n] == 7.0).all()                      # nothing written behind the last record
        fresh = r.closest_points(torch.from_numpy(points).to("cuda:0"))
        torch.cuda.synchronize()
        assert fresh.shape == (257, 8) and records_of(fresh).tobytes() == want.tobytes()
        with pytest.raises(ValueError):
            r.closest_points(torch.zeros((4, 3), dtype=torch.float32, device="cuda:0"))
        off = torch.zeros(4 * 5 + 1, dtype=torch.float32, device="cuda:0")[1:].view(5, 4)
        with pytest.raises(abi.RtError) as e:
            r.closest_points(off)                             # not 16-byte aligned
        assert e.value.code == abi.RT_ERR_INVALID_ARG
    finally:
        r.close()


# ---- 3. after scene changes ----
def test_after_a_deformation_and_a_rebuild():
    scene, mat = triangle_scene(seed=40, n_models=3)
    r = make(scene, mat)
    try:
        r.render()
        before = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[0]
        tris = deform(scene.static["triangles"], first, count, "grow")
        r.update_triangles(first, tris[first:first + count])
        r.refit()
        buf = tri_buffers(scene, mat)
        pts = make_points(buf, 400, 51)
        points = with_radius(pts, np.inf)
        want = brute(buf, points)
        assert len(np.nonzero((want["dist2"] != brute(before, points)["dist2"]))[0]) > 50      # the points see the change
        assert_same(host_query(r, points), want, "after update_triangles + refit")
        r.rebuild()
        buf = tri_buffers(scene, mat)
        assert_same(host_query(r, points), brute(buf, points), "after rebuild")
        check_state(r, buf, 300, 53, "after rebuild, the mixed radii")
    finally:
        r.close()


def test_a_turned_mesh_with_a_frame_in_flight(oracle):
    sky = random_sky(72)
    scene, mat = triangle_scene(seed=3, n_models=5)
    r = make(scene, mat, sky)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        ref_old = oracle.render_tri(scene.pack_params(B), old, sky.faces, W, H)[0]
        assert np.array_equal(r.read_pixels(), ref_old)
        host = r.host_frames(1)
        r.enqueue()                                           # a frame of the old pose, not awaited
        r.read_pixels_async(0, host[0])
        scene.update(0.5)
        new = tri_buffers(scene, mat)
        pts = make_points(new, 600, 55)
        res = r.closest_points(pts)                           # writes the new pose as per-frame data: nothing drains
        want = brute(new, with_radius(pts, np.inf))
        assert_same(as_records(res), want, "the pose the next frame shows")
        assert len(np.nonzero(want["dist2"] != brute(old, with_radius(pts, np.inf))["dist2"])[0]) > 50
        r.wait()
        r.read_pixels_wait()
        assert np.array_equal(host[0].reshape(H, W, 4), ref_old)       # the frame in flight kept its pose
        r.enqueue()
        r.wait()
        assert np.array_equal(r.read_pixels(), oracle.render_tri(scene.pack_params(B), new, sky.faces, W, H)[0])
    finally:
        r.close()


# ---- 4. ties ----
def test_coincident_instances_resolve_by_index():
    scene, mat = twin_scene()
    r = make(scene, mat)
    try:
        r.recalculateScene()
        buf = tri_buffers(scene, mat)
        pts = make_points(buf, 600, 57)
        points = with_radius(pts, np.inf)
        want = brute(buf, points)
        assert (want["instance"] == 1).sum() > 60 and not (want["instance"] == 3).any() and (want["dist2"] == 0).sum() > 100
        assert_same(host_query(r, points), want, "coincident instances")
        r.set_instance_masks([ALL, 0, ALL, ALL])              # the lower twin hidden: the upper one answers
        hidden = brute(buf, points, [ALL, 0, ALL, ALL])
        assert (hidden["instance"] == 3).sum() > 60
        assert_same(host_query(r, points), hidden, "the lower twin hidden")
    finally:
        r.close()


# ---- 5. the checks ----
def test_the_checks_in_order_and_a_sphere_scene(oracle, constant_sky):
    cfg = rt.BASELINE_CONFIGS["C1"]
    scene = rt.synthetic_scene(cfg["spheres"], cfg["seed"])
    r = rt.RendererRaytracing(cfg["width"], cfg["height"], scene, maxBounces=cfg["bounces"]).initialize(constant_sky)
    L, vp = r._lib, ctypes.c_void_p
    pts = with_radius(np.zeros((3, 3), F), 1.0)
    out = np.zeros(3, dtype=abi.CLOSEST_DTYPE)
    try:
        inv = abi.RT_ERR_INVALID_ARG
        # before any scene: the context, n == 0, the buffers, then the state
        assert L.rt_closest_points_host(None, vp(pts.ctypes.data), 3, vp(out.ctypes.data)) == inv
        assert L.rt_closest_points_host(r._ctx, None, 0, None) == abi.RT_OK and L.rt_closest_points(r._ctx, None, 0, None, None) == abi.RT_OK
        assert L.rt_closest_points_host(r._ctx, None, 3, vp(out.ctypes.data)) == inv
        assert L.rt_closest_points_host(r._ctx, vp(pts.ctypes.data), 3, None) == inv
        assert L.rt_closest_points(r._ctx, vp(16), 3, None, None) == inv and L.rt_closest_points(r._ctx, vp(20), 3, vp(32), None) == inv
        assert L.rt_closest_points(r._ctx, vp(32), 3, vp(72), None) == inv
        assert L.rt_closest_points_host(r._ctx, vp(pts.ctypes.data), 3, vp(out.ctypes.data)) == abi.RT_ERR_STATE
        r.set_mode(True)
        r.recalculateScene()                                  # spheres
        stats = r.stats()
        assert L.rt_closest_points_host(r._ctx, vp(pts.ctypes.data), 3, vp(out.ctypes.data)) == abi.RT_ERR_UNSUPPORTED
        assert b"sphere" in L.rt_last_error(r._ctx)
        assert L.rt_closest_points_host(r._ctx, None, 3, None) == inv                  # the buffers still come first
        with pytest.raises(abi.RtError) as e:
            r.closest_points(np.zeros((2, 3), F))
        assert e.value.code == abi.RT_ERR_UNSUPPORTED and r.stats() == stats
        r.render()                                            # the context is as usable as before: the golden frame
        golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.json")))["C1"]
        assert hashlib.sha256(r.read_pixels().tobytes()).hexdigest() == golden["sha256"] and r.stats()["rays"] == golden["rays"]
    finally:
        r.close()
