"""Device mesh deformation on the MI355X (include/rt355.h: rt_deform_triangles, rt_deform_triangles_host,
rt_update_triangles_device, rt_read_triangles; RendererRaytracing.deform): the records the kernel leaves against the serial model
and its numpy restatement (tests/deform_common.py) bit for bit, a deformation through deform() against the same records through
update_triangles() + refit() on a second context -- nodes, frames and queries byte for byte, and both against the CPU oracle on
the buffers the scene object then holds --, flat normals against the oracle, the torch path on a side stream, and every refused
call followed by a frame.  No tolerance anywhere.

The scene is refit_common.view_scene(): frames of 64 x 48, meshes of 96 and 176 triangles, 274 triangles in all."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from deform_common import (F, FLAT, NRM_WORDS, POS_WORDS, all_cases, bits, check_records, indexed, make_case, mesh_vertices, model, prepared,
                           same)
from helpers import diff_stats, oracle_render, random_sky, tri_buffers
from query_common import camera_rays, check_all_queries, random_rays, scene_box
from refit_common import B, FP, H, W, deform, mesh_ranges, view_scene
from test_refit_tri_gpu import all_roots, expect_nodes, frames_in_flight, make, oracle_frame

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def on_device(a, dtype=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.view(dtype))).to(DEV)


def dptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def hptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def call_device(r, first, n, case, V=None):
    """rt_deform_triangles on device copies of the case's arrays (made on torch's default stream and complete: no stream to name)"""
    import torch
    v, f, nr = prepared(case["vertices"], case["faces"], case["normals"])
    tv, tf, tn = on_device(v), on_device(f, np.int32), on_device(nr)
    torch.cuda.synchronize()
    rc = r._lib.rt_deform_triangles(r._ctx, first, n, dptr(tv), v.shape[0] if V is None else V, dptr(tf), dptr(tn), case["flags"], None)
    del tv, tf, tn
    return rc


def call_host(r, first, n, case, V=None):
    v, f, nr = prepared(case["vertices"], case["faces"], case["normals"])
    return r._lib.rt_deform_triangles_host(r._ctx, first, n, hptr(v), v.shape[0] if V is None else V, hptr(f), hptr(nr), case["flags"])


def check_against_model(name, got, before, first, n, case):
    rc, want = model(before, first, n, **case)
    assert rc == abi.RT_OK, name
    flat = bool(case["flags"] & FLAT)
    other = np.setdiff1d(np.arange(40), NRM_WORDS) if flat else np.arange(40)
    assert np.array_equal(bits(got[:, other]), bits(want[:, other])), name
    assert same(got[:, NRM_WORDS], want[:, NRM_WORDS]), name                   # a NaN that 0 / 0 makes has no promised sign
    check_records(name, got, before, first, n, case)


def test_the_records_of_both_entry_points_are_the_models():
    """Every argument combination and shape of the CPU list, at 274 triangles: n = 1, 64, 65 (ending at the last triangle) and a
    257-triangle range across the meshes, and the two meshes' own ranges (96 and 176: not multiples of 64); each through device
    memory and through host memory, read back with rt_read_triangles."""
    scene, mat = view_scene()
    r = make(scene, mat, random_sky(41))
    try:
        r.recalculateScene()
        T = scene.triangleCount
        assert T == 274
        cases = all_cases(T)
        for k, (root, first, count) in enumerate(mesh_ranges(scene)[0:2]):
            cases.append(("mesh %d soup flat" % k, first, count, make_case(300 + k, count, False, "flat")))
            cases.append(("mesh %d faces given" % k, first, count, make_case(310 + k, count, True, "given")))
        assert {n for _, _, n, _ in cases} >= {1, 64, 65, 96, 176, 257}
        base = np.ascontiguousarray(scene.pack_triangles(), F)
        assert np.array_equal(bits(r.read_triangles()), bits(base))
        for name, first, n, case in cases:
            for path, call in (("device", call_device), ("host", call_host)):
                before = r.read_triangles()
                assert call(r, first, n, case) == abi.RT_OK, (name, path, r._lib.rt_last_error(r._ctx))
                check_against_model("%s, %s" % (name, path), r.read_triangles(), before, first, n, case)
                r.update_triangles(0, base)                                   # the next call starts from the scene's records
    finally:
        r.close()


def test_update_triangles_device_leaves_the_bytes_of_update_triangles():
    scene, mat = view_scene()
    r = make(scene, mat, random_sky(42))
    try:
        r.recalculateScene()
        base = np.ascontiguousarray(scene.pack_triangles(), F)
        rng = np.random.default_rng(43)
        for first, n in ((0, 1), (5, 65), (scene.triangleCount - 176, 176)):
            rec = rng.standard_normal((n, 40)).astype(F)
            bits(rec)[0, 3] = 0x7FC01234
            r.update_triangles(first, rec)
            want = r.read_triangles()
            assert np.array_equal(bits(want[first:first + n]), bits(rec))
            r.update_triangles(0, base)
            r.update_triangles(first, on_device(rec))
            assert np.array_equal(bits(r.read_triangles()), bits(want))
            assert np.array_equal(bits(scene.to_packed()["triangles"]), bits(want))
            r.update_triangles(0, base)
        with pytest.raises(ValueError):
            r.update_triangles(0, on_device(rec)[:, :39])
        with pytest.raises(abi.RtError) as e:
            r.update_triangles(scene.triangleCount - 1, on_device(rec[:2]))
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        assert np.array_equal(bits(r.read_triangles()), bits(base))
    finally:
        r.close()


@pytest.mark.parametrize("variant", [0, 6])
@pytest.mark.parametrize("kind", ["grow", "shrink"])
def test_deform_is_update_triangles_and_refit(oracle, kind, variant):
    """deform(..., refit=True) from device memory on one context, update_triangles(the model's records) + refit() on another:
    the same nodes, the same awaited frame, the same three frames in flight, the same answers of every query family -- and all
    of them the CPU oracle's on the buffers the scene object holds.  Through the pair records (variant 0) and through the node
    buffer alone (variant 6); the pair records are not rebuilt."""
    sky = random_sky(44)
    scenes = [view_scene(), view_scene()]
    rs = [make(scene, mat, sky, variant) for scene, mat in scenes]
    try:
        for r in rs:
            r.render()
        rebuilds = [r.stats()["pair_rebuilds"] for r in rs]
        assert rebuilds == [0 if variant == 6 else 1] * 2
        old = tri_buffers(*scenes[0])
        root, first, count = mesh_ranges(scenes[0][0])[1]
        assert count == 176
        corners = mesh_vertices(old["triangles"], first, count, kind)
        rc, tris = model(old["triangles"], first, count, corners)
        assert rc == abi.RT_OK and np.array_equal(bits(tris), bits(deform(old["triangles"], first, count, kind)))
        want, plan = expect_nodes(old, tris, all_roots(scenes[0][0]))
        rs[0].deform(first, on_device(corners))
        rs[1].update_triangles(first, tris[first:first + count])
        rs[1].refit()
        bufs = [tri_buffers(scene, mat) for scene, mat in scenes]
        for r, (scene, mat), buf in zip(rs, scenes, bufs):
            assert np.array_equal(bits(r.read_triangles()), bits(tris))
            assert np.array_equal(bits(scene.to_packed()["triangles"]), bits(tris))
            assert np.array_equal(bits(r.read_nodes()), bits(want)) and np.array_equal(bits(buf["nodes"]), bits(want))
        fresh = oracle_frame(oracle, *scenes[0], sky, bufs[0])
        stale = oracle_frame(oracle, *scenes[0], sky, dict(old, triangles=tris))
        if kind == "grow":                          # the input condition of the pixel checks: the deformation and its refit show
            assert int((stale != fresh).any(axis=-1).sum()) > 20
        assert int((oracle_frame(oracle, *scenes[0], sky, old) != fresh).any(axis=-1).sum()) > 20
        params = np.asarray(scenes[0][0].pack_params(B), F)
        lo, hi = scene_box(bufs[0], scenes[0][0])
        sets = [camera_rays(scenes[0][0], W, H, 4), random_rays(lo, hi, 200, 9)]
        rays = (np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
        for k, (r, buf) in enumerate(zip(rs, bufs)):
            r.render()
            img = r.read_pixels()
            assert np.array_equal(img, fresh), (k, diff_stats(img, fresh))
            for f, img in enumerate(frames_in_flight(r)):
                assert np.array_equal(img, fresh), (k, f, diff_stats(img, fresh))
            assert check_all_queries(oracle, r, dict(tri=buf, params=params, faces=sky.faces), rays) > 20
            assert r.stats()["pair_rebuilds"] == rebuilds[k]
    finally:
        for r in rs:
            r.close()


def test_flat_normals_show(oracle):
    """The finer sphere with one normal per face instead of its smooth ones: the oracle's two frames differ (the input condition),
    and the device's frame is the oracle's on the flat records."""
    scene, mat = view_scene()
    sky = random_sky(45)
    r = make(scene, mat, sky)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        root, first, count = mesh_ranges(scene)[1]
        corners = mesh_vertices(old["triangles"], first, count, "grow")
        smooth = model(old["triangles"], first, count, corners)[1]
        rc, flat = model(old["triangles"], first, count, corners, flags=FLAT)
        assert rc == abi.RT_OK
        degenerate = np.isnan(flat[first:first + count][:, NRM_WORDS]).any(axis=1)      # the pole triangles have no area: 0 / 0, never hit
        assert 0 < degenerate.sum() < count // 4
        nodes, _ = expect_nodes(old, flat, all_roots(scene))
        img_smooth = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=smooth, nodes=nodes))
        img_flat = oracle_frame(oracle, scene, mat, sky, dict(old, triangles=flat, nodes=nodes))
        assert int((img_smooth != img_flat).any(axis=-1).sum()) > 20
        r.deform(first, corners, flat_normals=True)
        got = r.read_triangles()
        assert same(got, flat) and np.array_equal(bits(got[:, POS_WORDS]), bits(flat[:, POS_WORDS]))
        assert np.array_equal(bits(tri_buffers(scene, mat)["triangles"]), bits(got))
        assert np.array_equal(bits(tri_buffers(scene, mat)["nodes"]), bits(nodes))
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, img_flat), diff_stats(img, img_flat)
        assert np.array_equal(oracle_frame(oracle, scene, mat, sky), img_flat)
    finally:
        r.close()


def test_the_torch_path(oracle):
    """A (T, 3, 3) tensor made on a side stream, deform() under that stream: the records of the numpy path.  Then the indexed
    form with normals from int32 / float32 tensors, and what deform() refuses before it calls the library."""
    import torch
    scene, mat = view_scene()
    sky = random_sky(46)
    r = make(scene, mat, sky)
    try:
        r.render()
        old = tri_buffers(scene, mat)
        base = old["triangles"].copy()
        root, first, count = mesh_ranges(scene)[1]
        corners = mesh_vertices(base, first, count, "grow")
        r.deform(first, corners)                                              # numpy: rt_deform_triangles_host
        want, want_nodes = r.read_triangles(), r.read_nodes()
        assert np.array_equal(bits(want), bits(deform(base, first, count, "grow")))
        r.update_triangles(0, base)
        r.refit()
        assert np.array_equal(bits(r.read_nodes()), bits(old["nodes"]))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                         # produced on a side stream: the call must wait for it
            t = torch.from_numpy(corners).to(DEV, non_blocking=True) * 1.0
            assert tuple(t.shape) == (count, 3, 3)
            r.deform(first, t)
        assert np.array_equal(bits(r.read_triangles()), bits(want)) and np.array_equal(bits(r.read_nodes()), bits(want_nodes))
        assert np.array_equal(bits(scene.to_packed()["triangles"]), bits(want))
        r.render()
        assert np.array_equal(r.read_pixels(), oracle_frame(oracle, scene, mat, sky))
        # indexed, with normals: (V, 3) float32, (T, 3) int32, on torch's default stream
        verts, faces = indexed(mesh_vertices(base, first, count, "shrink"))
        nrm = np.random.default_rng(47).uniform(-1, 1, verts.shape).astype(F)
        rc, want = model(r.read_triangles(), first, count, verts, faces, nrm)
        assert rc == abi.RT_OK
        r.deform(first, on_device(verts), faces=on_device(faces, np.int32), normals=on_device(nrm), refit=False)
        assert np.array_equal(bits(r.read_triangles()), bits(want))
        before = r.read_triangles()
        t = on_device(corners)
        for bad in (dict(vertices=t.cpu()), dict(vertices=t.double()), dict(vertices=t.transpose(1, 2)), dict(vertices=t[:, :, :2]),
                    dict(vertices=t, faces=on_device(faces, np.int32).long()), dict(vertices=t, normals=on_device(nrm)),
                    dict(vertices=t, faces=faces), dict(vertices=t, flat_normals=True, normals=t)):
            with pytest.raises(ValueError):
                r.deform(first, **bad)
        assert np.array_equal(bits(r.read_triangles()), bits(before))
    finally:
        r.close()


def test_refused_calls_leave_the_scene_usable(oracle):
    """Every check of include/rt355.h, in its order, on both context entry points: the documented status, unchanged records, and
    a frame that is the oracle's after each."""
    import torch
    inv, state, ok = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_STATE, abi.RT_OK
    scene, mat = view_scene()
    sky = random_sky(48)
    r = make(scene, mat, sky)
    L = r._lib
    try:
        r.render()
        ref = oracle_frame(oracle, scene, mat, sky)
        assert np.array_equal(r.read_pixels(), ref)
        T = scene.triangleCount
        base = r.read_triangles()
        v = np.ones((30, 3), F)
        nr = np.ones((30, 3), F)
        tv, tn = on_device(v), on_device(nr)
        torch.cuda.synchronize()

        def frame_is_the_oracles(what):
            assert np.array_equal(bits(r.read_triangles()), bits(base)), what
            r.render()
            assert np.array_equal(r.read_pixels(), ref), what

        def both(first, n, vertices=True, V=30, normals=False, flags=0):
            d = L.rt_deform_triangles(r._ctx, first, n, dptr(tv) if vertices else None, V, None, dptr(tn) if normals else None, flags, None)
            h = L.rt_deform_triangles_host(r._ctx, first, n, hptr(v) if vertices else None, V, None, hptr(nr) if normals else None, flags)
            assert d == h, (d, h)
            return d

        # 1. flags (each call would fail a later check too)
        assert both(T, 1, vertices=False, flags=2) == inv and b"flag" in L.rt_last_error(r._ctx)
        frame_is_the_oracles("unknown flag bits")
        assert both(T, 1, vertices=False, normals=True, flags=FLAT) == inv
        frame_is_the_oracles("flat normals with normals")
        # 3. the range, in 64 bits, before n == 0 and the arrays
        assert both(T - 9, 10) == inv and both(0xFFFFFFFF, 2) == inv and both(T + 1, 0, vertices=False) == inv
        frame_is_the_oracles("beyond the triangles written")
        # 4. n == 0
        assert both(T, 0, vertices=False, V=0) == ok
        frame_is_the_oracles("n == 0")
        # 5. the arrays
        assert both(0, 10, vertices=False) == inv and both(0, 10, V=0) == inv and both(0, 10, V=29) == inv and both(0, 11) == inv
        frame_is_the_oracles("vertices")
        off = ctypes.c_void_p(tv.data_ptr() + 2)
        assert L.rt_deform_triangles(r._ctx, 0, 1, off, 3, None, None, 0, None) == inv and b"aligned" in L.rt_last_error(r._ctx)
        assert L.rt_deform_triangles(r._ctx, 0, 1, dptr(tv), 3, off, None, 0, None) == inv
        assert L.rt_deform_triangles(r._ctx, 0, 1, dptr(tv), 3, None, off, 0, None) == inv
        assert L.rt_update_triangles_device(r._ctx, 0, 1, off, None) == inv
        assert L.rt_update_triangles_device(r._ctx, T, 1, dptr(tv), None) == inv and L.rt_update_triangles_device(r._ctx, 0, 1, None, None) == inv
        assert L.rt_update_triangles_device(r._ctx, T, 0, None, None) == ok
        assert L.rt_read_triangles(r._ctx, T, 1, base.ctypes.data_as(FP)) == inv and L.rt_read_triangles(r._ctx, 0, 1, None) == inv
        frame_is_the_oracles("alignment")
        with pytest.raises(abi.RtError) as e:
            r.deform(T - 1, np.zeros((2, 3, 3), F))
        assert e.value.code == inv
        frame_is_the_oracles("deform() beyond the scene")
        # and a call that is accepted, after all of them
        assert both(T - 10, 10, flags=FLAT) == ok
        assert np.array_equal(bits(r.read_triangles()[:T - 10]), bits(base[:T - 10]))
    finally:
        r.close()


def test_a_sphere_scene_is_a_state_error(oracle):
    """2. and 6.: no triangle scene -- before any scene is written, and with spheres; the sphere frame is the oracle's afterwards"""
    import torch
    scene = rt.synthetic_scene(5, 3)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(None)
    L = r._lib
    try:
        v = np.ones((3, 3), F)
        tv = on_device(v)
        torch.cuda.synchronize()
        for written in (False, True):
            if written:
                r.recalculateScene()
            assert L.rt_deform_triangles(r._ctx, 0, 1, dptr(tv), 3, None, None, 0, None) == abi.RT_ERR_STATE
            assert L.rt_deform_triangles_host(r._ctx, 0, 1, hptr(v), 3, None, None, 0) == abi.RT_ERR_STATE
            assert L.rt_deform_triangles_host(r._ctx, 0, 0, None, 0, None, None, 0) == abi.RT_ERR_STATE          # before n == 0
            assert L.rt_deform_triangles_host(r._ctx, 0, 1, hptr(v), 3, None, None, 2) == abi.RT_ERR_INVALID_ARG    # flags come first
            assert L.rt_update_triangles_device(r._ctx, 0, 1, dptr(tv), None) == abi.RT_ERR_STATE
        r.render()
        assert np.array_equal(r.read_pixels(), oracle_render(oracle, scene, W, H, B)[0])
    finally:
        r.close()
