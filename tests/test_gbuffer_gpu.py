"""Geometry frames on the MI355X (include/rt355.h: rt_render_gbuffer, rt_render_gbuffer_host): the planes of a 41 x 23 frame --
ragged against the 8 x 8 tile of a wave and the 32 x 8 pixels of a workgroup -- against the CPU oracle, the float32 restatements of
tests/query_common.py and rt_pick, on float bits and integers, no tolerance anywhere and no pixel left out."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import tri_buffers, triangle_scene
from query_common import F, _check_sphere_nearest, bits, camera_rays, check_triangle_hits, same
from test_gbuffer_cpu import spheres_with_a_view
from test_render_samples_gpu import TRI

pytestmark = pytest.mark.gpu

W, H = 41, 23
N = W * H
NAMES = ("depth", "normal", "ids", "uv")
RECTS = [(3, 5, 17, 9), (40, 22, 1, 1), (0, 0, 41, 1), (33, 0, 8, 23), None]
TRI_HITS = {"ref": 566, "spine24": 275, "leafy3": 367, "inst3": 563, "inst13": 572, "inst17": 576}   # the oracle's, of 943


def make_renderer(scene, mat=None, w=W, h=H, **kw):
    r = rt.RendererRaytracing(w, h, scene, maxBounces=2, **kw).initialize(None, mat)
    r.recalculateScene()
    return r


def hits_of(g):
    """The four planes of a rectangle as the dict of flat rt_hit fields check_triangle_hits and pick() deal in."""
    assert g["depth"].dtype == np.float32 and g["normal"].dtype == np.float32 and g["ids"].dtype == np.int32 and g["uv"].dtype == np.float32
    h, w = g["depth"].shape
    assert g["normal"].shape == (h, w, 4) and g["ids"].shape == (h, w, 2) and g["uv"].shape == (h, w, 2)
    assert np.all(bits(g["normal"][:, :, 3]) == 0), "word 3 of the normal plane is not +0"
    return {"t": g["depth"].reshape(-1), "u": g["uv"][:, :, 0].reshape(-1), "v": g["uv"][:, :, 1].reshape(-1),
            "prim": g["ids"][:, :, 0].reshape(-1), "instance": g["ids"][:, :, 1].reshape(-1),
            "normal": np.ascontiguousarray(g["normal"][:, :, 0:3]).reshape(-1, 3)}


def same_planes(a, b, names=NAMES):
    return all(np.array_equal(np.ascontiguousarray(a[n]).view(np.uint32), np.ascontiguousarray(b[n]).view(np.uint32)) for n in names)


def crop(g, rect):
    if rect is None:
        return g
    x0, y0, w, h = rect
    return {n: a[y0:y0 + h, x0:x0 + w] for n, a in g.items()}


CANARY = 64


def device_planes(w, h, names=NAMES):
    """Per name a flat tensor of w h pixels and CANARY elements more, every element 7, and the (h, w[, k]) view of its head."""
    import torch
    flat, view = {}, {}
    for n in names:
        tail, dtype, _ = abi.GBUFFER_PLANES[n]
        k = int(np.prod(tail, dtype=np.int64))
        flat[n] = torch.full((w * h * k + CANARY,), 7, dtype=torch.int32 if dtype == "<i4" else torch.float32, device="cuda:0")
        view[n] = flat[n][:w * h * k].view((h, w) + tail)
    return flat, view


def canaries_intact(flat, w, h):
    return all(bool((t[t.numel() - CANARY:] == 7).all()) for t in flat.values())


def to_numpy(view):
    return {n: t.cpu().numpy() for n, t in view.items()}


# ---- 1. triangles against the oracle: every launch form, before the first frame and after one ----------------------------------------
@pytest.mark.parametrize("name", list(TRI))
def test_triangles_against_the_oracle(oracle, name):
    scene, mat = TRI[name]()
    buf = tri_buffers(scene, mat)
    o, d = camera_rays(scene, W, H)
    r = make_renderer(scene, mat)
    try:
        for when in ("before the first frame", "after a frame"):
            g = r.render_gbuffer()
            hits = check_triangle_hits(oracle, buf, o, d, hits_of(g))
            assert 0 < hits < N and hits == TRI_HITS[name], "%s %s: %d hits" % (name, when, hits)
            r.render()
            r.read_pixels()                               # (builds the relinked pair records where the scene fits them)
    finally:
        r.close()


# ---- 2. spheres against the float32 restatement ----------------------------------------------------------------------------------------
def sphere_cases():
    return {"one chunk": lambda: rt.synthetic_scene(37, 11), "two chunks": lambda: rt.synthetic_scene(1100, 11),
            "with a view": lambda: spheres_with_a_view()[0]}


@pytest.mark.parametrize("case", list(sphere_cases()))
def test_spheres_against_the_restatement(oracle, case):
    scene = sphere_cases()[case]()
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    o, d = camera_rays(scene, W, H)
    r = make_renderer(scene)
    try:
        g = r.render_gbuffer()
        hits = _check_sphere_nearest(oracle, sp, o, d, hits_of(g), F(0.001), F(9999.0))
        assert 0 < hits < N, hits
    finally:
        r.close()


# ---- 3 - 6. rt_pick, rectangles, plane subsets, the device form -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["inst3", "spheres"])
def subject(request):
    """One triangle and one sphere scene: the renderer, and the four whole-frame planes of the host form (never written to)."""
    if request.param == "spheres":
        scene, mat = spheres_with_a_view()[0], None
    else:
        scene, mat = TRI[request.param]()
    r = make_renderer(scene, mat)
    whole = r.render_gbuffer()
    for a in whole.values():
        a.setflags(write=False)
    yield r, whole
    r.close()


def test_equal_to_pick(subject):
    r, whole = subject
    ys, xs = np.mgrid[0:H, 0:W]
    p = r.pick(xs.reshape(-1), ys.reshape(-1))
    h = hits_of(whole)
    assert 0 < int((p["prim"] >= 0).sum()) < N
    for k in ("t", "u", "v", "normal"):
        assert same(p[k], h[k]), k
    for k in ("prim", "instance"):
        assert p[k].dtype == np.int32 and np.array_equal(p[k], h[k]), k


@pytest.mark.parametrize("rect", RECTS, ids=[str(q) for q in RECTS])
def test_rectangles(subject, rect):
    r, whole = subject
    want = crop(whole, rect)
    w, h = (rect[2], rect[3]) if rect else (W, H)
    assert same_planes(r.render_gbuffer(rect), want)
    flat, view = device_planes(w, h)
    import torch
    assert r.render_gbuffer(rect, out=view) is view
    torch.cuda.synchronize()
    assert same_planes(to_numpy(view), want)
    assert canaries_intact(flat, w, h)


@pytest.mark.parametrize("name", NAMES)
def test_plane_subsets(subject, name):
    import torch
    r, whole = subject
    alone = r.render_gbuffer(planes=(name,))
    assert list(alone) == [name] and same_planes(alone, whole, (name,))
    # the library directly: the planes not asked for are NULL in rt_gbuffer, and tensors the call was not given keep every element
    flat, view = device_planes(W, H)
    assert r.render_gbuffer(out={name: view[name]})[name] is view[name]
    torch.cuda.synchronize()
    assert same_planes(to_numpy({name: view[name]}), whole, (name,))
    for other in NAMES:
        if other != name:
            assert bool((flat[other] == 7).all()), "%s was written by a call that asked for %s" % (other, name)
    assert canaries_intact(flat, W, H)


def test_device_form_on_a_side_stream(subject):
    import torch
    r, whole = subject
    flat, view = device_planes(W, H)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert r.render_gbuffer(out=view) is view
    side.synchronize()
    assert same_planes(to_numpy(view), whole)
    assert canaries_intact(flat, W, H)


# ---- 7. the pose no frame has carried --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst", [3, 17])
def test_planes_see_the_pose_no_frame_has_carried(oracle, n_inst):
    """Three instances travel in the kernel's arguments; seventeen are read from a version of the per-frame buffers."""
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    o, d = camera_rays(scene, W, H)
    r = make_renderer(scene, mat)
    try:
        r.render()                                        # a frame carries the first pose
        r.read_pixels()
        old = oracle.trace_tri_rays(tri_buffers(scene, mat), o, d)
        scene.update(0.5)
        r.recalculateScene()                              # rt_write_blas / _blas_lookup / _nodes of the new pose, and no frame
        buf = tri_buffers(scene, mat)
        assert not same(old, oracle.trace_tri_rays(buf, o, d))      # the poses differ where the camera looks
        hits = check_triangle_hits(oracle, buf, o, d, hits_of(r.render_gbuffer()))
        assert 0 < hits < N
    finally:
        r.close()


# ---- 8. beside frames in flight; the statistics -----------------------------------------------------------------------------------------
def test_planes_do_not_disturb_frames_or_stats(oracle):
    import torch
    scene, mat = triangle_scene(seed=80, n_models=3)
    r = make_renderer(scene, mat)
    try:
        buf = tri_buffers(scene, mat)
        o, d = camera_rays(scene, W, H)
        r.render()
        frames = r.host_frames(4)
        flat, view = device_planes(W, H)

        def batch(query):
            for _ in range(4):
                r.enqueue()
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    r.render_gbuffer(out=view)
            r.enqueue()
            for k in range(4):
                r.read_pixels_async(k, frames[k])
            r.wait()
            r.read_pixels_wait()
            if query:
                side.synchronize()
            return [f.copy() for f in frames] + [r.read_pixels()]

        batch(False)
        plain = batch(False)              # (the library now knows the caller keeps frames in flight: the same form for both)
        s0 = r.stats()
        beside = batch(True)
        s1 = r.stats()
        ref = oracle.render_tri(np.asarray(scene.pack_params(2), F), buf, r.skyboxMaterial.faces, W, H)[0]
        for a, b in zip(plain, beside):
            assert np.array_equal(a, b) and np.array_equal(b, ref)
        assert s1["frames"] == s0["frames"] + 5 and s1["batch_frames"] == s0["batch_frames"]
        for k in ("rays", "kernel_id", "tri_form"):
            assert s1[k] == s0[k], k
        g = to_numpy(view)
        hits = check_triangle_hits(oracle, buf, o, d, hits_of(g))
        assert 0 < hits < N and canaries_intact(flat, W, H)
        before = r.stats()
        again = r.render_gbuffer()
        after = r.stats()
        for k in before:
            assert after[k] == before[k], k                          # the call changes no statistic, field by field
        assert same_planes(again, g)
        # heatmap, strict mode, the node-walk variant: the same planes
        for setup in (r.showHeatmap, lambda: (r.showRaytracer(), r.set_mode(True)), lambda: r.set_variant(6)):
            setup()
            assert same_planes(r.render_gbuffer(), g)
    finally:
        r.close()


# ---- 9. scene switches on one context ---------------------------------------------------------------------------------------------------
def test_scene_switches_on_one_context(oracle):
    sph_a, sph_b = rt.synthetic_scene(1100, 11), spheres_with_a_view()[0]
    tri, mat = TRI["inst3"]()
    r = make_renderer(sph_a)
    try:
        for scene, m in ((sph_a, None), (tri, mat), (sph_b, None)):
            r.scene, r.loaded = scene, False              # everything is written again by the next recalculateScene()
            if m is not None:
                r.meshMaterial = m
            o, d = camera_rays(scene, W, H)
            h = hits_of(r.render_gbuffer())
            if m is not None:
                hits = check_triangle_hits(oracle, tri_buffers(scene, m), o, d, h)
            else:
                sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
                hits = _check_sphere_nearest(oracle, sp, o, d, h, F(0.001), F(9999.0))
            assert 0 < hits < N
    finally:
        r.close()


# ---- a partitioned context still gives the whole frame ---------------------------------------------------------------------------------
def test_a_partitioned_context_returns_the_whole_frame():
    scene = spheres_with_a_view()[0]
    r = make_renderer(scene)
    try:
        whole = r.render_gbuffer()
    finally:
        r.close()
    r = make_renderer(scene, rank=1, world=2)                         # rt_set_partition(1, 2)
    try:
        assert 0 < int((whole["depth"] > 0).sum()) < N
        assert same_planes(r.render_gbuffer(), whole)
        assert same_planes(r.render_gbuffer((3, 5, 17, 9)), crop(whole, (3, 5, 17, 9)))
    finally:
        r.close()


# ---- 10. errors that need a context, in the header's order --------------------------------------------------------------------------------
def test_errors_in_the_headers_order():
    import torch
    lib = abi.load()
    fp = ctypes.POINTER(ctypes.c_float)
    vp = ctypes.c_void_p
    scene = rt.synthetic_scene(3, 1)
    flat, view = device_planes(16, 16)
    host = {n: np.full((16, 16) + abi.GBUFFER_PLANES[n][0], 7, abi.GBUFFER_PLANES[n][1]) for n in NAMES}
    dev_gb = abi.RtGbuffer(**{n: t.data_ptr() for n, t in view.items()})
    host_gb = abi.RtGbuffer(**{n: a.ctypes.data for n, a in host.items()})
    none_gb = abi.RtGbuffer()
    odd_gb = abi.RtGbuffer(depth=view["depth"].data_ptr(), normal=view["normal"].data_ptr() + 4)
    rect = lambda *q: (ctypes.c_uint32 * 4)(*q)
    both = {"rt_render_gbuffer": (lambda c, q, g, cap: lib.rt_render_gbuffer(c, q, g, cap, None), dev_gb),
            "rt_render_gbuffer_host": (lambda c, q, g, cap: lib.rt_render_gbuffer_host(c, q, g, cap), host_gb)}
    ctx = vp()
    abi.check(lib.rt_create(0, ctypes.byref(ctx)))
    try:
        def state_error(word):
            """RT_ERR_STATE naming `word` -- before the (empty) rectangle and the (short) capacity are looked at, after the arguments"""
            for name, (call, gb) in both.items():
                for q, cap in ((None, 256), (rect(0, 0, 0, 0), 0), (rect(0xFFFFFFFF, 0, 2, 1), 0)):
                    assert call(ctx, q, ctypes.byref(gb), cap) == abi.RT_ERR_STATE, name
                    assert word in lib.rt_last_error(ctx) and name.encode() + b":" in lib.rt_last_error(ctx)
                # the argument checks come first
                assert call(ctx, None, None, 256) == abi.RT_ERR_INVALID_ARG and b"out is NULL" in lib.rt_last_error(ctx)
                assert call(ctx, None, ctypes.byref(none_gb), 256) == abi.RT_ERR_INVALID_ARG and b"planes are NULL" in lib.rt_last_error(ctx)
            assert lib.rt_render_gbuffer(ctx, None, ctypes.byref(odd_gb), 256, None) == abi.RT_ERR_INVALID_ARG
            assert b"aligned" in lib.rt_last_error(ctx)

        state_error(b"rt_resize")
        abi.check(lib.rt_resize(ctx, 16, 16), ctx)
        state_error(b"no scene")
        sp = np.ascontiguousarray(scene.pack_spheres(), dtype=F)
        abi.check(lib.rt_write_spheres(ctx, sp.ctypes.data_as(fp), sp.shape[0]), ctx)
        state_error(b"rt_write_params")
        p = scene.pack_params(2)
        abi.check(lib.rt_write_params(ctx, p.ctypes.data_as(fp)), ctx)
        # the state is complete (no cube map face was ever written: not an error here)
        for name, (call, gb) in both.items():
            g = ctypes.byref(gb)
            for q in (rect(0, 0, 0, 4), rect(0, 0, 4, 0), rect(0xFFFFFFFF, 0, 2, 1), rect(0, 0xFFFFFFFF, 1, 2), rect(15, 0, 2, 1),
                      rect(0, 15, 1, 2), rect(16, 16, 1, 1), rect(0, 0, 17, 16)):
                for cap in (0, 1 << 40):                             # the rectangle before the capacity
                    assert call(ctx, q, g, cap) == abi.RT_ERR_INVALID_ARG, (name, list(q))
                    assert b"rectangle" in lib.rt_last_error(ctx)
            assert call(ctx, None, g, 255) == abi.RT_ERR_CAPACITY
            assert call(ctx, rect(3, 5, 7, 9), g, 62) == abi.RT_ERR_CAPACITY and b"63 pixels" in lib.rt_last_error(ctx)
            assert call(ctx, None, None, 256) == abi.RT_ERR_INVALID_ARG and b"out is NULL" in lib.rt_last_error(ctx)
            assert call(ctx, None, ctypes.byref(none_gb), 256) == abi.RT_ERR_INVALID_ARG and b"planes are NULL" in lib.rt_last_error(ctx)
        assert lib.rt_render_gbuffer(ctx, rect(0, 0, 0, 0), ctypes.byref(odd_gb), 0, None) == abi.RT_ERR_INVALID_ARG
        assert b"aligned" in lib.rt_last_error(ctx)
        for odd in (abi.RtGbuffer(depth=view["depth"].data_ptr() + 2), abi.RtGbuffer(ids=view["ids"].data_ptr() + 4),
                    abi.RtGbuffer(uv=view["uv"].data_ptr() + 4), abi.RtGbuffer(normal=view["normal"].data_ptr() + 8)):
            assert lib.rt_render_gbuffer(ctx, None, ctypes.byref(odd), 256, None) == abi.RT_ERR_INVALID_ARG
        # (the host form has no alignment to ask for)
        off = abi.RtGbuffer(normal=host["normal"].ctypes.data + 4)
        assert lib.rt_render_gbuffer_host(ctx, rect(0, 0, 15, 15), ctypes.byref(off), 225) == abi.RT_OK
        # the refused calls wrote nothing; a call that is not refused does
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in flat.values())
        assert all(np.all(a == 7) for n, a in host.items() if n != "normal")
        for name, (call, gb) in both.items():
            assert call(ctx, None, ctypes.byref(gb), 256) == abi.RT_OK, lib.rt_last_error(ctx)
        torch.cuda.synchronize()
        assert same_planes(to_numpy(view), host) and not np.all(host["depth"] == 7)
        assert canaries_intact(flat, 16, 16)
    finally:
        lib.rt_destroy(ctx)
