"""Supersampled frames on the MI355X (include/rt355.h: rt_render_samples, rt_render_samples_host) against the CPU oracle, on float
bits and bytes, no tolerance anywhere.  Sample (sx, sy) of pixel (x, y) at factor s is pixel (x s + sx, y s + sy) of an
(s W) x (s H) target (RK:78-86), so the expected image is the oracle's float frame of that target, box-averaged in numpy float32
(resolve_np, tests/test_render_samples_cpu.py) -- and quantised by RK:98's rule for the bytes.  41 x 23 = 943 pixels are ragged
against the 256, 64, 28 and 16 pixels a workgroup covers at s = 1 .. 4."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import leafy_scene, random_sky, ref_fixture, spine_scene, tri_buffers, triangle_scene
from shade_common import F, bits, camera_rays, quantise, same
from test_render_samples_cpu import resolve_np

pytestmark = pytest.mark.gpu

W, H = 41, 23


def make_renderer(scene, bounces, sky=None, mat=None, w=W, h=H, **kw):
    r = rt.RendererRaytracing(w, h, scene, maxBounces=bounces, **kw).initialize(sky, mat)
    r.recalculateScene()
    return r


def check(img, flt, want_rgb, what=""):
    """(H, W, 4) uint8 and / or (H, W, 4) float32 against the resolved float frame want_rgb (H, W, 3)"""
    if flt is not None:
        assert flt.shape == want_rgb.shape[:2] + (4,) and flt.dtype == np.float32
        bad = int((bits(flt[:, :, 0:3]) != bits(want_rgb)).any(axis=-1).sum())
        assert bad == 0, "%s: %d of %d float pixels differ from the resolved oracle frame" % (what, bad, want_rgb.shape[0] * want_rgb.shape[1])
        assert np.all(bits(flt[:, :, 3]) == 0x3F800000), what               # word 3 is 1.0f
    if img is not None:
        assert img.shape == want_rgb.shape[:2] + (4,) and img.dtype == np.uint8
        bad = int((img[:, :, 0:3] != quantise(want_rgb)).any(axis=-1).sum())
        assert bad == 0, "%s: %d pixels differ from the quantised resolved oracle frame" % (what, bad)
        assert np.all(img[:, :, 3] == 255), what                            # the frame's own alpha byte


# ---- 1. spheres ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "textured"])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("n,bounces", [(37, 3), (1100, 3), (37, 0)])
def test_spheres(oracle, constant_sky, n, bounces, s, flat):
    """37 spheres are one staged chunk, 1,100 are two (staged in every search); bounces = 0 leaves the bounce loop unentered."""
    scene = rt.synthetic_scene(n, 11)
    sky = constant_sky if flat else random_sky(13)
    params = np.asarray(scene.pack_params(bounces), F)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    _, big, _ = oracle.render(params, sp, sky.faces, s * W, s * H, want_float=True)
    want = resolve_np(big, s)
    r = make_renderer(scene, bounces, sky)
    try:
        img, flt = r.render_samples(s, float_out=True)
        check(img, flt, want, "n=%d s=%d" % (n, s))
        if bounces:
            assert len(np.unique(img.reshape(-1, 4), axis=0)) > 20           # a picture, not a constant
    finally:
        r.close()


# ---- 2. triangles: every launch form, before the first frame and after one ---------------------------------------------------------
def tri_cases():
    def insts(k):                     # triangle_scene adds a floor to its k models
        return lambda: triangle_scene(seed=40 + k, n_models=k - 1)
    return {
        "ref": lambda: (ref_fixture()[0], rt.Material.white()),
        "spine24": lambda: (spine_scene(24), rt.Material.white()),
        "leafy3": lambda: (leafy_scene(3), rt.Material.white()),
        "inst3": insts(3), "inst13": insts(13), "inst17": insts(17),
    }


TRI = tri_cases()


@pytest.mark.parametrize("name,s", [(k, s) for k in TRI for s in (2, 3)] + [("inst3", 4)])
def test_triangles(oracle, name, s):
    """The cases of tests/test_shade_rays_gpu.py.  Before the first frame the context has no relinked pair records (staged
    instances with the node walk; the per-frame buffer versions for seventeen instances); a frame builds them where the scene fits."""
    scene, mat = TRI[name]()
    bounces = 4 if name == "ref" else 2
    sky = random_sky(14)
    params = np.asarray(scene.pack_params(bounces), F)
    _, big, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, s * W, s * H, want_float=True)
    want = resolve_np(big, s)
    r = make_renderer(scene, bounces, sky, mat)
    try:
        img, flt = r.render_samples(s, float_out=True)
        check(img, flt, want, "%s s=%d before the first frame" % (name, s))
        r.render()
        r.read_pixels()
        img, flt = r.render_samples(s, float_out=True)
        check(img, flt, want, "%s s=%d after a frame" % (name, s))
    finally:
        r.close()


# ---- 3. one sample per pixel is the renderer's own frame ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spheres", "inst3", "inst17"])
def test_one_sample_is_the_rendered_frame(kind):
    if kind == "spheres":
        scene, mat = rt.synthetic_scene(300, 11), None
    else:
        scene, mat = TRI[kind]()
    r = make_renderer(scene, 3, random_sky(15), mat)
    try:
        r.render()
        frame = r.read_pixels()
        assert np.array_equal(r.render_samples(1), frame)
    finally:
        r.close()


# ---- 4. the float output is the resolve of the shaded queries ----------------------------------------------------------------------
@pytest.mark.parametrize("kind,s", [("spheres", 3), ("inst3", 2)])
def test_float_output_is_the_resolve_of_shade_rays(kind, s):
    if kind == "spheres":
        scene, mat = rt.synthetic_scene(37, 11), None
    else:
        scene, mat = TRI[kind]()
    r = make_renderer(scene, 2, random_sky(16), mat)
    try:
        o, d = camera_rays(scene.pack_params(2), s * W, s * H)
        shaded = r.shade_rays(o, d, compose=True)[:, 0:3].reshape(s * H, s * W, 3)
        img, flt = r.render_samples(s, float_out=True)
        check(img, flt, resolve_np(shaded, s), kind)
    finally:
        r.close()


# ---- 5. the pose no frame has carried ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst", [3, 17])
def test_samples_see_the_pose_no_frame_has_carried(oracle, n_inst):
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    bounces, s = 2, 2
    sky = random_sky(17)
    r = make_renderer(scene, bounces, sky, mat)
    try:
        params = np.asarray(scene.pack_params(bounces), F)
        r.render()                                        # a frame carries the first pose
        _, old, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, s * W, s * H, want_float=True)
        scene.update(0.5)
        _, new, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, s * W, s * H, want_float=True)
        img, flt = r.render_samples(s, float_out=True)    # (no frame in between)
        check(img, flt, resolve_np(new, s), "%d instances" % n_inst)
        assert not same(old, new)                         # the poses differ where the camera looks
    finally:
        r.close()


# ---- 6. beside frames in flight ----------------------------------------------------------------------------------------------------
def test_samples_do_not_disturb_frames(oracle):
    import torch
    scene, mat = triangle_scene(seed=80, n_models=3)
    w, h, bounces, s = 160, 100, 2, 2
    r = make_renderer(scene, bounces, None, mat, w, h)
    try:
        sky = r.skyboxMaterial
        params = np.asarray(scene.pack_params(bounces), F)
        buf = tri_buffers(scene, mat)
        ref, _, ref_rays = oracle.render_tri(params, buf, sky.faces, w, h)
        _, big, _ = oracle.render_tri(params, buf, sky.faces, s * w, s * h, want_float=True)
        want = resolve_np(big, s)
        r.render()
        frames = r.host_frames(4)
        img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        flt = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")

        def batch(query):
            for _ in range(4):
                r.enqueue()
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    r.render_samples(s, out=(img, flt))
            r.enqueue()
            for k in range(4):
                r.read_pixels_async(k, frames[k])
            r.wait()
            r.read_pixels_wait()
            if query:
                side.synchronize()

        batch(False)
        batch(False)                      # (the library now knows the caller keeps frames in flight: the same form for both)
        s0 = r.stats()
        batch(True)
        s1 = r.stats()
        for f in frames + [r.read_pixels()]:
            assert np.array_equal(f, ref)
        assert s1["frames"] == s0["frames"] + 5 and s1["batch_frames"] == s0["batch_frames"]
        for k in ("rays", "kernel_id", "tri_form"):
            assert s1[k] == s0[k], k
        assert s1["rays"] == ref_rays
        check(img.cpu().numpy(), flt.cpu().numpy(), want, "beside frames in flight")
        before = r.stats()
        again = r.render_samples(s)
        after = r.stats()
        for k in before:
            assert after[k] == before[k], k                          # the call changes no statistic, field by field
        assert np.array_equal(again, img.cpu().numpy())
        # heatmap, strict mode, the node-walk variant: the same frame
        for setup in (r.showHeatmap, lambda: (r.showRaytracer(), r.set_mode(True)), lambda: r.set_variant(6)):
            setup()
            assert np.array_equal(r.render_samples(s), again)
    finally:
        r.close()


# ---- 7. a partitioned context still gives the whole frame --------------------------------------------------------------------------
def test_a_partitioned_context_returns_the_whole_frame(oracle):
    scene = rt.synthetic_scene(37, 11)
    sky = random_sky(18)
    s = 2
    params = np.asarray(scene.pack_params(3), F)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    _, big, _ = oracle.render(params, sp, sky.faces, s * W, s * H, want_float=True)
    r = make_renderer(scene, 3, sky, rank=1, world=2)                # rt_set_partition(1, 2)
    try:
        img, flt = r.render_samples(s, float_out=True)
        check(img, flt, resolve_np(big, s), "rank 1 of 2")
    finally:
        r.close()


# ---- 8. paths and arguments --------------------------------------------------------------------------------------------------------
def test_device_host_and_numpy_paths_agree_and_arguments_are_checked():
    import torch
    scene, mat = triangle_scene(seed=90, n_models=5)
    s = 3
    r = make_renderer(scene, 2, random_sky(19), mat)
    lib = r._lib
    vp = ctypes.c_void_p
    try:
        img, flt = r.render_samples(s, float_out=True)
        # the host form, both outputs and each alone
        h8, hf = np.full((H, W, 4), 7, np.uint8), np.full((H, W, 4), 7, F)
        abi.check(lib.rt_render_samples_host(r._ctx, s, h8.ctypes.data, h8.nbytes, hf.ctypes.data, hf.nbytes), r._ctx)
        assert np.array_equal(h8, img) and same(hf, flt)
        h8[:], hf[:] = 7, 7
        abi.check(lib.rt_render_samples_host(r._ctx, s, h8.ctypes.data, h8.nbytes, None, 0), r._ctx)
        abi.check(lib.rt_render_samples_host(r._ctx, s, None, 0, hf.ctypes.data, hf.nbytes), r._ctx)
        assert np.array_equal(h8, img) and same(hf, flt)
        assert np.array_equal(r.render_samples(s), img)
        # the device form on a side stream and on the current one, both outputs and each alone
        d8 = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda:0")
        df = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = r.render_samples(s, out=(d8, df))
        side.synchronize()
        assert out[0] is d8 and out[1] is df
        assert np.array_equal(d8.cpu().numpy(), img) and same(df.cpu().numpy(), flt)
        d8.fill_(7)
        df.fill_(7.0)
        assert r.render_samples(s, out=d8) is d8 and r.render_samples(s, out=df) is df
        torch.cuda.synchronize()
        assert np.array_equal(d8.cpu().numpy(), img) and same(df.cpu().numpy(), flt)
        # s, outputs, alignment, capacities
        n8, nf = W * H * 4, W * H * 16
        for bad in (0, 5):
            assert lib.rt_render_samples(r._ctx, bad, vp(d8.data_ptr()), n8, vp(df.data_ptr()), nf, None) == abi.RT_ERR_INVALID_ARG
            assert lib.rt_render_samples_host(r._ctx, bad, h8.ctypes.data, n8, hf.ctypes.data, nf) == abi.RT_ERR_INVALID_ARG
            assert b"RT355_MAX_SUPERSAMPLE" in lib.rt_last_error(r._ctx)
        assert lib.rt_render_samples(r._ctx, s, None, n8, None, nf, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_render_samples_host(r._ctx, s, None, n8, None, nf) == abi.RT_ERR_INVALID_ARG
        assert b"NULL" in lib.rt_last_error(r._ctx)
        assert lib.rt_render_samples(r._ctx, s, None, 0, vp(df.data_ptr() + 4), nf, None) == abi.RT_ERR_INVALID_ARG
        assert b"aligned" in lib.rt_last_error(r._ctx)
        assert lib.rt_render_samples(r._ctx, s, vp(d8.data_ptr()), n8 - 1, None, 0, None) == abi.RT_ERR_CAPACITY
        assert lib.rt_render_samples(r._ctx, s, vp(d8.data_ptr()), n8, vp(df.data_ptr()), nf - 1, None) == abi.RT_ERR_CAPACITY
        assert lib.rt_render_samples_host(r._ctx, s, h8.ctypes.data, n8 - 1, hf.ctypes.data, nf) == abi.RT_ERR_CAPACITY
        assert lib.rt_render_samples_host(r._ctx, s, None, 0, hf.ctypes.data, nf - 1) == abi.RT_ERR_CAPACITY
        # (the capacity of a NULL output is not looked at)
        assert lib.rt_render_samples_host(r._ctx, s, h8.ctypes.data, n8, None, 0) == abi.RT_OK
        torch.cuda.synchronize()
        assert np.array_equal(d8.cpu().numpy(), img) and same(df.cpu().numpy(), flt)      # the refused calls wrote nothing
    finally:
        r.close()
    # a context without rt_resize: RT_ERR_STATE, before the (short) capacity is looked at; then without a scene, without parameters
    fp = ctypes.POINTER(ctypes.c_float)
    scene = rt.synthetic_scene(3, 1)
    ctx = ctypes.c_void_p()
    abi.check(lib.rt_create(0, ctypes.byref(ctx)))
    try:
        h8 = np.zeros((16, 16, 4), np.uint8)
        assert lib.rt_render_samples_host(ctx, 2, h8.ctypes.data, 1, None, 0) == abi.RT_ERR_STATE
        assert b"rt_resize" in lib.rt_last_error(ctx)
        abi.check(lib.rt_resize(ctx, 16, 16), ctx)
        assert lib.rt_render_samples_host(ctx, 2, h8.ctypes.data, 1, None, 0) == abi.RT_ERR_STATE
        assert b"no scene" in lib.rt_last_error(ctx)
        sp = np.ascontiguousarray(scene.pack_spheres(), dtype=F)
        abi.check(lib.rt_write_spheres(ctx, sp.ctypes.data_as(fp), sp.shape[0]), ctx)
        assert lib.rt_render_samples_host(ctx, 2, h8.ctypes.data, 1, None, 0) == abi.RT_ERR_STATE
        assert b"rt_write_params" in lib.rt_last_error(ctx)
        p = scene.pack_params(2)
        abi.check(lib.rt_write_params(ctx, p.ctypes.data_as(fp)), ctx)
        assert lib.rt_render_samples_host(ctx, 2, h8.ctypes.data, 1, None, 0) == abi.RT_ERR_STATE
        assert b"cube map" in lib.rt_last_error(ctx)
    finally:
        lib.rt_destroy(ctx)
