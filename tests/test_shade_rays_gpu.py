"""Shaded ray queries on the MI355X (include/rt355.h: rt_shade_rays, rt_shade_rays_host, RT_SHADE_COMPOSE) against the CPU oracle,
on float bits, no tolerance anywhere: sphere scenes against oracle.ray_color, ray by ray; composed camera rays against the oracle's
float frame and, quantised, against the bytes of the renderer's own frame, spheres and triangles; triangle rays from arbitrary
origins against one-pixel oracle frames (the method: tests/test_shade_rays_cpu.py); the pose no frame has carried; queries beside
frames in flight; the three paths against each other and the argument checks that need a context."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import leafy_scene, random_sky, ref_fixture, spine_scene, tri_buffers, triangle_scene
from shade_common import (F, OracleRays, axis_rays, bits, camera_rays, compose_np, pack, quantise, random_rays, same, settled_unit,
                          sphere_box)

pytestmark = pytest.mark.gpu


def mismatches(got, want):
    return int((bits(got) != bits(want)).any(axis=-1).sum())


def make_renderer(scene, bounces, sky=None, mat=None, W=96, H=64):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=bounces).initialize(sky, mat)
    r.recalculateScene()
    return r


# ---- 1. spheres against oracle.ray_color ---------------------------------------------------------------------------------------
def sphere_scene_with_duplicates():
    scene = rt.synthetic_scene(24, 5)
    scene.spheres = list(scene.spheres) + list(scene.spheres)      # equal t for every pair: the lower index wins
    return scene


_SPHERE_RAYS = {}


def sphere_case(n):
    """scene, records, rays: the 96 x 64 camera rays, 2,000 incoherent rays of any length, 600 along the axes"""
    if n not in _SPHERE_RAYS:
        scene = sphere_scene_with_duplicates() if n == "dup" else rt.synthetic_scene(n, 11)
        sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
        lo, hi = sphere_box(sp)
        sets = [camera_rays(scene.pack_params(1), 96, 64), random_rays(lo, hi, 2000, 3), axis_rays(lo, hi, 4)]
        _SPHERE_RAYS[n] = (scene, sp, np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
    return _SPHERE_RAYS[n]


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "textured"])
@pytest.mark.parametrize("bounces", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 37, 1100, "dup"])
def test_spheres_against_ray_color(oracle, constant_sky, n, bounces, flat):
    """1,100 spheres are more than one staged chunk of 1,024; in the duplicated scene every hit has two candidates."""
    scene, sp, o, d = sphere_case(n)
    sky = constant_sky if flat else random_sky(9)
    r = make_renderer(scene, bounces, sky)
    try:
        got = r.shade_rays(o, d)
        assert got.shape == (o.shape[0], 4) and got.dtype == np.float32
        want, cnt = OracleRays(oracle, scene.pack_params(bounces), sp, sky.faces).ray_color(o, d)
        assert same(got, want), "%d of %d rays differ from oracle.ray_color" % (mismatches(got, want), o.shape[0])
        if bounces == 0:
            assert np.all(got == np.array([1, 1, 1, 0], F))
        else:
            assert (want[:, 3] != 0).sum() >= 100                       # paths that hit something
            assert np.all(cnt[want[:, 3] == 0] == 1)                     # a first ray that misses: one traversal, dist 0
        if bounces == 3:
            assert ((cnt % 2 == 1) & (cnt >= 3)).sum() >= 100          # paths that end in the sky after at least one bounce
    finally:
        r.close()


def test_an_empty_sphere_scene_gives_the_sky(oracle):
    """rt_write_spheres(n = 0) counts as a scene written (the existing queries report a miss for every ray then): every path
    escapes at once, along the direction as given."""
    scene = rt.synthetic_scene(0, 11)
    sky = random_sky(10)
    r = make_renderer(scene, 3, sky)
    try:
        o, d = random_rays([-5, -5, -5], [5, 5, 5], 700, 12)
        got = r.shade_rays(o, d)
        orc = OracleRays(oracle, scene.pack_params(3), np.zeros((0, 8), F), sky.faces)
        want, _ = orc.ray_color(o, d)
        assert same(got, want)
        assert same(got[:, 0:3], F(scene.pack_params(3)[20]) * orc.sky(d)) and np.all(got[:, 3] == 0)
        assert r.trace_rays(o, d)["prim"].max() == -1
    finally:
        r.close()


# ---- 2. dead lanes and the ragged tail ------------------------------------------------------------------------------------------
def test_finished_lanes_and_lanes_past_the_end_meet_every_barrier(oracle):
    """1,100 spheres (two chunks, staged in every search) and 257 rays: the 256 of the first workgroup leave the scene at once, the
    one ray of the second workgroup -- 255 lanes past n beside it -- bounces four times."""
    scene, sp, o_all, d_all = sphere_case(1100)
    sky = random_sky(9)
    bounces = 4
    orc = OracleRays(oracle, scene.pack_params(bounces), sp, sky.faces)
    lo, hi = sphere_box(sp)
    away = np.tile(np.array([[0.3, 1.0, 0.2]], F), (256, 1)) * np.linspace(0.5, 3.0, 256, dtype=F)[:, None]
    o_away = np.tile(np.array([[0.0, float(hi[1]) + 1.0, 0.0]], F), (256, 1))
    _, cnt = orc.ray_color(o_all, d_all)
    long_paths = np.nonzero(cnt == 2 * bounces)[0]
    assert long_paths.size > 0
    o = np.concatenate([o_away, o_all[long_paths[:1]]])
    d = np.concatenate([away, d_all[long_paths[:1]]])
    want, cnt = orc.ray_color(o, d)
    assert np.all(cnt[:256] == 1) and cnt[256] == 2 * bounces
    r = make_renderer(scene, bounces, sky)
    try:
        got = r.shade_rays(o, d)
        assert same(got, want), "%d of 257 rays differ" % mismatches(got, want)
    finally:
        r.close()


# ---- 3. compose equals the frame -------------------------------------------------------------------------------------------------
def check_compose_against_frame(r, params, W, H, want_rgb, orc_sky, before_frame=False):
    """Every camera ray shaded with and without RT_SHADE_COMPOSE, against the oracle's float frame `want_rgb` (H, W, 3) and the
    renderer's own next frame."""
    o, d = camera_rays(params, W, H)
    if before_frame:                                 # (triangles: no frame yet -- the forms without the relinked pair records)
        early = r.shade_rays(o, d, compose=True)
        assert same(early[:, 0:3], want_rgb.reshape(-1, 3)), "%d pixels differ before the first frame" % mismatches(
            early[:, 0:3], want_rgb.reshape(-1, 3))
    r.render()
    frame = r.read_pixels()
    plain = r.shade_rays(o, d)
    comp = r.shade_rays(o, d, compose=True)
    assert same(comp[:, 0:3], want_rgb.reshape(-1, 3)), "%d of %d pixels differ from the oracle's float frame" % (
        mismatches(comp[:, 0:3], want_rgb.reshape(-1, 3)), W * H)
    assert np.array_equal(quantise(comp[:, 0:3]).reshape(H, W, 3), frame[:, :, 0:3])
    assert same(comp[:, 3], plain[:, 3])
    assert same(comp[:, 0:3], compose_np(plain, orc_sky(d), params[20]))
    return plain


@pytest.mark.parametrize("n,flat", [(37, False), (300, False), (37, True)])
def test_compose_equals_the_frame_spheres(oracle, constant_sky, n, flat):
    scene = rt.synthetic_scene(n, 11)
    sky = constant_sky if flat else random_sky(13)
    W, H, bounces = 96, 64, 3
    params = np.asarray(scene.pack_params(bounces), F)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    ref8, ref_rgb, _ = oracle.render(params, sp, sky.faces, W, H, want_float=True)
    r = make_renderer(scene, bounces, sky, None, W, H)
    try:
        plain = check_compose_against_frame(r, params, W, H, ref_rgb, OracleRays(oracle, params, sp, sky.faces).sky)
        assert np.array_equal(r.read_pixels(), ref8)
        assert (plain[:, 3] > 0).sum() > 100 and (plain[:, 3] == 0).sum() > 100
    finally:
        r.close()


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


@pytest.mark.parametrize("name,flat", [(k, False) for k in TRI] + [("inst3", True)])
def test_compose_equals_the_frame_triangles(oracle, constant_sky, name, flat):
    """The cases of tests/test_ray_query_gpu.py that between them reach every launch form (rt_shade.hip: the selection of
    rt_query_form.h).  Before the first frame the context has no relinked pair records: staged instances with the node walk, and
    the per-frame buffer versions for seventeen instances; a frame builds the records where the scene fits them, and the same
    rays then go through the pair forms, with 16-bit entries where every meta fits them."""
    scene, mat = TRI[name]()
    W, H, bounces = (168, 106, 4) if name == "ref" else (160, 100, 2)
    sky = constant_sky if flat else random_sky(14)
    params = np.asarray(scene.pack_params(bounces), F)
    _, ref_rgb, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, W, H, want_float=True)
    r = make_renderer(scene, bounces, sky, mat, W, H)
    try:
        orc = OracleRays(oracle, params, np.zeros((0, 8), F), sky.faces)
        plain = check_compose_against_frame(r, params, W, H, ref_rgb, orc.sky, before_frame=True)
        assert (plain[:, 3] > 0).sum() > 100
    finally:
        r.close()


# ---- 4. triangles, arbitrary origins ----------------------------------------------------------------------------------------------
def scene_box(buf, params):
    """The top-level root's box, within 20 of the camera (the reference's floor spans millions)."""
    root, cam = buf["nodes"][0], params[0:3]
    return np.maximum(root[0:3], cam - 20.0), np.minimum(root[4:7], cam + 20.0)


def one_pixel_frames(oracle, params, buf, faces, o, d):
    """The oracle's float frame of one pixel per ray: the camera at the ray's origin, looking along its (settled) direction"""
    out = np.zeros((o.shape[0], 3), F)
    for i in range(o.shape[0]):
        p = np.array(params, F)
        p[0:3], p[4:7] = o[i], d[i]
        p[8:11] = 0.0
        p[12:15] = 0.0
        out[i] = oracle.render_tri(p, buf, faces, 1, 1, want_float=True, threads=1)[1][0, 0]
    return out


@pytest.mark.parametrize("name", ["inst3", "inst17"])
def test_triangles_from_arbitrary_origins(oracle, name):
    scene, mat = TRI[name]()
    bounces = 3
    sky = random_sky(15)
    params = np.asarray(scene.pack_params(bounces), F)
    buf = tri_buffers(scene, mat)
    lo, hi = scene_box(buf, params)
    o, d = random_rays(lo, hi, 220, 16)
    o[:, 1] = np.abs(o[:, 1]) + F(0.25)                          # above the floor
    # (few of those meet the models: eighty more, from the same kind of origin towards where triangle_scene puts them)
    rng = np.random.default_rng(19)
    o2 = random_rays(lo, hi, 80, 20)[0]
    o2[:, 1] = np.abs(o2[:, 1]) + F(0.25)
    aim = np.stack([rng.uniform(-4, 4, 80), rng.uniform(0, 1.5, 80), rng.uniform(-9, -3, 80)], axis=1)
    o, d = np.concatenate([o, o2]), np.concatenate([d, (aim - o2).astype(F)])
    d, ok = settled_unit(d)                                      # (a 1x1 frame normalises once more: tests/test_shade_rays_cpu.py)
    o, d = o[ok], d[ok]
    assert o.shape[0] >= 250 and np.all(d != 0)
    want = one_pixel_frames(oracle, params, buf, sky.faces, o, d)
    r = make_renderer(scene, bounces, sky, mat, 160, 100)
    try:
        got = r.shade_rays(o, d, compose=True)
        assert same(got[:, 0:3], want), "%d of %d rays differ from their one-pixel frames" % (mismatches(got[:, 0:3], want), o.shape[0])
        assert (got[:, 3] > 0).sum() >= 20                       # rays that hit geometry
        t = r.trace_rays(o, d)["t"]
        assert same(got[:, 3], np.where(t < 0, F(0.0), t))       # dist is the nearest hit's t
    finally:
        r.close()


# ---- 5. the pose no frame has carried --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst", [3, 17])
def test_shade_sees_the_pose_no_frame_has_carried(oracle, n_inst):
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    W, H, bounces = 160, 100, 2
    sky = random_sky(17)
    r = make_renderer(scene, bounces, sky, mat, W, H)
    try:
        params = np.asarray(scene.pack_params(bounces), F)
        r.render()                                        # a frame carries the first pose
        _, old_rgb, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, W, H, want_float=True)
        scene.update(0.5)
        _, new_rgb, _ = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, W, H, want_float=True)
        o, d = camera_rays(params, W, H)
        got = r.shade_rays(o, d, compose=True)
        assert same(got[:, 0:3], new_rgb.reshape(-1, 3)), "%d pixels differ from the new pose's frame" % mismatches(
            got[:, 0:3], new_rgb.reshape(-1, 3))
        assert not same(old_rgb, new_rgb)                 # the poses differ where the rays look
    finally:
        r.close()


# ---- 6. beside frames in flight ---------------------------------------------------------------------------------------------------
def test_shade_queries_do_not_disturb_frames(oracle):
    import torch
    scene, mat = triangle_scene(seed=80, n_models=3)
    W, H, bounces = 160, 100, 2
    r = make_renderer(scene, bounces, None, mat, W, H)
    try:
        sky = r.skyboxMaterial
        params = np.asarray(scene.pack_params(bounces), F)
        ref, ref_rgb, ref_rays = oracle.render_tri(params, tri_buffers(scene, mat), sky.faces, W, H, want_float=True)
        r.render()
        o, d = camera_rays(params, W, H)
        dev = torch.from_numpy(pack(o, d)).to("cuda:0")
        frames = r.host_frames(4)

        def batch(query):
            for _ in range(4):
                r.enqueue()
            out = None
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    out = r.shade_rays(dev, compose=True)
            r.enqueue()
            for k in range(4):
                r.read_pixels_async(k, frames[k])
            r.wait()
            r.read_pixels_wait()
            if query:
                side.synchronize()
            return out

        batch(False)
        batch(False)                      # (the library now knows the caller keeps frames in flight: the same form for both)
        s0 = r.stats()
        out = batch(True)
        s1 = r.stats()
        for f in frames + [r.read_pixels()]:
            assert np.array_equal(f, ref)
        assert s1["frames"] == s0["frames"] + 5 and s1["batch_frames"] == s0["batch_frames"]
        for k in ("rays", "kernel_id", "tri_form"):
            assert s1[k] == s0[k], k
        assert s1["rays"] == ref_rays
        assert same(out.cpu().numpy()[:, 0:3], ref_rgb.reshape(-1, 3))
        before = r.stats()
        again = r.shade_rays(o, d, compose=True)
        after = r.stats()
        for k in before:
            assert after[k] == before[k], k                          # a query changes no statistic, field by field
        assert same(again[:, 0:3], ref_rgb.reshape(-1, 3))
        # heatmap, strict mode, the node-walk variant: the same answers
        for setup in (r.showHeatmap, lambda: (r.showRaytracer(), r.set_mode(True)), lambda: r.set_variant(6)):
            setup()
            assert same(r.shade_rays(dev, compose=True).cpu().numpy(), again)
    finally:
        r.close()


# ---- 7. paths and arguments -------------------------------------------------------------------------------------------------------
def test_device_out_and_host_paths_agree_and_arguments_are_checked():
    import torch
    scene, mat = triangle_scene(seed=90, n_models=5)
    W, H = 150, 90
    r = make_renderer(scene, 2, random_sky(18), mat, W, H)
    lib = r._lib
    try:
        o, d = camera_rays(scene.pack_params(2), W, H)
        o, d = o[::3], d[::3]
        rays = pack(o, d)
        rays[:, 3], rays[:, 7] = 123.0, -4.0                        # words 3 and 7 are ignored
        host = r.shade_rays(o, d)
        raw = np.zeros(rays.shape[0], dtype=abi.SHADE_DTYPE)
        abi.check(lib.rt_shade_rays_host(r._ctx, rays.ctypes.data, rays.shape[0], 0, raw.ctypes.data), r._ctx)
        assert same(raw.view(F).reshape(-1, 4), host)
        dev = torch.from_numpy(rays).to("cuda:0")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = r.shade_rays(dev)
        side.synchronize()
        assert on_side.shape == (rays.shape[0], 4) and same(on_side.cpu().numpy(), host)
        out = torch.full((rays.shape[0], 4), 7.0, device="cuda:0")
        assert r.shade_rays(dev, out=out) is out
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), host)
        for flags in (0, abi.RT_SHADE_COMPOSE):
            comp = r.shade_rays(dev, compose=bool(flags))
            torch.cuda.synchronize()
            assert same(comp.cpu().numpy(), r.shade_rays(o, d, compose=bool(flags)))
        # misaligned device rays, unknown flags, NULL pointers, n == 0
        vp = ctypes.c_void_p
        assert lib.rt_shade_rays(r._ctx, vp(dev.data_ptr() + 4), 8, 0, vp(out.data_ptr()), None) == abi.RT_ERR_INVALID_ARG
        assert b"aligned" in lib.rt_last_error(r._ctx)
        assert lib.rt_shade_rays(r._ctx, vp(dev.data_ptr()), 8, 0, vp(out.data_ptr() + 8), None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shade_rays(r._ctx, vp(dev.data_ptr()), 8, 2, vp(out.data_ptr()), None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shade_rays_host(r._ctx, rays.ctypes.data, 8, 0x80000000, raw.ctypes.data) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shade_rays_host(r._ctx, None, 4, 0, raw.ctypes.data) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shade_rays_host(r._ctx, rays.ctypes.data, 4, 0, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shade_rays_host(r._ctx, None, 0, 0, None) == abi.RT_OK
        # the messages whole, and the order when two arguments are wrong: flags, pointers, alignment
        err = lambda: lib.rt_last_error(r._ctx)
        for off_rays, off_out in ((4, 0), (0, 8)):
            assert lib.rt_shade_rays(r._ctx, vp(dev.data_ptr() + off_rays), 8, 0, vp(out.data_ptr() + off_out), None) == abi.RT_ERR_INVALID_ARG
            assert err() == b"rt_shade_rays: rays and out must be 16-byte aligned"
        for fn, name, tail in ((lib.rt_shade_rays, b"rt_shade_rays", (None,)), (lib.rt_shade_rays_host, b"rt_shade_rays_host", ())):
            assert fn(r._ctx, None, 4, 2, None, *tail) == abi.RT_ERR_INVALID_ARG and err() == name + b": unknown flag bits 0x2"
            assert fn(r._ctx, None, 4, 0, vp(out.data_ptr() + 8), *tail) == abi.RT_ERR_INVALID_ARG and err() == name + b": NULL argument"
        assert lib.rt_shade_rays(r._ctx, None, 0, abi.RT_SHADE_COMPOSE, None, None) == abi.RT_OK
    finally:
        r.close()
    # a context with a scene and a sky but no rt_write_params, and one with parameters but no scene
    fp = ctypes.POINTER(ctypes.c_float)
    rays = np.zeros((1, 8), F)
    rays[0, 6] = -1.0
    res = np.zeros(1, dtype=abi.SHADE_DTYPE)
    scene = rt.synthetic_scene(3, 1)
    for write_params in (False, True):
        bare = rt.RendererRaytracing(16, 16, scene).initialize()
        try:
            if write_params:
                p = scene.pack_params(2)
                abi.check(lib.rt_write_params(bare._ctx, p.ctypes.data_as(fp)), bare._ctx)
            else:
                s = np.ascontiguousarray(scene.pack_spheres(), dtype=F)
                abi.check(lib.rt_write_spheres(bare._ctx, s.ctypes.data_as(fp), s.shape[0]), bare._ctx)
            assert lib.rt_shade_rays_host(bare._ctx, rays.ctypes.data, 1, 0, res.ctypes.data) == abi.RT_ERR_STATE
            assert (b"rt_write_params" if not write_params else b"no scene") in lib.rt_last_error(bare._ctx)
        finally:
            bare.close()
