"""Ambient-occlusion frames on the MI355X (include/rt355.h: rt_render_ao, rt_render_ao_host): the count plane of a 41 x 23 frame --
ragged against the 8 x 8 tile of a wave and the 32 x 8 pixels of a workgroup -- against the composition it replaces (pick(), the
float32 restatement of tests/ao_common.py, occluded(), a sum), against the CPU oracle alone and against the numpy sphere loop.
Counts compare as integers and `ao` on float bits: no tolerance anywhere and no pixel left out."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from ao_common import ao_of, ao_rays, counts_from
from helpers import tri_buffers, triangle_scene
from query_common import F, bits, camera_rays, trace_spheres
from refit_common import deform, mesh_ranges, view_scene
from test_gbuffer_cpu import spheres_with_a_view
from test_gbuffer_gpu import RECTS, TRI_HITS
from test_render_ao_cpu import CPU_CASES, CPU_K, cpu_counts
from test_render_samples_gpu import TRI

pytestmark = pytest.mark.gpu

W, H = 41, 23
N = W * H
KS = (1, 5, 64)
NAMES = ("count", "ao")
TMIN = 0.001

# Per triangle scene the radius of the rays, whether its directions point below the horizon (see case_dirs), and per k what the
# composition finds among the pixels that hit: (count == 0, 0 < count < k, count == k).  ref and inst*: the CPU oracle's figures
# (tests/test_render_ao_cpu.py shows them for k = 5 without a device); spine24 and leafy3: pick() and occluded() on the device.
TRI_CASES = {
    "ref":     (1.0, False, {1: (533, 0, 33), 5: (470, 93, 3), 64: (396, 170, 0)}),
    "spine24": (4.0, True,  {1: (274, 0, 1), 5: (271, 4, 0), 64: (270, 5, 0)}),
    "leafy3":  (2.0, True,  {1: (250, 0, 117), 5: (225, 142, 0), 64: (208, 159, 0)}),
    "inst3":   (2.0, False, {1: (558, 0, 5), 5: (549, 14, 0), 64: (536, 27, 0)}),
    "inst13":  (1.0, False, {1: (542, 0, 30), 5: (483, 86, 3), 64: (438, 134, 0)}),
    "inst17":  (1.0, False, {1: (543, 0, 33), 5: (496, 79, 1), 64: (462, 114, 0)}),
}
# The sphere cases at radius 2: (hits of the 943 primary rays, per k the same three figures), by the numpy loop alone
SPHERE_RADIUS = 2.0
SPHERE_CASES = {
    "one chunk":   (707, {1: (686, 0, 21), 5: (630, 77, 0), 64: (554, 153, 0)}),
    "two chunks":  (778, {1: (645, 0, 133), 5: (407, 368, 3), 64: (284, 494, 0)}),
    "with a view": (217, {1: (205, 0, 12), 5: (183, 34, 0), 64: (120, 97, 0)}),
}


def case_dirs(k, down=False):
    """ao_directions(k); down: every other one, the first included, turned to point steeply below the horizon and not of unit length
    (nothing normalises directions).  The hand-made scenes are stacks of triangles that all face +z: a ray into the upper
    hemisphere meets back faces alone there, and is never occluded."""
    d = rt.ao_directions(k)
    if down:
        d[0::2] *= F(-1.0)
        d[0::2, 0:2] *= F(-0.25)
    return d


def make_renderer(scene, mat=None, **kw):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=2, **kw).initialize(None, mat)
    r.recalculateScene()
    return r


def composition(r, scene, dirs, radius, tmin=TMIN):
    """The route the call replaces, on the same renderer: pick() of every pixel, the restated rays, occluded(), a sum per pixel.
    -> the (H, W) uint8 counts, the flat pick-style hits, and the rays (m, k, 8) of the pixels that hit."""
    ys, xs = np.mgrid[0:H, 0:W]
    p = r.pick(xs.reshape(-1), ys.reshape(-1))
    o, d = camera_rays(scene, W, H)
    hit, rays = ao_rays(p, o, d, dirs, tmin, radius)
    flat = rays.reshape(-1, 8)
    occ = r.occluded(flat[:, 0:3], flat[:, 4:7], flat[:, 3], flat[:, 7])
    return counts_from(N, hit, occ, dirs.shape[0]).reshape(H, W), p, rays


def kinds_of(count, p, k):
    c = count.reshape(-1)[p["prim"] >= 0]
    return int((c == 0).sum()), int(((c > 0) & (c < k)).sum()), int((c == k).sum())


def check_planes(g, want, p, k, what=""):
    """Both planes of a call against the expected counts; the misses are exactly pick's"""
    assert g["count"].dtype == np.uint8 and g["count"].shape == (H, W) and g["ao"].dtype == np.float32 and g["ao"].shape == (H, W)
    bad = int((g["count"] != want).sum())
    assert bad == 0, "%s: %d of %d counts differ from the composition" % (what, bad, N)
    assert np.array_equal(bits(g["ao"]), bits(ao_of(want, k))), what
    miss = (p["prim"] < 0).reshape(H, W)
    assert np.all(g["count"][miss] == 0) and np.all(bits(g["ao"][miss]) == 0x3F800000), what


def same_planes(a, b, names=NAMES):
    return all(a[n].dtype == b[n].dtype and np.array_equal(np.ascontiguousarray(a[n]).view(np.uint8), np.ascontiguousarray(b[n]).view(np.uint8))
               for n in names)


def crop(g, rect):
    if rect is None:
        return g
    x0, y0, w, h = rect
    return {n: a[y0:y0 + h, x0:x0 + w] for n, a in g.items()}


CANARY = 64


def device_planes(w, h, names=NAMES):
    """Per name a flat tensor of w h pixels and CANARY elements more, every element 7, and the (h, w) view of its head."""
    import torch
    flat = {n: torch.full((w * h + CANARY,), 7, dtype=torch.uint8 if n == "count" else torch.float32, device="cuda:0") for n in names}
    return flat, {n: t[:w * h].view(h, w) for n, t in flat.items()}


def canaries_intact(flat):
    return all(bool((t[t.numel() - CANARY:] == 7).all()) for t in flat.values())


def to_numpy(view):
    return {n: t.cpu().numpy() for n, t in view.items()}


# ---- 1, 3. triangles against the composition: every launch form, before the first frame and after one -------------------------------------
@pytest.mark.parametrize("name", list(TRI))
def test_triangles_against_the_composition(name):
    scene, mat = TRI[name]()
    radius, down, kinds = TRI_CASES[name]
    r = make_renderer(scene, mat)
    try:
        for when in ("before the first frame", "after a frame"):
            for k in KS:
                dirs = case_dirs(k, down)
                want, p, _ = composition(r, scene, dirs, radius)
                got = kinds_of(want, p, k)
                print(name, when, "k =", k, "hits", int((p["prim"] >= 0).sum()), "kinds", got)
                # the input: pixels without an occluded ray, pixels with some (for k > 1: and not all), and misses
                assert int((p["prim"] >= 0).sum()) == TRI_HITS[name] < N
                assert got == kinds[k], (name, when, k, got)
                assert got[0] > 0 and (got[1] > 0 if k > 1 else got[2] > 0)
                check_planes(r.render_ao(dirs, radius=radius, planes=NAMES), want, p, k, "%s %s k = %d" % (name, when, k))
            r.render()
            r.read_pixels()                               # (builds the relinked pair records where the scene fits them)
    finally:
        r.close()


# ---- 2. against a route without the device's rt_occluded, rt_pick or anything else of it ---------------------------------------------
@pytest.mark.parametrize("name", list(CPU_CASES))
def test_triangles_against_the_cpu_alone(oracle, name):
    """The primary hits by the float32 brute force checked against the oracle's walk, the rays by the restatement, their occlusion by
    the oracle's walk (tests/test_render_ao_cpu.py: cpu_counts)."""
    want, h = cpu_counts(oracle, name)
    scene, mat = TRI[name]()
    r = make_renderer(scene, mat)
    try:
        g = r.render_ao(k=CPU_K, radius=CPU_CASES[name][0], planes=NAMES)           # (the default directions: ao_directions(k))
        check_planes(g, want.reshape(H, W), h, CPU_K, name)
        assert kinds_of(want, h, CPU_K) == CPU_CASES[name][1] == TRI_CASES[name][2][CPU_K]
    finally:
        r.close()


# ---- 4. spheres: the numpy loop and occluded() --------------------------------------------------------------------------------------
def sphere_scenes():
    return {"one chunk": lambda: rt.synthetic_scene(37, 11), "two chunks": lambda: rt.synthetic_scene(1100, 11),
            "with a view": lambda: spheres_with_a_view()[0]}


@pytest.mark.parametrize("case", list(SPHERE_CASES))
def test_spheres_against_the_restatement(case):
    scene = sphere_scenes()[case]()
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    hits, kinds = SPHERE_CASES[case]
    r = make_renderer(scene)
    try:
        for k in KS:
            dirs = case_dirs(k)
            want, p, rays = composition(r, scene, dirs, SPHERE_RADIUS)
            flat = rays.reshape(-1, 8)
            with np.errstate(all="ignore"):
                occ = trace_spheres(sp, flat[:, 0:3], flat[:, 4:7], flat[:, 3], flat[:, 7])[1] >= 0
            by_numpy = counts_from(N, np.nonzero(p["prim"] >= 0)[0], occ, k).reshape(H, W)
            assert np.array_equal(by_numpy, want), "occluded() and the numpy loop differ"
            got = kinds_of(want, p, k)
            print(case, "k =", k, "kinds", got)
            assert int((p["prim"] >= 0).sum()) == hits < N and got == kinds[k], (case, k, got)
            assert got[0] > 0 and (got[1] > 0 if k > 1 else got[2] > 0)
            check_planes(r.render_ao(dirs, radius=SPHERE_RADIUS, planes=NAMES), want, p, k, "%s k = %d" % (case, k))
    finally:
        r.close()


# ---- 5, 6. limits, rectangles, plane subsets, the device form ------------------------------------------------------------------------------
SUBJECT_K = 5


@pytest.fixture(scope="module", params=["inst3", "spheres"])
def subject(request):
    """One triangle and one sphere scene: the renderer, its scene, the radius, and both whole-frame planes of the host form at
    SUBJECT_K rays (never written to) -- equal to the composition, with pixels of every kind."""
    if request.param == "spheres":
        scene, mat, radius = sphere_scenes()["one chunk"](), None, SPHERE_RADIUS
    else:
        (scene, mat), radius = TRI[request.param](), TRI_CASES[request.param][0]
    r = make_renderer(scene, mat)
    whole = r.render_ao(k=SUBJECT_K, radius=radius, planes=NAMES)
    want, p, _ = composition(r, scene, rt.ao_directions(SUBJECT_K), radius)
    check_planes(whole, want, p, SUBJECT_K, request.param)
    kinds = kinds_of(want, p, SUBJECT_K)
    assert kinds[0] > 0 and kinds[1] > 0 and 0 < int((p["prim"] >= 0).sum()) < N
    for a in whole.values():
        a.setflags(write=False)
    yield r, scene, radius, whole
    r.close()


def test_limits(subject):
    r, scene, radius, whole = subject
    for tmin, rad in ((1.0, 1.0), (2.0, 1.0), (TMIN, float("nan")), (float("nan"), 1.0)):
        g = r.render_ao(k=SUBJECT_K, radius=rad, tmin=tmin, planes=NAMES)
        assert not g["count"].any() and np.all(bits(g["ao"]) == 0x3F800000), (tmin, rad)
    # every ray as far as the reference's own: unlimited occluded()
    dirs = rt.ao_directions(SUBJECT_K)
    ys, xs = np.mgrid[0:H, 0:W]
    p = r.pick(xs.reshape(-1), ys.reshape(-1))
    o, d = camera_rays(scene, W, H)
    hit, rays = ao_rays(p, o, d, dirs, TMIN, 9999.0)
    flat = rays.reshape(-1, 8)
    far = counts_from(N, hit, r.occluded(flat[:, 0:3], flat[:, 4:7]), SUBJECT_K).reshape(H, W)
    assert far.sum() > whole["count"].sum()
    check_planes(r.render_ao(dirs, radius=9999.0, planes=NAMES), far, p, SUBJECT_K, "radius 9999")


@pytest.mark.parametrize("rect", RECTS, ids=[str(q) for q in RECTS])
def test_rectangles(subject, rect):
    import torch
    r, scene, radius, whole = subject
    want = crop(whole, rect)
    w, h = (rect[2], rect[3]) if rect else (W, H)
    assert same_planes(r.render_ao(k=SUBJECT_K, radius=radius, rect=rect, planes=NAMES), want)
    flat, view = device_planes(w, h)
    assert r.render_ao(k=SUBJECT_K, radius=radius, rect=rect, out=view) is view
    torch.cuda.synchronize()
    assert same_planes(to_numpy(view), want)
    assert canaries_intact(flat)


@pytest.mark.parametrize("name", NAMES)
def test_plane_subsets(subject, name):
    import torch
    r, scene, radius, whole = subject
    alone = r.render_ao(k=SUBJECT_K, radius=radius, planes=(name,))
    assert list(alone) == [name] and same_planes(alone, whole, (name,))
    assert same_planes(r.render_ao(k=SUBJECT_K, radius=radius), whole, ("ao",))       # the default: ao alone
    # the library directly: the plane not asked for is NULL in rt_ao, and a tensor the call was not given keeps every element
    flat, view = device_planes(W, H)
    assert r.render_ao(k=SUBJECT_K, radius=radius, out={name: view[name]})[name] is view[name]
    torch.cuda.synchronize()
    assert same_planes(to_numpy({name: view[name]}), whole, (name,))
    other = NAMES[1 - NAMES.index(name)]
    assert bool((flat[other] == 7).all()), "%s was written by a call that asked for %s" % (other, name)
    assert canaries_intact(flat)


def test_device_form_on_a_side_stream_copies_the_directions_at_the_call(subject):
    import torch
    r, scene, radius, whole = subject
    flat, view = device_planes(W, H)
    dirs = rt.ao_directions(SUBJECT_K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert r.render_ao(dirs, radius=radius, out=view) is view
    dirs[:] = 0.0                                         # the caller's array, right after the call: the enqueued call has its own
    side.synchronize()
    assert same_planes(to_numpy(view), whole)
    assert canaries_intact(flat)


# ---- 6. beside frames in flight; the statistics -------------------------------------------------------------------------------------------
def test_ao_does_not_disturb_frames_or_stats(oracle):
    import torch
    scene, mat = triangle_scene(seed=80, n_models=3)
    r = make_renderer(scene, mat)
    try:
        buf = tri_buffers(scene, mat)
        r.render()
        frames = r.host_frames(4)
        flat, view = device_planes(W, H)
        dirs = rt.ao_directions(SUBJECT_K)

        def batch(query):
            for _ in range(4):
                r.enqueue()
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    r.render_ao(dirs, radius=2.0, out=view)
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
        want, p, _ = composition(r, scene, dirs, 2.0)
        assert kinds_of(want, p, SUBJECT_K)[1] > 0
        check_planes(to_numpy(view), want, p, SUBJECT_K, "beside frames in flight")
        assert canaries_intact(flat)
        before = r.stats()
        again = r.render_ao(dirs, radius=2.0, planes=NAMES)
        after = r.stats()
        for k in before:
            assert after[k] == before[k], k                          # the call changes no statistic, field by field
        assert same_planes(again, to_numpy(view))
        # heatmap, strict mode, the node-walk variant: the same planes
        for setup in (r.showHeatmap, lambda: (r.showRaytracer(), r.set_mode(True)), lambda: r.set_variant(6)):
            setup()
            assert same_planes(r.render_ao(dirs, radius=2.0, planes=NAMES), again)
    finally:
        r.close()


# ---- 8. after the scene changes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["refit", "rebuild", "update"])
def test_after_the_scene_changes(change):
    """update_triangles + refit, update_triangles + rebuild, and an instance update(dt) no frame has carried: the call equals the
    composition on the new state, which differs from the old one."""
    scene, mat = view_scene()
    if change == "rebuild":
        scene = scene.createTriangleScene(scene.meshes, scene.instances, node_capacity="full")
    dirs = rt.ao_directions(SUBJECT_K)
    r = make_renderer(scene, mat)
    try:
        r.render()
        r.read_pixels()
        old, p, _ = composition(r, scene, dirs, 2.0)
        check_planes(r.render_ao(dirs, radius=2.0, planes=NAMES), old, p, SUBJECT_K, "before " + change)
        if change == "update":
            scene.update(0.5)
            r.recalculateScene()
        else:
            root, first, count = mesh_ranges(scene)[1]
            tris = deform(tri_buffers(scene, mat)["triangles"], first, count, "grow")
            r.update_triangles(first, tris[first:first + count])
            r.refit() if change == "refit" else r.rebuild()
        want, p, _ = composition(r, scene, dirs, 2.0)
        assert not np.array_equal(want, old) and kinds_of(want, p, SUBJECT_K)[1] > 0
        check_planes(r.render_ao(dirs, radius=2.0, planes=NAMES), want, p, SUBJECT_K, "after " + change)
    finally:
        r.close()


# ---- 7. errors that need a context, in the header's order -------------------------------------------------------------------------------
def test_errors_in_the_headers_order():
    import torch
    lib = abi.load()
    fp = ctypes.POINTER(ctypes.c_float)
    scene = rt.synthetic_scene(3, 1)
    flat, view = device_planes(16, 16)
    host = {"count": np.full((16, 16), 7, np.uint8), "ao": np.full((16, 16), 7, F)}
    dev_ao = abi.RtAo(**{n: t.data_ptr() for n, t in view.items()})
    host_ao = abi.RtAo(**{n: a.ctypes.data for n, a in host.items()})
    none_ao = abi.RtAo()
    odd_ao = abi.RtAo(count=view["count"].data_ptr(), ao=view["ao"].data_ptr() + 2)
    dirs = rt.ao_directions(4)
    dp = dirs.ctypes.data_as(fp)
    rect = lambda *q: (ctypes.c_uint32 * 4)(*q)
    both = {"rt_render_ao": (lambda c, q, dd, k, g, cap: lib.rt_render_ao(c, q, dd, k, TMIN, 1.0, g, cap, None), dev_ao),
            "rt_render_ao_host": (lambda c, q, dd, k, g, cap: lib.rt_render_ao_host(c, q, dd, k, TMIN, 1.0, g, cap), host_ao)}
    ctx = ctypes.c_void_p()
    abi.check(lib.rt_create(0, ctypes.byref(ctx)))
    try:
        def argument_errors(call, gb):
            """k before everything; then dirs, out, the planes -- whatever the state, the rectangle and the capacity are"""
            for q, cap in ((None, 256), (rect(0, 0, 0, 0), 0)):
                for k in (0, 65):
                    assert call(ctx, q, None, k, None, cap) == abi.RT_ERR_INVALID_ARG and b"k = " in lib.rt_last_error(ctx)
                    assert call(ctx, q, dp, k, ctypes.byref(gb), cap) == abi.RT_ERR_INVALID_ARG and b"k = " in lib.rt_last_error(ctx)
                assert call(ctx, q, None, 4, None, cap) == abi.RT_ERR_INVALID_ARG and b"dirs is NULL" in lib.rt_last_error(ctx)
                assert call(ctx, q, dp, 4, None, cap) == abi.RT_ERR_INVALID_ARG and b"out is NULL" in lib.rt_last_error(ctx)
                assert call(ctx, q, dp, 4, ctypes.byref(none_ao), cap) == abi.RT_ERR_INVALID_ARG and b"planes are NULL" in lib.rt_last_error(ctx)
            assert lib.rt_render_ao(ctx, rect(0, 0, 0, 0), dp, 4, TMIN, 1.0, ctypes.byref(odd_ao), 0, None) == abi.RT_ERR_INVALID_ARG
            assert b"aligned" in lib.rt_last_error(ctx)

        def state_error(word):
            """RT_ERR_STATE naming `word` -- before the (empty) rectangle and the (short) capacity are looked at, after the arguments"""
            for name, (call, gb) in both.items():
                for q, cap in ((None, 256), (rect(0, 0, 0, 0), 0), (rect(0xFFFFFFFF, 0, 2, 1), 0)):
                    assert call(ctx, q, dp, 4, ctypes.byref(gb), cap) == abi.RT_ERR_STATE, name
                    assert word in lib.rt_last_error(ctx) and name.encode() + b":" in lib.rt_last_error(ctx)
                argument_errors(call, gb)

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
                    assert call(ctx, q, dp, 4, g, cap) == abi.RT_ERR_INVALID_ARG, (name, list(q))
                    assert b"rectangle" in lib.rt_last_error(ctx)
            assert call(ctx, None, dp, 4, g, 255) == abi.RT_ERR_CAPACITY
            assert call(ctx, rect(3, 5, 7, 9), dp, 4, g, 62) == abi.RT_ERR_CAPACITY and b"63 pixels" in lib.rt_last_error(ctx)
            argument_errors(call, gb)
        # (the host form has no alignment to ask for)
        off = abi.RtAo(ao=host["ao"].ctypes.data + 2)
        assert lib.rt_render_ao_host(ctx, rect(0, 0, 15, 15), dp, 4, TMIN, 1.0, ctypes.byref(off), 225) == abi.RT_OK
        # the refused calls wrote nothing; a call that is not refused does; NaN limits and tmin >= radius are not errors
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in flat.values()) and np.all(host["count"] == 7)
        for name, (call, gb) in both.items():
            assert call(ctx, None, dp, 4, ctypes.byref(gb), 256) == abi.RT_OK, lib.rt_last_error(ctx)
        torch.cuda.synchronize()
        assert same_planes(to_numpy(view), host) and not np.all(host["count"] == 7) and host["count"].max() <= 4
        assert canaries_intact(flat)
        for tmin, radius in ((float("nan"), 1.0), (1.0, float("nan")), (1.0, 1.0), (2.0, 1.0)):
            assert lib.rt_render_ao_host(ctx, None, dp, 4, tmin, radius, ctypes.byref(host_ao), 256) == abi.RT_OK
            assert not host["count"].any() and np.all(host["ao"] == 1.0)
    finally:
        lib.rt_destroy(ctx)
