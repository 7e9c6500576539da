"""Device top-level builds on the MI355X (include/rt355.h: rt_build_tlas, rt_build_tlas_device, rt_read_blas, rt_read_blas_lookup):
the top-level nodes, BLAS records and BLAS lookup the device leaves against the host model (rt_build_tlas_host: the same inline
arithmetic, run serially -- tests/test_build_tlas_cpu.py pins it to a numpy restatement) bit for bit; the state of the context
against a second context given the same bytes through the three rt_write_* calls; every query family, frames, and the error list.
No tolerance anywhere.  Frames are 96 x 64.

n = 16 / 17 is the edge of the instance sets that travel with the frames, 64 / 65 the wave's, 256 / 257 kBuildShort's (one wave or
the whole block prices and partitions a run).  The floor-only scene is one whose whole node buffer lies in the head that frames
carry: the device's copy of the root records is then brought up to date by the call itself."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from ao_common import ao_of, ao_rays, counts_from
from helpers import diff_stats, obj_floor, random_sky, tri_buffers, triangle_scene
from mask_common import TRIALS, assert_trials_move, instance_masks, twin, visible
from query_common import camera_rays, check_all_queries, check_triangle_hits, random_rays
from refit_common import F, FP, U32, deform, mesh_ranges, view_scene
from test_gbuffer_gpu import hits_of
from tlas_common import (SIZES_GPU, SPINE_HALF, bits, build_host, info_dict, numpy_prims, scene_args, spine_xs, with_top_level)

pytestmark = pytest.mark.gpu

W, H, B = 96, 64, 2
INFO = ctypes.POINTER(abi.RtTlasInfo)


def make(scene, mat, sky):
    return rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky, mat)


def read_state(r):
    """(whole node buffer, BLAS records, BLAS lookup) as the next frame would read them"""
    return r.read_nodes(), r.read_blas(), r.read_blas_lookup()


def same_state(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def frame(r):
    """an awaited frame of the context's state as it is: no host write precedes it (render() would rewrite the per-frame buffers)"""
    r.enqueue()
    r.wait()
    return r.read_pixels(), r.stats()["rays"]


def frames_in_flight(r, n=4):
    host = r.host_frames(n)
    for f in range(n):
        r.enqueue()
        r.read_pixels_async(0, host[f])
    r.wait()
    r.read_pixels_wait()
    return [h.reshape(H, W, 4) for h in host]


def model_of(scene, mat):
    """the host model on the scene's packed buffers -> (tlas, blas, lookup, info)"""
    rc, tlas, blas, lookup, info = build_host(*scene_args(scene, tri_buffers(scene, mat)))
    assert rc == abi.RT_OK
    return tlas, blas, lookup, info


# ---- 1. the bytes ----
@pytest.mark.parametrize("n", SIZES_GPU)
def test_device_build_is_the_model(n):
    scene, mat = triangle_scene(seed=60 + n, n_models=n - 1)
    assert len(scene.instances) == n and scene.tlasNodesMax == 2 * n - 1
    r = make(scene, mat, random_sky(61))
    try:
        r.recalculateScene()
        before = r.read_nodes()
        tlas, blas, lookup, info = model_of(scene, mat)
        if n >= 16:
            assert info["nodes_used"] > 1                     # the input condition: a tree, not one leaf
        got = r.build_top_level()
        assert got == info
        nodes = r.read_nodes()
        cap = scene.tlasNodesMax
        bad = np.nonzero((bits(nodes[:cap]) != bits(tlas)).any(axis=1))[0]
        assert bad.size == 0, "top-level nodes %s differ from the model" % bad[:8]
        assert np.array_equal(bits(nodes[cap:]), bits(before[cap:]))               # no bottom-level node moved
        assert np.array_equal(bits(r.read_blas()), bits(blas)) and np.array_equal(bits(r.read_blas_lookup()), bits(lookup))
        assert np.array_equal(bits(scene.frame["tlas_nodes"]), bits(tlas)) and np.array_equal(bits(scene.frame["blas"]), bits(blas))
        assert np.array_equal(bits(scene.frame["blas_lookup"]), bits(lookup)) and scene.tlasNodesUsed == info["nodes_used"]
        state = read_state(r)
        assert r.build_top_level() == info and same_state(read_state(r), state)    # a second build leaves the same bytes
        r.recalculateScene()                                                      # ... and so does rewriting scene.frame
        assert same_state(read_state(r), state)
    finally:
        r.close()


def test_a_scene_inside_the_head_of_the_node_buffer(oracle):
    """Three instances of a two-triangle floor: five top-level nodes and one bottom-level node, all below node 31 -- rt_write_nodes
    keeps such writes in the host copy that frames carry, and no frame has carried it to the device when the build reads the root."""
    floor = rt.load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 0.8], alignBottom=False, scale=3))
    models = [dict(meshIndex=0, position=[-4.0 + 4.0 * k, 0.5 * k, -6.0], eulers=[0, 25.0 * k, 0]) for k in range(3)]
    scene = rt.SceneRaytracing().createScene([]).createTriangleScene([floor], models)
    assert scene.node_buffer_length() == 6
    mat, sky = rt.Material.white(), random_sky(67)
    r = make(scene, mat, sky)
    try:
        r.recalculateScene()
        tlas, blas, lookup, info = model_of(scene, mat)
        assert info["nodes_used"] == 5
        assert r.build_top_level() == info
        buf = tri_buffers(scene, mat)
        assert np.array_equal(bits(buf["nodes"][:5]), bits(tlas)) and np.array_equal(bits(buf["blas"]), bits(blas))
        assert same_state(read_state(r), (buf["nodes"], buf["blas"], buf["blas_lookup"]))
        ref = oracle.render_tri(scene.pack_params(B), buf, sky.faces, W, H)[0]
        img, _ = frame(r)
        assert np.array_equal(img, ref), diff_stats(img, ref)
    finally:
        r.close()


# ---- 2. the state of the context ----
@pytest.mark.parametrize("n", [3, 16, 17, 65])
def test_the_built_context_is_the_written_one(oracle, n):
    """Context A builds; context B is given A's read-back bytes through rt_write_blas, rt_write_blas_lookup and rt_write_nodes
    (recalculateScene of a scene whose `frame` they are).  Awaited and with four frames in flight both render the same frame with
    the same ray count, the oracle's on those buffers."""
    sky = random_sky(62)
    scene, mat = triangle_scene(seed=70 + n, n_models=n - 1)
    a = make(scene, mat, sky)
    twin_scene, _ = triangle_scene(seed=70 + n, n_models=n - 1)
    b = make(twin_scene, mat, sky)
    try:
        a.recalculateScene()
        b.recalculateScene()
        placeholder = frame(a)
        assert np.array_equal(frame(b)[0], placeholder[0])                        # the same history in both contexts
        a.build_top_level()
        nodes, blas, lookup = read_state(a)
        cap = scene.tlasNodesMax
        twin_scene.frame = dict(blas=blas.copy(), blas_lookup=lookup.copy(), tlas_nodes=nodes[:cap].copy())
        b.recalculateScene()
        assert same_state(read_state(b), (nodes, blas, lookup))
        buf = with_top_level(tri_buffers(twin_scene, mat), nodes[:cap], blas, lookup)
        ref, _, ref_rays = oracle.render_tri(scene.pack_params(B), buf, sky.faces, W, H)
        img_a, rays_a = frame(a)
        img_b, rays_b = frame(b)
        assert np.array_equal(img_a, ref), diff_stats(img_a, ref)
        assert np.array_equal(img_b, ref) and rays_a == rays_b == ref_rays
        assert np.array_equal(placeholder[0], ref)                                 # the reference's tree shows the same picture
        for k, (fa, fb) in enumerate(zip(frames_in_flight(a), frames_in_flight(b))):
            assert np.array_equal(fa, ref) and np.array_equal(fb, ref), k
        assert a.stats()["rays"] == b.stats()["rays"] == ref_rays
        assert a.stats()["tri_form"] == b.stats()["tri_form"] and a.stats()["pair_rebuilds"] == b.stats()["pair_rebuilds"]
        assert same_state(read_state(a), read_state(b))
    finally:
        a.close()
        b.close()


# ---- 3. every query family on a built scene ----
def ao_composition(r, scene, dirs, radius, tmin=0.001):
    """tests/test_render_ao_gpu.py: composition, at this file's frame size: pick() of every pixel, the restated rays, occluded()"""
    ys, xs = np.mgrid[0:H, 0:W]
    p = r.pick(xs.reshape(-1), ys.reshape(-1))
    o, d = camera_rays(scene, W, H)
    hit, rays = ao_rays(p, o, d, dirs, tmin, radius)
    flat = rays.reshape(-1, 8)
    occ = r.occluded(flat[:, 0:3], flat[:, 4:7], flat[:, 3], flat[:, 7])
    return counts_from(W * H, hit, occ, dirs.shape[0]).reshape(H, W), p


@pytest.mark.parametrize("n", [9, 18])
def test_every_query_family_on_a_built_scene(oracle, n):
    """n = 9: the instance data travels with the queries; 18: they read a version of the per-frame buffers"""
    scene, mat = triangle_scene(seed=80 + n, n_models=n - 1)
    sky = random_sky(63)
    r = make(scene, mat, sky)
    try:
        masks = instance_masks(n)
        r.set_instance_masks(masks)                           # before the build: the table is by record index, which the build keeps
        info = r.build_top_level()
        assert info["nodes_used"] > 1
        buf = tri_buffers(scene, mat)
        assert same_state(read_state(r), (buf["nodes"], buf["blas"], buf["blas_lookup"]))
        params = np.asarray(scene.pack_params(B), F)
        lo, hi, _ = numpy_prims(*scene_args(scene, buf)[:3])
        cam = params[0:3]
        sets = [camera_rays(scene, W, H, 2), random_rays(np.maximum(lo.min(axis=0), cam - 20.0), np.minimum(hi.max(axis=0), cam + 20.0), 400, 9)]
        rays = (np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]))
        # the masks set before the build select the same instances after it
        assert_trials_move(oracle, buf, rays[0], rays[1], masks)
        for trial in TRIALS:
            r.set_query_masks(nearest=trial)
            tw = twin(buf, visible(masks, trial, n))
            check_triangle_hits(oracle, tw, rays[0], rays[1], r.trace_rays(*rays))
        r.set_query_masks()
        r.set_instance_masks(None)                            # every instance visible again: the unmasked references
        assert check_all_queries(oracle, r, dict(tri=buf, params=params, faces=sky.faces), rays) > 100
        o, d = camera_rays(scene, W, H)
        assert check_triangle_hits(oracle, buf, o, d, hits_of(r.render_gbuffer())) > 100
        dirs = rt.ao_directions(5)
        want, p = ao_composition(r, scene, dirs, 1.0)
        g = r.render_ao(dirs, radius=1.0, planes=("count", "ao"))
        assert int((want > 0).sum()) > 20 and np.array_equal(g["count"], want) and np.array_equal(bits(g["ao"]), bits(ao_of(want, 5)))
    finally:
        r.close()


# ---- 4. after a refit ----
def test_deform_refit_and_build(oracle):
    scene, mat = view_scene(5)
    sky = random_sky(64)
    r = make(scene, mat, sky)
    try:
        r.render()
        root, first, count = mesh_ranges(scene)[0]
        tris = deform(scene.static["triangles"], first, count, "grow")
        r.update_triangles(first, tris[first:first + count])
        r.refit()
        placeholder = tri_buffers(scene, mat)                 # the refitted trees under the reference's top level
        r.build_top_level()
        buf = tri_buffers(scene, mat)
        assert same_state(read_state(r), (buf["nodes"], buf["blas"], buf["blas_lookup"]))
        tlas, blas, lookup, info = model_of_buffers(scene, placeholder)
        assert np.array_equal(bits(buf["nodes"][:scene.tlasNodesMax]), bits(tlas)) and np.array_equal(bits(buf["blas_lookup"]), bits(lookup))
        ref = oracle.render_tri(scene.pack_params(B), buf, sky.faces, W, H)[0]
        img, _ = frame(r)
        assert np.array_equal(img, ref), diff_stats(img, ref)
        o, d = camera_rays(scene, W, H)
        h = r.trace_rays(o, d)
        t_placeholder = oracle.trace_tri_rays(placeholder, o, d)
        assert np.array_equal(bits(h["t"]), bits(t_placeholder)) and int((t_placeholder > 0).sum()) > 500
    finally:
        r.close()


def model_of_buffers(scene, buf):
    rc, tlas, blas, lookup, info = build_host(*scene_args(scene, buf))
    assert rc == abi.RT_OK
    return tlas, blas, lookup, info


# ---- 5. matrices in device memory ----
@pytest.mark.parametrize("n", [5, 40])
def test_the_device_entry_gives_the_host_entrys_bytes(n):
    import torch
    scene, mat = triangle_scene(seed=90 + n, n_models=n - 1)
    r = make(scene, mat, random_sky(65))
    try:
        info = r.build_top_level()
        state = read_state(r)
        scene.buildTopLevel()                                 # back to the reference's tree, so that the second build has work to do
        r.recalculateScene()
        assert not same_state(read_state(r), state)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                         # produced on a side stream: the call must wait for it
            m = torch.from_numpy(scene.instances.matrices()).to("cuda:0", non_blocking=True) * 1.0
            assert r.build_top_level(m) == info
        assert same_state(read_state(r), state)
        m = torch.from_numpy(scene.instances.matrices()).to("cuda:0")
        scene.buildTopLevel()
        r.recalculateScene()
        assert r.build_top_level(m) == info and same_state(read_state(r), state)   # torch's default stream
        with pytest.raises(ValueError):
            r.build_top_level(m[:, :15])
        off = torch.zeros(16 * n + 1, dtype=torch.float32, device="cuda:0")[1:].view(n, 16)
        with pytest.raises(abi.RtError) as e:
            r.build_top_level(off)                            # not 16-byte aligned
        assert e.value.code == abi.RT_ERR_INVALID_ARG and same_state(read_state(r), state)
    finally:
        r.close()


# ---- 6. the error list ----
def test_every_error_leaves_the_context_alone(oracle):
    scene, mat = triangle_scene(seed=95, n_models=22)          # 23 instances: room for the spine
    sky = random_sky(66)
    r = make(scene, mat, sky)
    L = r._lib
    try:
        r.build_top_level()
        state = read_state(r)
        ref = oracle.render_tri(scene.pack_params(B), tri_buffers(scene, mat), sky.faces, W, H)[0]
        img, _ = frame(r)
        assert np.array_equal(img, ref)
        models, roots, nodes, cap = scene_args(scene, tri_buffers(scene, mat))
        n, n_nodes = len(roots), nodes.shape[0]
        info = abi.RtTlasInfo()

        def call(m=models, rt_=roots, n_=n, cap_=cap, ctx=r._ctx):
            m = None if m is None else np.ascontiguousarray(m, F)
            rt_ = None if rt_ is None else np.ascontiguousarray(rt_, np.uint32)
            return L.rt_build_tlas(ctx, None if m is None else m.ctypes.data_as(FP), None if rt_ is None else rt_.ctypes.data_as(U32), n_, cap_,
                                   ctypes.byref(info))

        def unchanged(what):
            assert same_state(read_state(r), state), what
            assert np.array_equal(frame(r)[0], ref), what

        inv = abi.RT_ERR_INVALID_ARG
        assert call(ctx=None) == inv and call(m=None) == inv and call(rt_=None) == inv
        assert call(n_=0) == inv and call(n_=(1 << 20) + 1) == inv
        beyond, below = roots.copy(), roots.copy()
        beyond[3], below[5] = n_nodes, cap - 1
        assert call(rt_=beyond) == inv and call(rt_=below) == inv and call(cap_=n_nodes + 1) == inv
        assert L.rt_build_tlas_device(r._ctx, ctypes.c_void_p(4), roots.ctypes.data_as(U32), n, cap, None, None) == inv      # misaligned
        unchanged("the bad arguments")
        used = scene.tlasNodesUsed
        assert used > 1 and call(cap_=used - 1) == abi.RT_ERR_CAPACITY and info.nodes_used == used
        unchanged("capacity one short")
        # a spine: the instances scaled to 2^-50 at x = 11^(i - 12), all of mesh 0 (tests/tlas_common.py: spine_xs)
        spine = np.zeros((n, 16), F)
        spine[:, [0, 5, 10]], spine[:, 15] = SPINE_HALF, 1.0
        spine[:, 12] = np.asarray(spine_xs(n), np.float64).astype(F)
        spine_roots = np.full(n, scene.meshes[0].root_node, np.uint32)
        rc, _, _, _, want = build_host(spine, spine_roots, nodes, cap)
        assert rc == abi.RT_ERR_UNSUPPORTED and want["depth"] == 22              # the input condition, on the model alone
        assert call(m=spine, rt_=spine_roots) == abi.RT_ERR_UNSUPPORTED and info_dict(info) == want
        unchanged("a spine of 22 levels")
        out = np.zeros(20 * n, F)
        assert L.rt_read_blas(r._ctx, n, 1, out.ctypes.data_as(FP)) == inv and L.rt_read_blas(r._ctx, 0, 1, None) == inv
        assert L.rt_read_blas(r._ctx, 0xFFFFFFFF, 2, out.ctypes.data_as(FP)) == inv and L.rt_read_blas(r._ctx, n, 0, None) == abi.RT_OK
        assert L.rt_read_blas_lookup(r._ctx, n, 1, out.ctypes.data_as(FP)) == inv and L.rt_read_blas_lookup(r._ctx, 0, 1, None) == inv
        assert call() == abi.RT_OK and info.nodes_used == used                   # and the good call still works
        unchanged("the good call")
    finally:
        r.close()


def test_a_sphere_scene_is_a_state_error():
    scene = rt.synthetic_scene(5, 3)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(None)
    try:
        r.recalculateScene()
        m, roots = np.zeros((1, 16), F), np.array([1], np.uint32)
        assert r._lib.rt_build_tlas(r._ctx, m.ctypes.data_as(FP), roots.ctypes.data_as(U32), 1, 1, None) == abi.RT_ERR_STATE
    finally:
        r.close()
