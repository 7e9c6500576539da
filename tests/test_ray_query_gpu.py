"""Ray queries on the MI355X (include/rt355.h: rt_trace_rays, rt_trace_rays_host, rt_pick) against the CPU oracle, bit for bit:
triangle scenes against oracle.trace_tri_rays plus a float32 restatement of the hit (RK:344-381, RK:334-338), sphere scenes
against rt_oracle_np._trace and oracle.hit_sphere; the pose a query sees after scene.update() without a frame; picking; queries
beside frames in flight; the three paths against each other."""

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import deepen_top_level, leafy_scene, ref_fixture, spine_scene, tri_buffers, triangle_scene
from oracle import rt_oracle_np
from query_common import axis_rays, camera_rays, check_triangle_hits, random_rays, same, scene_box

pytestmark = pytest.mark.gpu
F = np.float32


def make_renderer(scene, mat=None, W=96, H=64, sky=None):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=2).initialize(sky, mat)
    r.recalculateScene()
    return r


def tri_cases():
    def insts(k):                     # triangle_scene adds a floor to its k models
        return lambda: triangle_scene(seed=40 + k, n_models=k - 1)
    def deep():
        scene, mat = triangle_scene(seed=50, n_models=3)
        deepen_top_level(scene, 3)
        return scene, mat
    return {
        "ref": lambda: (ref_fixture()[0], rt.Material.white()),
        "spine24": lambda: (spine_scene(24), rt.Material.white()),
        "leafy3": lambda: (leafy_scene(3), rt.Material.white()),
        "deepened": deep,
        "inst1": insts(1), "inst3": insts(3), "inst5": insts(5), "inst13": insts(13), "inst17": insts(17),
    }


CASES = tri_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_triangles_against_the_oracle(oracle, name):
    scene, mat = CASES[name]()
    W, H = (336, 212) if name == "ref" else (160, 100)
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        lo, hi = scene_box(buf, scene)
        sets = [camera_rays(scene, W, H), random_rays(lo, hi, 10000, 7), axis_rays(lo, hi, 8)]
        hits = 0
        for o, d in sets:
            h = r.trace_rays(o, d)
            hits += check_triangle_hits(oracle, buf, o, d, h)
        assert hits > 100                 # the rays do meet the scene
    finally:
        r.close()


@pytest.mark.parametrize("n_inst", [3, 17])
def test_query_sees_the_pose_no_frame_has_carried(oracle, n_inst):
    """scene.update() and then a query without a frame: the result is the NEW pose's (the small frame forms carry their instance
    data in their arguments; the device's per-frame buffers lag behind)."""
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    W, H = 160, 100
    r = make_renderer(scene, mat, W, H)
    try:
        r.render()                                        # a frame carries the first pose
        old = tri_buffers(scene, mat)
        scene.update(0.5)
        new = tri_buffers(scene, mat)
        o, d = camera_rays(scene, W, H)
        h = r.trace_rays(o, d)
        check_triangle_hits(oracle, new, o, d, h)
        assert not same(oracle.trace_tri_rays(old, o, d), h["t"])     # the poses differ where the rays look
        scene.update(0.5)                                 # and a pick, again without a frame
        ys, xs = np.mgrid[0:H:7, 0:W:7]
        p = r.pick(xs.reshape(-1), ys.reshape(-1))
        params = scene.pack_params(2)
        dirs = np.stack([oracle.ray_dir(params, W, H, int(x), int(y)) for x, y in zip(xs.reshape(-1), ys.reshape(-1))])
        orig = np.broadcast_to(params[0:3], dirs.shape).astype(F)
        check_triangle_hits(oracle, tri_buffers(scene, mat), orig, dirs, p)
    finally:
        r.close()


def sphere_scene_with_duplicates():
    scene = rt.synthetic_scene(24, 5)
    scene.spheres = list(scene.spheres) + list(scene.spheres)      # equal t for every pair: the lower index wins
    return scene


@pytest.mark.parametrize("n", [1, 37, 1024, 5000, "dup"])
def test_spheres_against_the_oracle(oracle, n):
    scene = sphere_scene_with_duplicates() if n == "dup" else rt.synthetic_scene(n, 11)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    r = make_renderer(scene)
    try:
        lo, hi = (sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)
        count = 2048 if sp.shape[0] > 1000 else 10000
        for o, d in [camera_rays(scene, 96, 64), random_rays(lo, hi, count, 3), axis_rays(lo, hi, 4, 50)]:
            h = r.trace_rays(o, d)
            with np.errstate(all="ignore"):
                nearest, idx = rt_oracle_np._trace(sp, o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])
            miss = idx < 0
            assert np.array_equal(h["prim"], np.where(miss, -1, idx).astype(np.int32))
            assert same(h["t"], np.where(miss, F(-1.0), nearest))
            assert np.all(h["instance"] == -1) and np.all(h["u"] == 0) and np.all(h["v"] == 0) and np.all(h["normal"][miss] == 0)
            hit = np.nonzero(~miss)[0]
            assert hit.size > 0
            if n == "dup":
                assert np.all(h["prim"][hit] < sp.shape[0] // 2)
            for i in hit[:: max(1, hit.size // 200)]:
                ok, t, nrm = oracle.hit_sphere(o[i], d[i], sp[h["prim"][i]], 0.001, 9999.0)
                assert ok and same(t, h["t"][i]) and same(nrm, h["normal"][i])
    finally:
        r.close()


def test_pick_against_the_oracle(oracle):
    scene, mat = triangle_scene(seed=70, n_models=4)
    W, H = 203, 118                                       # a ragged last tile row and column
    r = make_renderer(scene, mat, W, H)
    try:
        xs = np.r_[np.arange(0, W, 13), W - 1]
        ys = np.r_[np.arange(0, H, 9), H - 1]
        gx, gy = np.meshgrid(xs, ys)
        params = scene.pack_params(2)
        dirs = np.stack([oracle.ray_dir(params, W, H, int(x), int(y)) for x, y in zip(gx.reshape(-1), gy.reshape(-1))])
        orig = np.broadcast_to(params[0:3], dirs.shape).astype(F)
        buf = tri_buffers(scene, mat)
        p = r.pick(gx, gy)
        assert p["t"].shape == gx.shape and p["normal"].shape == gx.shape + (3,)
        flat = {k: v.reshape((-1,) + v.shape[gx.ndim:]) for k, v in p.items()}
        assert check_triangle_hits(oracle, buf, orig, dirs, flat) > 10
        mesh = np.asarray(scene.instances.mesh_index)
        assert np.array_equal(flat["mesh"], np.where(flat["instance"] >= 0, mesh[np.maximum(flat["instance"], 0)], -1))
        one = r.pick(int(gx[3, 4]), int(gy[3, 4]))
        assert one["t"].shape == () and same(one["t"], p["t"][3, 4])
        for x, y in [(W, 0), (0, H), (-1, 0)]:
            with pytest.raises(abi.RtError) as e:
                r.pick(x, y)
            assert e.value.code == abi.RT_ERR_INVALID_ARG
        # under a partition, coordinates stay full-frame (rows of tiles this rank does not render included)
        abi.check(r._lib.rt_set_partition(r._ctx, 1, 2), r._ctx)
        q = r.pick(gx, gy)
        for k in p:
            assert np.array_equal(np.ascontiguousarray(q[k]).view(np.uint8), np.ascontiguousarray(p[k]).view(np.uint8)), k
    finally:
        r.close()


def test_queries_do_not_disturb_frames(oracle):
    import torch
    scene, mat = triangle_scene(seed=80, n_models=3)
    W, H = 200, 120
    r = make_renderer(scene, mat, W, H)
    try:
        sky = r.skyboxMaterial
        ref, _, ref_rays = oracle.render_tri(scene.pack_params(2), tri_buffers(scene, mat), sky.faces, W, H)
        r.render()
        buf = tri_buffers(scene, mat)
        o, d = camera_rays(scene, W, H, 3)
        rays = np.zeros((o.shape[0], 8), F)
        rays[:, 0:3], rays[:, 4:7] = o, d
        dev = torch.from_numpy(rays).to("cuda:0")
        frames = r.host_frames(4)

        def batch(query):
            for _ in range(4):
                r.enqueue()
            out = None
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    out = r.trace_rays(dev)
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
        before = r.stats()
        h = out.cpu().numpy()
        hd = r.trace_rays(o, d)
        assert r.stats() == before                               # a query changes no statistic
        check_triangle_hits(oracle, buf, o, d, hd)
        host = np.zeros(o.shape[0], dtype=abi.HIT_DTYPE)
        abi.check(r._lib.rt_trace_rays_host(r._ctx, rays.ctypes.data, rays.shape[0], host.ctypes.data), r._ctx)
        want = h.view(np.uint32)
        assert np.array_equal(want.reshape(-1), host.view(np.uint32))
        # heatmap, strict mode, the node-walk variant: the same answers
        for setup in (r.showHeatmap, lambda: (r.showRaytracer(), r.set_mode(True)), lambda: r.set_variant(6)):
            setup()
            again = r.trace_rays(dev).cpu().numpy().view(np.uint32)
            assert np.array_equal(again, want)
    finally:
        r.close()


def test_device_host_and_pick_paths_agree():
    import torch
    scene, mat = triangle_scene(seed=90, n_models=5)
    W, H = 150, 90
    r = make_renderer(scene, mat, W, H)
    lib = r._lib
    try:
        ys, xs = np.mgrid[0:H:4, 0:W:4]
        p = r.pick(xs.reshape(-1), ys.reshape(-1))
        hits = np.zeros(p["t"].shape[0], dtype=abi.HIT_DTYPE)
        xy = np.ascontiguousarray(np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.uint32))
        abi.check(lib.rt_pick(r._ctx, xy.ctypes.data, xy.shape[0], hits.ctypes.data), r._ctx)
        o, d = camera_rays(scene, W, H, 4)
        rays = np.zeros((o.shape[0], 8), F)
        rays[:, 0:3], rays[:, 4:7] = o, d
        host = np.zeros_like(hits)
        abi.check(lib.rt_trace_rays_host(r._ctx, rays.ctypes.data, rays.shape[0], host.ctypes.data), r._ctx)
        dev = r.trace_rays(torch.from_numpy(rays).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(hits.view(np.uint8), host.view(np.uint8))
        assert np.array_equal(dev.cpu().numpy().view(np.uint8).reshape(-1), host.view(np.uint8))
        out = torch.full((rays.shape[0], 8), 7.0, device="cuda:0")
        assert r.trace_rays(torch.from_numpy(rays).to("cuda:0"), out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), host.view(np.uint8))
        # n == 0: nothing to do
        assert lib.rt_trace_rays_host(r._ctx, None, 0, None) == abi.RT_OK
        assert lib.rt_trace_rays(r._ctx, None, 0, None, None) == abi.RT_OK
        assert lib.rt_pick(r._ctx, None, 0, None) == abi.RT_OK
        assert lib.rt_trace_rays_host(r._ctx, None, 4, None) == abi.RT_ERR_INVALID_ARG
        # the messages whole: NULL pointers, misalignment (the pointers are looked at first), a pixel outside the frame
        err = lambda: lib.rt_last_error(r._ctx)
        assert err() == b"rt_trace_rays_host: NULL argument"
        dev_rays = torch.from_numpy(rays).to("cuda:0")
        assert lib.rt_trace_rays(r._ctx, None, 4, out.data_ptr() + 4, None) == abi.RT_ERR_INVALID_ARG and err() == b"rt_trace_rays: NULL argument"
        for off_rays, off_hits in ((4, 0), (0, 4)):
            assert lib.rt_trace_rays(r._ctx, dev_rays.data_ptr() + off_rays, 1, out.data_ptr() + off_hits, None) == abi.RT_ERR_INVALID_ARG
            assert err() == b"rt_trace_rays: rays and hits must be 16-byte aligned"
        assert lib.rt_pick(r._ctx, None, 4, hits.ctypes.data) == abi.RT_ERR_INVALID_ARG and err() == b"rt_pick: NULL argument"
        outside = np.array([[0, 0], [W, 0]], np.uint32)
        assert lib.rt_pick(r._ctx, outside.ctypes.data, 2, hits.ctypes.data) == abi.RT_ERR_INVALID_ARG and err() == b"rt_pick: pixel outside the frame"
    finally:
        r.close()
    # a context without a scene
    bare = rt.RendererRaytracing(16, 16, rt.synthetic_scene(3, 1)).initialize()
    try:
        rays = np.zeros((1, 8), F)
        rays[0, 6] = -1.0
        hits = np.zeros(1, dtype=abi.HIT_DTYPE)
        assert bare._lib.rt_trace_rays_host(bare._ctx, rays.ctypes.data, 1, hits.ctypes.data) == abi.RT_ERR_STATE
        assert bare._lib.rt_last_error(bare._ctx) == b"rt_trace_rays_host: no scene has been written"
        xy = np.zeros((1, 2), np.uint32)
        assert bare._lib.rt_pick(bare._ctx, xy.ctypes.data, 1, hits.ctypes.data) == abi.RT_ERR_STATE
    finally:
        bare.close()
