"""Multi-hit ray queries on the MI355X (include/rt355.h: rt_trace_rays_multi, rt_trace_rays_multi_host), bit for bit: the k
smallest hits under the order (t, instance, prim) against a float32 brute force over every (triangle, instance) pair and over
every sphere, in every triangle kernel form and on sphere scenes on both sides of the chunk size; layers and exact ties; the
nearest, limited and occlusion queries against hit 0; the device and host paths, and what a query must leave alone."""

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi, load_mesh
from compute_raytracer_amd.procedural import obj_floor
from helpers import tri_buffers, triangle_scene
from query_common import (MISS, all_triangle_hits, brute_spheres, camera_rays, check_order, host_multi, k_smallest, pack, random_rays,
                          restate_triangle_hits, same, scene_box)
from test_ray_limits_gpu import FORMS, NOT_EXHAUSTIVE, host_ex, host_occ, quad_stack, same_records, sphere_rays, sphere_setup
from test_ray_query_gpu import make_renderer

pytestmark = pytest.mark.gpu
F = np.float32
L = abi.RT_QUERY_LIMITS
# forms of at least thirteen instances in front of the camera: among 4,000 rays some cross three surfaces, some more than four
DENSE = ("inst13", "inst17", "inst17_u16", "inst17_u32")


def check_layout(h):
    """Filled records first, then exact miss records; returns the count per ray."""
    filled = h["prim"] >= 0
    count = filled.sum(axis=1)
    assert np.array_equal(filled, np.arange(h.shape[1])[None, :] < count[:, None]), "a miss record precedes a hit"
    assert same_records(h[~filled], np.broadcast_to(MISS, ((~filled).sum(),))), "an unused place is not the miss record"
    return count


def check_restated(buf, o, d, h):
    """t, u, v and the normal of every filled record are the float32 restatement's for its (prim, instance)."""
    ray, j = np.nonzero(h["prim"] >= 0)
    g = h[ray, j]
    with np.errstate(all="ignore"):
        t, u, v, nrm = restate_triangle_hits(buf, o[ray], d[ray], g["prim"], g["instance"])
    assert same(t, g["t"]) and same(u, g["u"]) and same(v, g["v"]) and same(nrm, g["normal"])


def check_against_brute(h, want):
    T, I, P, _ = want
    bad = (h["prim"] != P) | (h["instance"] != I) | (h["t"].view(np.uint32) != T.view(np.uint32))
    assert not bad.any(), "the walk and the brute force differ on %d rays, first %s" % (
        int(bad.any(axis=1).sum()), np.nonzero(bad.any(axis=1))[0][:5])


# ---- 1. layers ----------------------------------------------------------------------------------------------------------------
def down_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.9, 0.9, n), np.full(n, 10.0), rng.uniform(-5.9, -4.1, n)], axis=1).astype(F)
    return o, np.tile(np.array([0.0, -1.0, 0.0], F), (n, 1)), rng


@pytest.mark.parametrize("instanced", [False, True])
def test_layers_come_in_order(instanced):
    layers = 9
    scene, mat = quad_stack(layers, instanced)
    r = make_renderer(scene, mat, 64, 40)
    try:
        buf = tri_buffers(scene, mat)
        n = 500
        o, d, rng = down_rays(n, 3)
        for k in (1, 4, 8):
            h = host_multi(r, pack(o, d), 0, k)                                  # layer j is at t = 10 + j, y = -j
            assert np.all(check_layout(h) == k)
            assert np.allclose(o[:, 1:2] + h["t"] * d[:, 1:2], -np.arange(k)[None, :], atol=1e-4)
            if instanced:
                assert np.array_equal(h["instance"], np.broadcast_to(np.arange(k), (n, k)))
            check_order(h, F(0.001), F(9999.0))
            check_restated(buf, o, d, h)
            # tmin between layers j-1 and j: the list starts at layer j and is short near the bottom
            j = rng.integers(0, layers, n)
            tmin = (10.0 + j - rng.uniform(0.05, 0.95, n)).astype(F)
            h = host_multi(r, pack(o, d, tmin, 9999.0), L, k)
            count = check_layout(h)
            assert np.array_equal(count, np.minimum(k, layers - j))
            filled = h["prim"] >= 0
            want_y = -(j[:, None] + np.arange(k)[None, :]).astype(np.float64)
            assert np.allclose((o[:, 1:2] + h["t"] * d[:, 1:2])[filled], want_y[filled], atol=1e-4)
            if instanced:
                assert np.array_equal(h["instance"][filled], (j[:, None] + np.arange(k)[None, :])[filled])
            assert (count < k).any() or k == 1
            check_order(h, tmin, F(9999.0))
            check_restated(buf, o, d, h)
            # a tmax between layers keeps the layers before it
            h2 = host_multi(r, pack(o, d, tmin, (10.0 + j + 1.5).astype(F)), L, k)
            assert np.array_equal(check_layout(h2), np.minimum(k, np.minimum(2, layers - j)))
            assert same_records(h2[:, :2], h[:, :2])
        assert np.all(host_multi(r, pack(o, d, F(10.0 + layers - 0.5), 9999.0), L, 4)["prim"] == -1)
    finally:
        r.close()


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------
def test_coincident_instances_come_in_pairs_ordered_by_instance():
    layers = 9
    mesh = load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 1.0], alignBottom=False, scale=1.0))
    models = [dict(meshIndex=0, position=[0.0, -float(j), -5.0], eulers=[0, 0, 0]) for j in range(layers)] * 2
    scene = rt.SceneRaytracing().createScene([])
    scene.createTriangleScene([mesh], models)                                 # instances j and j + 9 coincide; eighteen: no staged instance data
    mat = rt.Material.white()
    r = make_renderer(scene, mat, 64, 40)
    try:
        buf = tri_buffers(scene, mat)
        n = 500
        o, d, _ = down_rays(n, 5)
        h = host_multi(r, pack(o, d), 0, 8)
        assert np.all(check_layout(h) == 8)
        assert same(h["t"][:, 0::2], h["t"][:, 1::2])
        assert np.array_equal(h["instance"], np.broadcast_to(np.array([0, 9, 1, 10, 2, 11, 3, 12]), (n, 8)))
        check_order(h, F(0.001), F(9999.0))
        check_restated(buf, o, d, h)
        h3 = host_multi(r, pack(o, d), 0, 3)                                   # the cut falls inside a pair: the lower instance stays
        assert same_records(h3, h[:, :3])
        assert np.array_equal(h3["instance"][:, 2], np.full(n, 1))
        cand = all_triangle_hits(buf, o, d)
        check_against_brute(h, k_smallest(n, 8, cand, F(0.001), F(9999.0)))
        # hit 0 on a tie: the same t as the nearest query, whichever of the two instances that one names
        assert same(h["t"][:, 0], host_ex(r, pack(o, d), 0)["t"])
    finally:
        r.close()


def test_duplicated_spheres_come_in_pairs_lower_index_first():
    scene, sp, lo, hi = sphere_setup("dup")
    half = sp.shape[0] // 2
    r = make_renderer(scene)
    try:
        pairs = 0
        for o, d in sphere_rays(scene, sp, lo, hi, 43):
            h = host_multi(r, pack(o, d), 0, 8)
            count = check_layout(h)
            assert np.all(count % 2 == 0)
            assert same(h["t"][:, 0::2], h["t"][:, 1::2])
            filled = h["prim"][:, 0::2] >= 0
            assert np.all(h["prim"][:, 0::2][filled] < half)
            assert np.array_equal(h["prim"][:, 1::2][filled], h["prim"][:, 0::2][filled] + half)
            h3 = host_multi(r, pack(o, d), 0, 3)
            assert same_records(h3, h[:, :3])
            pairs += int(filled.sum())
        assert pairs > 100
    finally:
        r.close()


# ---- 3. every kernel form -----------------------------------------------------------------------------------------------------
def form_rays(name, scene, buf, seed):
    lo, hi = scene_box(buf, scene)
    o1, d1 = camera_rays(scene, 64, 40)
    o2, d2 = random_rays(lo, hi, 1500, seed)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def random_limits(r, o, d, seed):
    """(tmin, tmax) drawn as in test_triangles_tmin_against_the_brute_force_and_occlusion"""
    first = host_ex(r, pack(o, d), 0)["t"]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 4, o.shape[0])
    tmin = np.select([pick == 0, pick == 1, pick == 2],
                     [np.maximum(first, F(0.0)), first * rng.uniform(0.5, 1.5, o.shape[0]).astype(F),
                      rng.uniform(0.0, 30.0, o.shape[0]).astype(F)], F(0.001)).astype(F)
    tmax = np.where(rng.random(o.shape[0]) < 0.5, F(9999.0), tmin + rng.uniform(0.5, 40.0, o.shape[0]).astype(F)).astype(F)
    return tmin, tmax


@pytest.mark.parametrize("name", list(FORMS))
def test_every_form_against_the_brute_force(name):
    scene, mat = FORMS[name]()
    r = make_renderer(scene, mat, 64, 40)
    try:
        buf = tri_buffers(scene, mat)
        o, d = form_rays(name, scene, buf, 23)
        n = o.shape[0]
        with np.errstate(all="ignore"):
            cand = None if name in NOT_EXHAUSTIVE else all_triangle_hits(buf, o, d)
        tmin, tmax = random_limits(r, o, d, 31)
        for k, flags, lo, hi in ((4, 0, F(0.001), F(9999.0)), (8, L, tmin, tmax)):
            # (without the flag words 3 and 7 are ignored, whatever they hold)
            h = host_multi(r, pack(o, d, tmin, tmax), flags, k)
            count = check_layout(h)
            check_order(h, lo, hi)
            check_restated(buf, o, d, h)
            print("%s k=%d: hits per ray %s" % (name, k, np.bincount(count, minlength=k + 1)))
            if cand is None:
                continue
            with np.errstate(all="ignore"):
                want = k_smallest(n, k, cand, lo, hi)
            print("%s k=%d: most hits on a ray before the cut %d" % (name, k, want[3].max()))
            check_against_brute(h, want)
            if name in DENSE:
                assert (count >= 3).any()
                if k == 4:
                    assert (want[3] > k).any()                              # some ray is cut at k
    finally:
        r.close()


# ---- 4. spheres ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37, 1500, "dup"])
def test_spheres_against_the_brute_force(oracle, n):
    scene, sp, lo, hi = sphere_setup(n)
    r = make_renderer(scene)
    try:
        rng = np.random.default_rng(41)
        several = short = 0
        for o, d in sphere_rays(scene, sp, lo, hi, 43):
            m = o.shape[0]
            first = host_ex(r, pack(o, d), 0)["t"]
            first = np.where(first > 0, first, F(5.0)).astype(F)
            pick = rng.integers(0, 4, m)
            reach = F(2.0) * sp[:, 7].max() / np.sqrt((d * d).sum(axis=1))               # (a root behind the origin: up to a diameter)
            tmin = np.select([pick == 0, pick == 1, pick == 2], [first, -rng.uniform(0.0, 1.0, m).astype(F) * reach,
                             first * rng.uniform(0.5, 1.5, m).astype(F)], F(0.001)).astype(F)
            tmax = np.where(rng.random(m) < 0.5, F(9999.0), first * rng.uniform(0.5, 6.0, m).astype(F)).astype(F)
            for flags, a, b in ((0, F(0.001), F(9999.0)), (L, tmin, tmax)):
                rays = pack(o, d, tmin, tmax)
                for k in (1, 8):
                    h = host_multi(r, rays, flags, k)
                    count = check_layout(h)
                    with np.errstate(all="ignore"):
                        want_t, want_i = brute_spheres(sp, o, d, a, b, k)
                    assert np.array_equal(h["prim"], want_i)
                    assert same(h["t"], want_t)
                    assert np.all(h["instance"] == -1) and np.all(h["u"] == 0) and np.all(h["v"] == 0)
                    if k == 1:
                        assert same_records(h[:, 0], host_ex(r, rays, flags))
                        continue
                    several, short = several + int((count >= 3).sum()), short + int(((count > 0) & (count < k)).sum())
                    ray, j = np.nonzero(h["prim"] >= 0)
                    lo_i, hi_i = np.broadcast_to(a, (m,)), np.broadcast_to(b, (m,))
                    for q in range(0, ray.size, max(1, ray.size // 60)):
                        i, g = ray[q], h[ray[q], j[q]]
                        ok, t, nrm = oracle.hit_sphere(o[i], d[i], sp[g["prim"]], lo_i[i], hi_i[i])
                        assert ok and same(t, g["t"]) and same(nrm, g["normal"])
        assert short > 0 and (several > 0 or n == 1)
    finally:
        r.close()


# ---- 5. consistency with the existing queries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f for f in FORMS if f not in NOT_EXHAUSTIVE])
def test_hit_0_is_the_nearest_query_and_occlusion(name):
    scene, mat = FORMS[name]()
    r = make_renderer(scene, mat, 64, 40)
    try:
        buf = tri_buffers(scene, mat)
        o, d = form_rays(name, scene, buf, 29)
        tmin, tmax = random_limits(r, o, d, 37)
        rays = pack(o, d, tmin, tmax)
        hit = 0
        for flags in (0, L):
            near = host_ex(r, rays, flags)
            for k in (1, 5):
                h = host_multi(r, rays, flags, k)
                assert same(h["t"][:, 0], near["t"])                                # (a miss: both -1)
                assert np.array_equal(h["prim"][:, 0] >= 0, near["prim"] >= 0)
                assert np.array_equal(host_occ(r, rays, flags).astype(bool), h["prim"][:, 0] >= 0)
            hit += int((near["prim"] >= 0).sum())
        assert 100 < hit < 2 * o.shape[0]
    finally:
        r.close()


# ---- 6. paths and state -------------------------------------------------------------------------------------------------------
def test_device_and_host_paths_agree_and_no_scene_is_refused():
    import torch
    scene, mat = triangle_scene(seed=91, n_models=4)
    r = make_renderer(scene, mat, 64, 40)
    lib = r._lib
    try:
        o, d = camera_rays(scene, 64, 40)
        rng = np.random.default_rng(1)
        rays = pack(o, d, rng.uniform(0.0, 8.0, o.shape[0]).astype(F), rng.uniform(4.0, 30.0, o.shape[0]).astype(F))
        dev_rays = torch.from_numpy(rays).to("cuda:0")
        for k, limits in ((3, True), (8, False)):
            host = host_multi(r, rays, L if limits else 0, k)
            dev = r.trace_rays_multi(dev_rays, k=k, limits=limits)
            torch.cuda.synchronize()
            assert tuple(dev.shape) == (o.shape[0], k, 8) and dev.dtype == torch.float32
            assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(-1), host.view(np.uint32).reshape(-1))
            out = torch.full((o.shape[0], k, 8), 7.0, device="cuda:0")
            assert r.trace_rays_multi(dev_rays, k=k, limits=limits, out=out) is out
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(-1), host.view(np.uint32).reshape(-1))
            # the numpy form: (n, k) arrays and the count
            res = r.trace_rays_multi(o, d, k=k, **(dict(tmin=rays[:, 3], tmax=rays[:, 7]) if limits else {}))
            assert res["t"].shape == (o.shape[0], k) and res["normal"].shape == (o.shape[0], k, 3)
            assert same(res["t"], host["t"]) and np.array_equal(res["prim"], host["prim"]) and same(res["normal"], host["normal"])
            assert np.array_equal(res["count"], (host["prim"] >= 0).sum(axis=1))
        # a stream of the caller's, 16-byte aligned buffers inside larger ones, n = 1 and a partial last workgroup
        side = torch.cuda.Stream()
        big_rays = torch.zeros(258 * 8 + 4, dtype=torch.float32, device="cuda:0")
        big_hits = torch.full((257 * 4 * 8 + 4,), 3.0, dtype=torch.float32, device="cuda:0")
        big_rays[4:4 + 257 * 8] = dev_rays[:257].reshape(-1)
        torch.cuda.synchronize()
        for n in (1, 257):
            want = host_multi(r, rays[:n], L, 4)
            with torch.cuda.stream(side):
                abi.check(lib.rt_trace_rays_multi(r._ctx, big_rays.data_ptr() + 16, n, L, 4, big_hits.data_ptr() + 16, side.cuda_stream), r._ctx)
            side.synchronize()
            got = big_hits.cpu().numpy()
            assert np.array_equal(got[4:4 + n * 32].view(np.uint32), want.view(np.uint32).reshape(-1))
            assert np.all(got[:4] == 3.0) and np.all(got[4 + n * 32:] == 3.0)           # nothing outside [n][k] is written
            big_hits.fill_(3.0)
        # n == 0, NULL pointers, misalignment
        hits = torch.zeros((4, 4, 8), dtype=torch.float32, device="cuda:0")
        assert lib.rt_trace_rays_multi(r._ctx, None, 0, L, 4, None, None) == abi.RT_OK
        assert lib.rt_trace_rays_multi_host(r._ctx, None, 0, 0, 8, None) == abi.RT_OK
        assert lib.rt_trace_rays_multi(r._ctx, None, 4, L, 4, None, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_multi_host(r._ctx, rays.ctypes.data, 4, 0, 4, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_multi(r._ctx, dev_rays.data_ptr() + 4, 1, 0, 4, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_multi(r._ctx, dev_rays.data_ptr(), 4, 0, 9, hits.data_ptr(), None) == abi.RT_ERR_INVALID_ARG
        # the messages whole, and the order when two arguments are wrong: flags, k, pointers, alignment
        err = lambda: lib.rt_last_error(r._ctx)
        k_msg = b": k = 9 is outside 1 .. RT355_MAX_HITS (%d)" % abi.RT355_MAX_HITS
        for fn, name, tail in ((lib.rt_trace_rays_multi, b"rt_trace_rays_multi", (None,)), (lib.rt_trace_rays_multi_host, b"rt_trace_rays_multi_host", ())):
            assert fn(r._ctx, None, 4, 2, 9, None, *tail) == abi.RT_ERR_INVALID_ARG and err() == name + b": unknown flag bits 0x2"
            assert fn(r._ctx, None, 4, L, 9, None, *tail) == abi.RT_ERR_INVALID_ARG and err() == name + k_msg
            assert fn(r._ctx, None, 4, L, 4, None, *tail) == abi.RT_ERR_INVALID_ARG and err() == name + b": NULL argument"
        for off_rays, off_hits in ((4, 0), (0, 4)):
            assert lib.rt_trace_rays_multi(r._ctx, dev_rays.data_ptr() + off_rays, 1, 0, 4, hits.data_ptr() + off_hits, None) == abi.RT_ERR_INVALID_ARG
            assert err() == b"rt_trace_rays_multi: rays and hits must be 16-byte aligned"
        torch.cuda.synchronize()
    finally:
        r.close()
    bare = rt.RendererRaytracing(16, 16, rt.synthetic_scene(3, 1)).initialize()
    try:
        rays = pack(np.zeros((1, 3), F), np.array([[0.0, 0.0, -1.0]], F))
        hits = np.zeros((1, 4), dtype=abi.HIT_DTYPE)
        for flags in (0, L):
            assert bare._lib.rt_trace_rays_multi_host(bare._ctx, rays.ctypes.data, 1, flags, 4, hits.ctypes.data) == abi.RT_ERR_STATE
            assert bare._lib.rt_last_error(bare._ctx) == b"rt_trace_rays_multi_host: no scene has been written"
    finally:
        bare.close()


@pytest.mark.parametrize("n_inst", [3, 17])
def test_query_sees_the_pose_no_frame_has_carried(n_inst):
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    r = make_renderer(scene, mat, 64, 40)
    try:
        r.render()                                        # a frame carries the first pose
        old = tri_buffers(scene, mat)
        scene.update(0.5)
        new = tri_buffers(scene, mat)
        o, d = camera_rays(scene, 64, 40)
        r.recalculateScene()                              # the per-frame writes, and no frame behind them
        h = host_multi(r, pack(o, d), 0, 4)
        with np.errstate(all="ignore"):
            check_against_brute(h, k_smallest(o.shape[0], 4, all_triangle_hits(new, o, d), F(0.001), F(9999.0)))
            stale = k_smallest(o.shape[0], 4, all_triangle_hits(old, o, d), F(0.001), F(9999.0))
        assert not same(stale[0], h["t"])                 # the poses differ where the rays look
    finally:
        r.close()


def test_queries_leave_frames_and_statistics_alone():
    scene, mat = triangle_scene(seed=81, n_models=3)
    r = make_renderer(scene, mat, 64, 40)
    try:
        r.render()
        before_frame = r.read_pixels().copy()
        o, d = camera_rays(scene, 64, 40)
        before = r.stats()
        host_multi(r, pack(o, d, 0.5, 12.0), L, 8)
        r.trace_rays_multi(o, d, k=2)
        assert r.stats() == before                        # a query changes no statistic
        r.render()
        assert np.array_equal(r.read_pixels(), before_frame)
    finally:
        r.close()
