"""Instance visibility masks on the MI355X (include/rt355.h: rt_write_instance_masks, rt_set_query_masks): every ray-query family, in
every form of the triangle query kernels, against the unmasked references given the twin scene of tests/mask_common.py, bit for
bit; the table across scene writes, mask writes between queries on two streams, frames that must not notice any of it, and sphere
scenes, which have no instances.  The masks and the six ray-mask trials are mask_common's; each test first shows, on the reference
alone, that its trials move the answers."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from ao_common import ao_rays, counts_from, cpu_occluded, cpu_primary_hits
from helpers import random_sky, tri_buffers, triangle_scene
from mask_common import ALL, TRIALS, assert_trials_move, filter_hits, instance_masks, twin, visible
from query_common import (F, MISS, _limits, all_triangle_hits, bits, camera_rays, check_order, check_triangle_hits, host_multi,
                          k_smallest, pack, random_rays, restate_triangle_hits, same, scene_box)
import shade_common
from test_ray_limits_gpu import NOT_EXHAUSTIVE, form_cases, quad_stack
from test_ray_query_gpu import make_renderer
from test_render_samples_cpu import resolve_np

pytestmark = pytest.mark.gpu
FORMS = form_cases()
U32P = ctypes.POINTER(ctypes.c_uint32)


def n_records(buf):
    return np.asarray(buf["blas"]).reshape(-1, 20).shape[0]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def write_masks(r, masks):
    """rt_write_instance_masks itself (set_instance_masks goes through it too)"""
    m = np.ascontiguousarray(masks, np.uint32)
    abi.check(r._lib.rt_write_instance_masks(r._ctx, m.ctypes.data_as(U32P) if m.size else None, m.size), r._ctx)


def pick_rays(oracle, scene, W, H, step=7):
    ys, xs = np.mgrid[0:H:step, 0:W:step]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    params = scene.pack_params(2)
    dirs = np.stack([oracle.ray_dir(params, W, H, int(x), int(y)) for x, y in zip(xs, ys)])
    return xs, ys, np.broadcast_to(params[0:3], dirs.shape).astype(F), dirs


def scene_rays(buf, scene, W, H):
    """mask_common's rays: the camera rays of the frame and 3,000 incoherent ones"""
    lo, hi = scene_box(buf, scene)
    o1, d1 = camera_rays(scene, W, H)
    o2, d2 = random_rays(lo, hi, 3000, 7)
    return np.ascontiguousarray(np.concatenate([o1, o2]), F), np.ascontiguousarray(np.concatenate([d1, d2]), F)


# ---- 1. nearest, bounded, occlusion, pick: every form, the six trials --------------------------------------------------------------
@pytest.mark.parametrize("name", list(FORMS))
def test_nearest_limited_occlusion_and_pick_follow_their_masks(oracle, name):
    """Before the first frame (the instance-staged node walks, the per-frame buffers for seventeen instances) and after one (the pair
    records, where the scene fits them).  The nearest searches carry trial i, the occlusion query trial i + 2: each family must
    follow its own."""
    scene, mat = FORMS[name]()
    W, H = 96, 64
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        nb = n_records(buf)
        masks = instance_masks(nb)
        o, d = scene_rays(buf, scene, W, H)
        if nb >= 3:
            assert_trials_move(oracle, buf, o, d, masks)
        step = 6 if name.startswith("ref") else 3       # the rays of the comparisons that rest on the brute force
        ob, db = np.ascontiguousarray(o[::step]), np.ascontiguousarray(d[::step])
        exhaustive = name not in NOT_EXHAUSTIVE
        first = oracle.trace_tri_rays(buf, ob, db)
        tmin, tmax = _limits(first, 5)
        if exhaustive:
            with np.errstate(all="ignore"):
                cand = all_triangle_hits(buf, ob, db)
        else:
            tmin = np.full_like(tmin, F(0.001))
        xs, ys, po, pd = pick_rays(oracle, scene, W, H)

        def limited_reference(tw, vis):
            """(found, t) of the limited nearest search under `vis`"""
            if exhaustive:
                with np.errstate(all="ignore"):
                    T = k_smallest(ob.shape[0], 1, filter_hits(cand, vis), tmin, tmax)[0][:, 0]
                return T != F(-1.0), T
            t = oracle.trace_tri_rays(tw, ob, db)
            found = (t != F(-1.0)) & (t < tmax)
            return found, np.where(found, t, F(-1.0)).astype(F)

        refs = {}
        for trial in TRIALS:
            vis = visible(masks, trial, nb)
            tw = twin(buf, vis)
            refs[trial] = (tw,) + limited_reference(tw, vis)

        r.set_instance_masks(masks)
        for when in ("before the first frame", "after a frame"):
            for i, trial in enumerate(TRIALS):
                occ_trial = TRIALS[(i + 2) % len(TRIALS)]
                r.set_query_masks(nearest=trial, occlusion=occ_trial)
                tw, found, t_lim = refs[trial]
                what = "%s, %s, trial 0x%x" % (name, when, trial)
                hits = check_triangle_hits(oracle, tw, o, d, r.trace_rays(o, d))
                if not visible(masks, trial, nb).any():
                    assert hits == 0, what
                lim = r.trace_rays(ob, db, tmin=tmin, tmax=tmax)
                got = lim["prim"] >= 0
                assert np.array_equal(got, found), "%s: the limited query and its reference disagree on %d rays" % (what, int((got != found).sum()))
                assert same(lim["t"], t_lim), "%s: limited t differs on %d rays" % (what, int((bits(lim["t"]) != bits(t_lim)).sum()))
                with np.errstate(all="ignore"):
                    t, u, v, nrm = restate_triangle_hits(tw, ob[got], db[got], lim["prim"][got], lim["instance"][got])
                assert same(t, lim["t"][got]) and same(u, lim["u"][got]) and same(v, lim["v"][got]) and same(nrm, lim["normal"][got]), what
                assert np.array_equal(words(lim_records(lim)[~got]), words(np.broadcast_to(MISS, (int((~got).sum()),)))), what
                assert np.all(visible(masks, trial, nb)[lim["instance"][got]]), what
                occ = r.occluded(ob, db, tmin, tmax)
                want_occ = refs[occ_trial][1]
                assert np.array_equal(occ, want_occ), "%s: occlusion (mask 0x%x) differs on %d rays" % (what, occ_trial, int((occ != want_occ).sum()))
                check_triangle_hits(oracle, tw, po, pd, r.pick(xs, ys))
            if when == "before the first frame":
                r.render()
                r.read_pixels()
    finally:
        r.close()


def lim_records(h):
    """trace_rays' dict as rt_hit records"""
    rec = np.zeros(h["t"].shape[0], dtype=abi.HIT_DTYPE)
    for k in ("t", "u", "v", "prim", "instance", "normal"):
        rec[k] = h[k]
    return rec


# ---- 2. the k nearest ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in FORMS if k not in NOT_EXHAUSTIVE])
def test_k_nearest_are_the_visible_hits_in_order(oracle, name):
    scene, mat = FORMS[name]()
    W, H = 96, 64
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        nb = n_records(buf)
        masks = instance_masks(nb)
        o, d = scene_rays(buf, scene, W, H)
        if nb >= 3:
            assert_trials_move(oracle, buf, o, d, masks)
        step = 6 if name.startswith("ref") else 3
        o, d = np.ascontiguousarray(o[::step]), np.ascontiguousarray(d[::step])
        n = o.shape[0]
        with np.errstate(all="ignore"):
            cand = all_triangle_hits(buf, o, d)
        r.set_instance_masks(masks)
        for when in ("before the first frame", "after a frame"):
            for trial in TRIALS:
                r.set_query_masks(nearest=trial, occlusion=ALL ^ trial)     # (the occlusion mask is not the multi-hit query's)
                vis = visible(masks, trial, nb)
                near = r.trace_rays(o, d)
                for k in (3, 6):
                    what = "%s, %s, trial 0x%x, k = %d" % (name, when, trial, k)
                    h = host_multi(r, pack(o, d), 0, k)
                    filled = h["prim"] >= 0
                    assert np.array_equal(filled, np.arange(k)[None, :] < filled.sum(axis=1)[:, None]), what
                    assert np.array_equal(words(h[~filled]), words(np.broadcast_to(MISS, (int((~filled).sum()),)))), what
                    check_order(h, F(0.001), F(9999.0))
                    with np.errstate(all="ignore"):
                        T, I, P, _ = k_smallest(n, k, filter_hits(cand, vis), F(0.001), F(9999.0))
                        ray, j = np.nonzero(filled)
                        g = h[ray, j]
                        t, u, v, nrm = restate_triangle_hits(buf, o[ray], d[ray], g["prim"], g["instance"])
                    assert same(t, g["t"]) and same(u, g["u"]) and same(v, g["v"]) and same(nrm, g["normal"]), what
                    bad = (h["prim"] != P) | (h["instance"] != I) | (bits(h["t"]) != bits(T))
                    assert not bad.any(), "%s: the walk and the filtered brute force differ on %d rays" % (what, int(bad.any(axis=1).sum()))
                    assert same(h["t"][:, 0], near["t"]) and np.array_equal(h["prim"][:, 0] >= 0, near["prim"] >= 0), what
            if when == "before the first frame":
                r.render()
                r.read_pixels()
    finally:
        r.close()


def test_k_nearest_through_a_stack_of_instances_reports_the_visible_ones():
    k = 7
    scene, mat = quad_stack(k, True)
    r = make_renderer(scene, mat, 64, 40)
    try:
        masks = instance_masks(k)
        r.set_instance_masks(masks)
        rng = np.random.default_rng(3)
        n = 300
        o = np.stack([rng.uniform(-0.9, 0.9, n), np.full(n, 10.0), rng.uniform(-5.9, -4.1, n)], axis=1).astype(F)
        d = np.tile(np.array([0.0, -1.0, 0.0], F), (n, 1))
        seen = set()
        for trial in TRIALS:
            r.set_query_masks(nearest=trial)
            want = np.nonzero(visible(masks, trial, k))[0]                  # layer j is instance j, at t = 10 + j
            h = host_multi(r, pack(o, d), 0, 8)
            assert np.all((h["prim"] >= 0).sum(axis=1) == want.size), "trial 0x%x" % trial
            assert np.array_equal(h["instance"][:, :want.size], np.broadcast_to(want, (n, want.size))), "trial 0x%x" % trial
            assert np.allclose(h["t"][:, :want.size], 10.0 + want[None, :], atol=1e-4)
            seen.add(tuple(want))
        assert len(seen) >= 4 and () in seen
    finally:
        r.close()


# ---- 3. shaded rays and supersampled frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inst5", "ref"])
def test_shaded_rays_and_supersampled_frames_see_the_twin(oracle, name):
    """Path rays and shadow rays alike carry the nearest mask: the oracle's frames of the twin, bit for bit."""
    scene, mat = FORMS[name]()
    W, H = 48, 32
    sky = random_sky(31)
    r = make_renderer(scene, mat, W, H, sky=sky)
    try:
        buf = tri_buffers(scene, mat)
        nb = n_records(buf)
        masks = instance_masks(nb)
        params = np.asarray(scene.pack_params(2), F)
        oc, dc = shade_common.camera_rays(params, W, H)
        base = oracle.render_tri(params, buf, sky.faces, W, H, want_float=True)[1]
        r.set_instance_masks(masks)
        moved = 0
        for trial in TRIALS:
            r.set_query_masks(nearest=trial, occlusion=ALL ^ trial)
            tw = twin(buf, visible(masks, trial, nb))
            img8, flt, _ = oracle.render_tri(params, tw, sky.faces, W, H, want_float=True)
            moved += int((bits(flt) != bits(base)).any(axis=-1).sum() >= 20)
            got = r.shade_rays(oc, dc, compose=True)
            diff = (bits(got[:, 0:3]) != bits(flt.reshape(-1, 3))).any(axis=-1)
            assert not diff.any(), "trial 0x%x: %d of %d shaded camera rays differ from the oracle's frame of the twin" % (trial, int(diff.sum()), W * H)
            assert np.array_equal(r.render_samples(1), img8), "trial 0x%x: render_samples(1)" % trial
            big = oracle.render_tri(params, tw, sky.faces, 2 * W, 2 * H, want_float=True)[1]
            img, f2 = r.render_samples(2, float_out=True)
            want = resolve_np(big, 2)
            assert np.array_equal(bits(f2[:, :, 0:3]), bits(want)), "trial 0x%x: render_samples(2)" % trial
            assert np.array_equal(img[:, :, 0:3], shade_common.quantise(want)) and np.all(img[:, :, 3] == 255)
        assert moved >= 3                                   # the masks change the picture
    finally:
        r.close()


# ---- 4. geometry frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", [None, (3, 5, 41, 23)], ids=["whole", "ragged"])
def test_geometry_frames_are_the_masked_pick(oracle, rect):
    scene, mat = FORMS["inst5"]()
    W, H = 70, 45
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        masks = instance_masks(n_records(buf))
        o, d = camera_rays(scene, W, H)
        assert_trials_move(oracle, buf, o, d, masks)
        r.set_instance_masks(masks)
        x0, y0, w, h = rect if rect else (0, 0, W, H)
        ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
        answers = set()
        for trial in TRIALS:
            r.set_query_masks(nearest=trial, occlusion=ALL ^ trial)
            p = r.pick(xs, ys)
            g = r.render_gbuffer(rect)
            assert np.array_equal(bits(g["depth"]), bits(p["t"]))
            assert np.array_equal(bits(g["normal"][:, :, 0:3]), bits(p["normal"])) and np.all(bits(g["normal"][:, :, 3]) == 0)
            assert np.array_equal(g["ids"][:, :, 0], p["prim"]) and np.array_equal(g["ids"][:, :, 1], p["instance"])
            assert np.array_equal(bits(g["uv"][:, :, 0]), bits(p["u"])) and np.array_equal(bits(g["uv"][:, :, 1]), bits(p["v"]))
            vis = visible(masks, trial, masks.size)
            hit = p["instance"] >= 0
            assert np.all(vis[p["instance"][hit]])
            answers.add(g["ids"].tobytes())
        assert len(answers) >= 3
    finally:
        r.close()


# ---- 5. ambient occlusion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size,radius", [("inst5", (24, 16), 2.0), ("inst17", (24, 16), 1.0), ("ref", (12, 8), 1.0)])
def test_ambient_occlusion_takes_both_masks(oracle, name, size, radius):
    """The primary ray carries the nearest mask, the k rays the occlusion mask: the counts by the CPU alone, from the two twins."""
    scene, mat = FORMS[name]()
    W, H = size
    K = 8
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        nb = n_records(buf)
        masks = instance_masks(nb)
        dirs = rt.ao_directions(K)
        o, d = camera_rays(scene, W, H)
        r.set_instance_masks(masks)
        planes = []
        for nearest, occlusion in ((ALL, ALL), (0x80000004, 0x1), (0x1, 0x80000004)):
            tw_n, tw_o = twin(buf, visible(masks, nearest, nb)), twin(buf, visible(masks, occlusion, nb))
            p = cpu_primary_hits(oracle, tw_n, o, d)
            hit, rays = ao_rays(p, o, d, dirs, 0.001, radius)
            want = counts_from(W * H, hit, cpu_occluded(oracle, tw_o, rays.reshape(-1, 8)), K).reshape(H, W)
            r.set_query_masks(nearest=nearest, occlusion=occlusion)
            g = r.render_ao(dirs, radius=radius, tmin=0.001, planes=("count", "ao"))
            assert np.array_equal(g["count"], want), "nearest 0x%x, occlusion 0x%x: %d counts differ" % (nearest, occlusion, int((g["count"] != want).sum()))
            assert np.array_equal(bits(g["ao"]), bits(((F(K) - want.astype(F)) / F(K)).astype(F)))
            planes.append(want.tobytes())
        assert len(set(planes)) == 3                        # the two masked frames differ from the unmasked one and from each other
    finally:
        r.close()


# ---- 6. lifecycle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst", [3, 17])
def test_masks_hold_across_a_pose_no_frame_has_carried(oracle, n_inst):
    scene, mat = triangle_scene(seed=60 + n_inst, n_models=n_inst - 1)
    W, H = 96, 64
    r = make_renderer(scene, mat, W, H)
    try:
        masks = instance_masks(n_inst)
        r.set_instance_masks(masks)
        r.render()
        old = tri_buffers(scene, mat)
        scene.update(0.5)
        new = tri_buffers(scene, mat)
        o, d = camera_rays(scene, W, H)
        for trial in (0x1, 0x80000004, 0x2):
            vis = visible(masks, trial, n_inst)
            r.set_query_masks(nearest=trial, occlusion=trial)
            h = r.trace_rays(o, d)                          # (no frame in between)
            check_triangle_hits(oracle, twin(new, vis), o, d, h)
            if trial == 0x1:
                assert not same(oracle.trace_tri_rays(twin(old, vis), o, d), h["t"])     # the poses differ where the rays look
                assert not same(oracle.trace_tri_rays(new, o, d), h["t"])                # ... and so do masked and unmasked
            assert np.array_equal(r.occluded(o, d), h["prim"] >= 0)
    finally:
        r.close()


def test_the_table_outlives_the_records_and_clears(oracle):
    """Five records, then eight, then three in one context: the table stays what it was, records beyond it are visible; n = 0 brings
    the defaults back."""
    W, H = 96, 64
    scenes = [triangle_scene(seed=45, n_models=4), triangle_scene(seed=48, n_models=7), triangle_scene(seed=43, n_models=2)]
    scene, mat = scenes[0]
    r = make_renderer(scene, mat, W, H)
    try:
        masks = instance_masks(5)
        write_masks(r, masks)
        for scene, mat in scenes:
            r.scene, r.meshMaterial, r.loaded = scene, mat, False
            r.recalculateScene()
            buf = tri_buffers(scene, mat)
            nb = n_records(buf)
            o, d = camera_rays(scene, W, H)
            for trial in (0x1, 0x80000004, 0):
                r.set_query_masks(nearest=trial, occlusion=trial)
                vis = visible(masks, trial, nb)
                if nb > 5:
                    assert np.all(vis[5:] == (trial != 0))
                hits = check_triangle_hits(oracle, twin(buf, vis), o, d, r.trace_rays(o, d))
                assert (hits > 20) == (trial != 0)
                assert not same(oracle.trace_tri_rays(buf, o, d), oracle.trace_tri_rays(twin(buf, vis), o, d))
        assert r._lib.rt_write_instance_masks(r._ctx, None, 0) == abi.RT_OK
        for trial in (0x1, ALL):
            r.set_query_masks(nearest=trial, occlusion=trial)
            check_triangle_hits(oracle, buf, o, d, r.trace_rays(o, d))
        r.set_instance_masks(masks)
        r.set_instance_masks(None)
        r.set_query_masks(0x2, 0x2)
        check_triangle_hits(oracle, buf, o, d, r.trace_rays(o, d))
        r.set_query_masks()
        assert r._lib.rt_write_instance_masks(r._ctx, None, 3) == abi.RT_ERR_INVALID_ARG
        assert r._lib.rt_last_error(r._ctx) == b"rt_write_instance_masks: masks is NULL"
    finally:
        r.close()


@pytest.mark.parametrize("n_inst", [5, 17])
def test_a_mask_write_between_two_streams_and_the_three_paths(oracle, n_inst):
    """Device-form queries return before they have run: the one enqueued before a mask write answers by the old table, the one after it
    -- on another stream -- by the new one, whatever the streams' timing.  Five instances travel in the arguments; seventeen read the
    device table.  Then the device, host and pick paths against each other."""
    import torch
    scene, mat = triangle_scene(seed=40 + n_inst, n_models=n_inst - 1)
    W, H = 96, 64
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        old, new = instance_masks(n_inst), instance_masks(n_inst)[::-1].copy()
        trial = 0x80000004
        o, d = scene_rays(buf, scene, W, H)
        n = o.shape[0]
        t_old = oracle.trace_tri_rays(twin(buf, visible(old, trial, n_inst)), o, d)
        t_new = oracle.trace_tri_rays(twin(buf, visible(new, trial, n_inst)), o, d)
        assert int((bits(t_old) != bits(t_new)).sum()) >= 20
        dev = torch.from_numpy(pack(o, d)).to("cuda:0")
        r.set_instance_masks(old)
        r.set_query_masks(nearest=trial, occlusion=trial)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = r.trace_rays(dev)
            first_occ = r.occluded(dev)
        r.set_instance_masks(new)
        second = r.trace_rays(dev)                          # the default stream
        r.set_query_masks(nearest=ALL, occlusion=ALL)       # (a later change does not reach a query already enqueued)
        torch.cuda.synchronize()
        for got, masks in ((first, old), (second, new)):
            h = np.ascontiguousarray(got.cpu().numpy()).view(abi.HIT_DTYPE).reshape(n)
            check_triangle_hits(oracle, twin(buf, visible(masks, trial, n_inst)), o, d, h)
        assert np.array_equal(first_occ.cpu().numpy().astype(bool), t_old != F(-1.0))
        # the three paths
        r.set_query_masks(nearest=trial, occlusion=trial)
        host = np.zeros(n, dtype=abi.HIT_DTYPE)
        rays = pack(o, d)
        abi.check(r._lib.rt_trace_rays_host(r._ctx, rays.ctypes.data, n, host.ctypes.data), r._ctx)
        assert np.array_equal(words(second.cpu().numpy()).reshape(-1), words(host))
        m = W * H                                           # (the first W * H rays are the frame's camera rays)
        ys, xs = np.mgrid[0:H, 0:W]
        xy = np.ascontiguousarray(np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.uint32))
        picked = np.zeros(m, dtype=abi.HIT_DTYPE)
        abi.check(r._lib.rt_pick(r._ctx, xy.ctypes.data, m, picked.ctypes.data), r._ctx)
        assert np.array_equal(picked["prim"] >= 0, host["prim"][:m] >= 0)
        check_triangle_hits(oracle, twin(buf, visible(new, trial, n_inst)), o[:m], d[:m],
                            {k: picked[k] for k in ("t", "u", "v", "prim", "instance", "normal")})
    finally:
        r.close()


# ---- 7. frames are not touched ---------------------------------------------------------------------------------------------------------
def test_frames_ignore_every_mask(oracle):
    import torch
    scene, mat = triangle_scene(seed=81, n_models=3)
    W, H = 160, 100
    r = make_renderer(scene, mat, W, H)
    try:
        buf = tri_buffers(scene, mat)
        nb = n_records(buf)
        ref, _, ref_rays = oracle.render_tri(scene.pack_params(2), buf, r.skyboxMaterial.faces, W, H)
        r.render()
        assert np.array_equal(r.read_pixels(), ref)
        plain = r.stats()
        o, d = camera_rays(scene, W, H, 3)
        dev = torch.from_numpy(pack(o, d)).to("cuda:0")
        frames = r.host_frames(4)
        masks = instance_masks(nb)
        want = oracle.trace_tri_rays(twin(buf, visible(masks, 0x1, nb)), o, d)
        assert int((bits(want) != bits(oracle.trace_tri_rays(buf, o, d))).sum()) >= 20

        def batch(query):
            for _ in range(4):
                r.enqueue()
            out = None
            if query:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    r.set_instance_masks(masks)             # a mask write and masked queries beside the frames in flight
                    r.set_query_masks(0x1, 0x1)
                    out = (r.trace_rays(dev), r.occluded(dev))
                    r.set_instance_masks(np.zeros(nb, np.uint32))
                    r.set_query_masks(0, 0)
                    out += (r.trace_rays(dev),)
            r.enqueue()
            for k in range(4):
                r.read_pixels_async(k, frames[k])
            r.wait()
            r.read_pixels_wait()
            if query:
                side.synchronize()
            return out

        # awaited, every instance hidden and both query masks 0: the frame of the original buffers, the statistics of before
        r.set_instance_masks(np.zeros(nb, np.uint32))
        r.set_query_masks(0, 0)
        assert np.all(r.trace_rays(o, d)["prim"] == -1)
        r.render()
        assert np.array_equal(r.read_pixels(), ref)
        for k in ("rays", "kernel_id", "tri_form"):
            assert r.stats()[k] == plain[k], k
        assert r.stats()["rays"] == ref_rays
        r.set_instance_masks(None)
        r.set_query_masks()
        batch(False)
        batch(False)                      # (the library now knows the caller keeps frames in flight: the same form for both)
        s0 = r.stats()
        # four frames in flight, masked queries and two mask writes beside them
        hits, occ, none = batch(True)
        s1 = r.stats()
        for f in frames + [r.read_pixels()]:
            assert np.array_equal(f, ref)
        assert s1["frames"] == s0["frames"] + 5 and s1["batch_frames"] == s0["batch_frames"]
        for k in ("rays", "kernel_id", "tri_form"):
            assert s1[k] == s0[k], k
        assert s1["rays"] == ref_rays
        h = np.ascontiguousarray(hits.cpu().numpy()).view(abi.HIT_DTYPE).reshape(o.shape[0])
        check_triangle_hits(oracle, twin(buf, visible(masks, 0x1, nb)), o, d, h)
        assert np.array_equal(occ.cpu().numpy().astype(bool), want != F(-1.0))
        assert np.all(np.ascontiguousarray(none.cpu().numpy()).view(abi.HIT_DTYPE)["prim"] == -1)
        before = r.stats()
        r.trace_rays(o, d)
        r.set_instance_masks(masks)
        assert r.stats() == before                          # neither a masked query nor a mask write changes a statistic
    finally:
        r.close()


# ---- 8. sphere scenes have no instances ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 1024])
def test_sphere_scenes_keep_and_ignore_the_masks(n):
    scene = rt.synthetic_scene(n, 11)
    W, H = 64, 40
    sky = random_sky(33)
    r = make_renderer(scene, None, W, H, sky=sky)
    try:
        sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
        lo, hi = (sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)
        o1, d1 = camera_rays(scene, W, H)
        o2, d2 = random_rays(lo, hi, 1000, 3)
        o, d = np.ascontiguousarray(np.concatenate([o1, o2]), F), np.ascontiguousarray(np.concatenate([d1, d2]), F)
        rng = np.random.default_rng(5)
        tmin = rng.uniform(0.0, 4.0, o.shape[0]).astype(F)
        tmax = (tmin + rng.uniform(0.5, 40.0, o.shape[0])).astype(F)
        ys, xs = np.mgrid[0:H:5, 0:W:5]

        def every_family():
            g = r.render_gbuffer()
            a = r.render_ao(k=8, radius=2.0, planes=("count", "ao"))
            img, flt = r.render_samples(2, float_out=True)
            p = r.pick(xs, ys)
            return [lim_records(r.trace_rays(o, d)), lim_records(r.trace_rays(o, d, tmin=tmin, tmax=tmax)), r.occluded(o, d, tmin, tmax),
                    host_multi(r, pack(o, d), 0, 3), host_multi(r, pack(o, d), 0, 6), r.shade_rays(o1, d1, compose=True),
                    img, flt, g["depth"], g["normal"], g["ids"], g["uv"], a["count"], a["ao"], lim_records({k: v.reshape((-1,) + v.shape[2:]) for k, v in p.items()})]

        plain = every_family()
        assert (plain[0]["prim"] >= 0).sum() > 100 and plain[2].sum() > 100
        r.set_instance_masks(np.zeros(4, np.uint32))
        r.set_query_masks(0, 0)
        masked = every_family()
        for a, b in zip(plain, masked):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    finally:
        r.close()
