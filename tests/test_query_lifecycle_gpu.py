"""Ray queries across every scene change a host can make, on the MI355X: one renderer and one context per test, a scripted sequence of
writes, and after every step every query family (tests/query_common.py: check_all_queries -- nearest, limited, occlusion, multi-hit
k = 3 and 6, shaded with compose, pick) against the state the host holds NOW, bit for bit.  Queries do not go through rt_enqueue:
query_prepare (rt_api.hip) decides on its own where the instance data is (the arguments, or a version of the per-frame buffers),
whether the relinked pair records may be walked (tri_pairs_current: never rebuilt by a query), which corner array, node count and
sphere count hold -- a query that reads a stale one of these returns plausible hits.  No frame is rendered unless the step says so.

Where a step changes the geometry the rays look at, the oracle alone first shows that the old state would answer otherwise on the
step's rays; every step but the empty scene's has more than 100 hits.  Shaded queries take the frame's own camera rays (a shaded ray
stands for a pixel only with the direction the frame itself forms: tests/test_shade_rays_gpu.py), all of them: none is left out."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import drift_spheres, random_sky, tri_buffers, triangle_scene
from oracle import rt_oracle_np
from query_common import (F, all_triangle_hits, axis_rays, bits, camera_rays, check_all_queries, check_order, check_triangle_hits,
                          host_multi, k_smallest, pack, random_rays, same, scene_box)

pytestmark = pytest.mark.gpu
W, H, B = 160, 100, 2
FP = ctypes.POINTER(ctypes.c_float)


def tri_state(scene, mat, sky):
    return dict(tri=tri_buffers(scene, mat), params=np.asarray(scene.pack_params(B), F), faces=sky.faces)


def sphere_state(scene, sky):
    return dict(spheres=np.asarray(scene.pack_spheres(), F).reshape(-1, 8), params=np.asarray(scene.pack_params(B), F), faces=sky.faces)


def scene_of(records):
    """A sphere scene (the reference's camera and light) of the (n, 8) float32 records, bit for bit."""
    return rt.SceneRaytracing().createScene([rt.Sphere(s[0:3], s[7], s[4:7]) for s in np.asarray(records, F).reshape(-1, 8)])


def step_rays(scene, state, n_random=1500):
    """The rays of one step: the frame's camera rays at every second pixel, incoherent rays through the scene's box, rays along
    the axes -- about 5.6k."""
    if "tri" in state:
        lo, hi = scene_box(state["tri"], scene)
    else:
        sp = state["spheres"][1:] if state["spheres"].shape[0] > 1 else state["spheres"]        # (without the ground sphere's box)
        lo, hi = ((sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)) if sp.shape[0] else (
            np.array([-12.0, 0.0, -26.0]), np.array([12.0, 4.0, -3.0]))
    sets = [camera_rays(scene, W, H, 2), random_rays(lo, hi, n_random, 7), axis_rays(lo, hi, 8, per_axis=20)]
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


def first_t(oracle, state, rays):
    """The oracle's nearest t (-1: none) of `rays` against `state`."""
    o, d = rays
    if "tri" in state:
        return oracle.trace_tri_rays(state["tri"], o, d)
    with np.errstate(all="ignore"):
        nearest, idx = rt_oracle_np._trace(state["spheres"], o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])
    return np.where(idx < 0, F(-1.0), nearest).astype(F)


class Script:
    """One renderer, one context: query(scene, state) checks every family against `state`; moved_from: the state before a step
    that changed the geometry -- the oracle must tell the two apart on the step's rays."""
    def __init__(self, oracle, r):
        self.oracle, self.r = oracle, r
        self.hits = []

    def query(self, scene, state, moved_from=None, n_random=1500, empty=False):
        rays = step_rays(scene, state, n_random)
        if moved_from is not None:
            assert not same(first_t(self.oracle, moved_from, rays), first_t(self.oracle, state, rays)), "the step's rays do not see the change"
        hits = check_all_queries(self.oracle, self.r, state, rays)
        assert hits == 0 if empty else hits > 100, hits
        self.hits.append(hits)
        return state

    def replace(self, scene, mat=None):
        """a new scene in the same context: everything is written again by the next recalculateScene()"""
        self.r.scene = scene
        if mat is not None:
            self.r.meshMaterial = mat
        self.r.loaded = False


def test_triangle_scene_lifecycle(oracle):
    sky = random_sky(21)
    scene, mat = triangle_scene(seed=101, n_models=2)
    # (triangle_scene hands model k mesh k % 2: both sphere meshes are referenced.  Step 4 needs a mesh no instance has named, as
    # the mesh-change frame test has: both models start on the coarse sphere, the fine one -- mesh 1 -- stays unreferenced)
    scene.instances.mesh_index[1] = 0
    scene.buildTopLevel()
    assert sorted(set(int(k) for k in scene.instances.mesh_index)) == [0, 2]
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky, mat)
    L = r._lib
    s = Script(oracle, r)
    try:
        # 1. written, no frame ever: no relinked copy exists -- inst = 1, the instance-staged node walk
        r.recalculateScene()
        st = s.query(scene, tri_state(scene, mat, sky))
        assert r.stats()["pair_rebuilds"] == 0 and r.stats()["frames"] == 0
        # 2. a frame builds the copy: inst = 1, tri_pairs_current -- the pair forms
        r.render()
        assert r.stats()["pair_rebuilds"] == 1
        s.query(scene, st)
        # 3. a new pose and no frame: the pair forms with the new roots' metas and the new records in the arguments
        scene.update(0.5)
        st = s.query(scene, tri_state(scene, mat, sky), moved_from=st)
        # 4. model 0 takes the mesh no instance has named: rt_flow_covers fails, the copy must be refused -- the node walk
        scene.instances.mesh_index[0] = 1
        scene.update(0.1)
        r.recalculateScene()
        st = s.query(scene, tri_state(scene, mat, sky), moved_from=st)
        assert r.stats()["pair_rebuilds"] == 1                          # (a query never rebuilds the copy)
        # 5. a frame rebuilds the copy with the new root: the pair forms again
        r.render()
        assert r.stats()["pair_rebuilds"] == 2
        s.query(scene, st)
        # 6. the BLAS nodes written again, the same bytes: flow_dirty -- the node walk
        nodes = np.ascontiguousarray(scene.pack_blas_nodes(), np.float32)
        abi.check(L.rt_write_nodes(r._ctx, 32 * scene.tlasNodesMax, nodes.ctypes.data_as(FP), nodes.shape[0]), r._ctx)
        s.query(scene, st)
        # 7. the whole node buffer, head included, in one call; then a new pose through the per-frame head write: still dirty, the
        #    walk over the head the arguments carry
        whole = np.ascontiguousarray(st["tri"]["nodes"], np.float32)
        abi.check(L.rt_write_nodes(r._ctx, 0, whole.ctypes.data_as(FP), whole.shape[0]), r._ctx)
        scene.update(0.4)
        r.recalculateScene()
        st = s.query(scene, tri_state(scene, mat, sky), moved_from=st)
        # 8. a lookup table twice the instance list, the leaves naming the copy: inst = 0, no version holds the state -- drain and
        #    apply_version(0); then the normal table again: back to inst = 1
        normal = dict(scene.frame)
        look = np.asarray(scene.frame["blas_lookup"], np.float32)
        scene.frame["blas_lookup"] = np.concatenate([look, look])
        t = np.asarray(scene.frame["tlas_nodes"], np.float32).copy()
        t[t[:, 7] > 0, 3] += len(look)
        scene.frame["tlas_nodes"] = t
        s.query(scene, tri_state(scene, mat, sky))
        scene.frame = normal
        r.recalculateScene()
        s.query(scene, st)
        # 9. another scene of twenty instances (over the sixteen whose records travel with a frame), no frame: blas_on is off, the
        #    records are in every version (write_versions) -- the version path
        scene9, mat9 = triangle_scene(seed=102, n_models=19, rings=4, sectors=5)
        assert len(scene9.instances) == 20
        s.replace(scene9, mat9)
        r.recalculateScene()
        st = s.query(scene9, tri_state(scene9, mat9, sky), moved_from=st, n_random=750)     # (twenty instances: the brute force's longest steps)
        # 10. a new pose, three frames enqueued and not awaited, then the queries: the version path beside frames in flight
        scene9.update(0.3)
        r.recalculateScene()
        frames_before = r.stats()["frames"]
        old, st = st, tri_state(scene9, mat9, sky)
        o, d = step_rays(scene9, st, 750)
        for _ in range(3):
            r.enqueue()
        # (the wrapper's query methods write the scene again first, and a write of twenty instances drains: these two go to the
        # library directly, while the frames run -- a current version is found and waited for, no write in between)
        rays, near = pack(o, d), np.zeros(o.shape[0], dtype=abi.HIT_DTYPE)
        abi.check(L.rt_trace_rays_host(r._ctx, rays.ctypes.data, rays.shape[0], near.ctypes.data), r._ctx)
        multi = host_multi(r, rays, 0, 3)
        assert r.stats()["frames"] == frames_before                     # (counted by rt_wait: nothing has drained the three)
        assert check_triangle_hits(oracle, st["tri"], o, d, near) > 100
        with np.errstate(all="ignore"):
            T, I, P, _ = k_smallest(o.shape[0], 3, all_triangle_hits(st["tri"], o, d), F(0.001), F(9999.0))
        bad = (multi["prim"] != P) | (multi["instance"] != I) | (bits(multi["t"]) != bits(T))
        assert not bad.any(), "beside frames in flight the k = 3 lists differ from the brute force on %d rays" % int(bad.any(axis=1).sum())
        st = s.query(scene9, st, moved_from=old, n_random=750)
        r.wait()
        assert np.array_equal(r.read_pixels(), oracle.render_tri(st["params"], st["tri"], sky.faces, W, H)[0])
        # 11. a scene smaller than any before it (fewer triangles, nodes, lookup slots; nodes_used and node_count_max keep their
        #     larger values): before any frame of it -- inst = 1, the copy refused --, and after one
        scene11, mat11 = triangle_scene(seed=103, n_models=1, rings=4, sectors=5)
        assert scene11.node_buffer_length() < min(scene.node_buffer_length(), scene9.node_buffer_length())
        s.replace(scene11, mat11)
        r.recalculateScene()
        st11 = st = s.query(scene11, tri_state(scene11, mat11, sky), moved_from=st)
        r.render()
        s.query(scene11, st)
        # 12. spheres in the same context: scene_kind = 0, c->d_records / c->n; a frame; triangles again, before a frame of them
        sph = rt.synthetic_scene(37, 5)
        s.replace(sph)
        st = s.query(sph, sphere_state(sph, sky), moved_from=st)
        r.render()
        assert np.array_equal(r.read_pixels(), oracle.render(st["params"], st["spheres"], sky.faces, W, H)[0])
        s.query(sph, st)
        s.replace(scene11, mat11)
        s.query(scene11, st11, moved_from=st)
        print("hits per step:", s.hits)
    finally:
        r.close()


def test_sphere_scene_lifecycle(oracle):
    sky = random_sky(22)
    s37 = rt.synthetic_scene(37, 11)
    base = np.asarray(s37.pack_spheres(), F).reshape(-1, 8)
    r = rt.RendererRaytracing(W, H, s37, maxBounces=B).initialize(sky)
    s = Script(oracle, r)
    try:
        # 1. 37 spheres, no frame ever: c->d_records / c->n as rt_write_spheres left them
        r.recalculateScene()
        st = s.query(s37, sphere_state(s37, sky))
        # 2. the same count, every sphere but the ground moved: the new records
        moved = scene_of(drift_spheres(base, 2, 3))
        s.replace(moved)
        st = s.query(moved, sphere_state(moved, sky), moved_from=st)
        # 3. a frame (it prepares its own copies of the records), then the queries
        r.render()
        assert np.array_equal(r.read_pixels(), oracle.render(st["params"], st["spheres"], sky.faces, W, H)[0])
        s.query(moved, st)
        # 4. 1,500 spheres: beyond cap_n -- the records are reallocated -- and more than one staged chunk
        s1500 = rt.synthetic_scene(1500, 12)
        s.replace(s1500)
        st = s.query(s1500, sphere_state(s1500, sky), moved_from=st)
        # 5. five spheres that are no prefix of the 1,500: records 5 .. 1,499 are still in memory and must not be hit
        s5 = rt.synthetic_scene(5, 13)
        assert not np.array_equal(s5.pack_spheres(), s1500.pack_spheres()[:5])
        s.replace(s5)
        st = s.query(s5, sphere_state(s5, sky), moved_from=st)
        # 6. rt_write_spheres(n = 0): every family reports a miss, the shaded query the sky
        s0 = rt.synthetic_scene(0, 1)
        s.replace(s0)
        st = s.query(s0, sphere_state(s0, sky), moved_from=st, empty=True)
        # 7. 37 spheres again; then two frames enqueued and not awaited, and the queries beside them
        s.replace(s37)
        st = s.query(s37, sphere_state(s37, sky), moved_from=st)
        for _ in range(2):
            r.enqueue()
        s.query(s37, st)
        r.wait()
        assert np.array_equal(r.read_pixels(), oracle.render(st["params"], st["spheres"], sky.faces, W, H)[0])
        print("hits per step:", s.hits)
    finally:
        r.close()


def test_device_stream_queries_across_a_scene_change(oracle):
    """The device-memory forms run on the caller's stream and return before they have run.  A scene write after them drains
    (rt_drain waits for ev_query), so queries issued BEFORE a change answer for the old state and queries issued after it, on
    another stream, for the new one -- whatever the streams' timing: values only, one synchronisation at the end."""
    import torch
    sky = random_sky(23)
    scene, mat = triangle_scene(seed=111, n_models=2)
    small, mat_s = triangle_scene(seed=112, n_models=1, rings=4, sectors=5)
    assert len(scene.instances) == 3 and small.node_buffer_length() < scene.node_buffer_length()
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky, mat)
    try:
        r.recalculateScene()
        old = tri_buffers(scene, mat)
        o, d = step_rays(scene, dict(tri=old))
        n = o.shape[0]
        dev = torch.from_numpy(pack(o, d)).to("cuda:0")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            near_old = r.trace_rays(dev)
            multi_old = r.trace_rays_multi(dev, k=3)
        scene.update(0.5)                                   # a pose no query ever sees
        r.recalculateScene()
        r.scene, r.meshMaterial, r.loaded = small, mat_s, False
        r.recalculateScene()                                # the smaller scene: every static buffer rewritten (these writes drain)
        new = tri_buffers(small, mat_s)
        near_new = r.trace_rays(dev)                        # the default stream
        multi_new = r.trace_rays_multi(dev, k=3)
        torch.cuda.synchronize()
        assert not same(oracle.trace_tri_rays(old, o, d), oracle.trace_tri_rays(new, o, d))
        for buf, near, multi in ((old, near_old, multi_old), (new, near_new, multi_new)):
            h = np.ascontiguousarray(near.cpu().numpy()).view(abi.HIT_DTYPE).reshape(n)
            assert check_triangle_hits(oracle, buf, o, d, h) > 100
            m = np.ascontiguousarray(multi.cpu().numpy()).view(abi.HIT_DTYPE).reshape(n, 3)
            check_order(m, F(0.001), F(9999.0))
            with np.errstate(all="ignore"):
                T, I, P, _ = k_smallest(n, 3, all_triangle_hits(buf, o, d), F(0.001), F(9999.0))
            bad = (m["prim"] != P) | (m["instance"] != I) | (bits(m["t"]) != bits(T))
            assert not bad.any(), "the k = 3 lists differ from the brute force on %d rays" % int(bad.any(axis=1).sum())
            assert same(m["t"][:, 0], h["t"])
    finally:
        r.close()
