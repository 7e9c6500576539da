"""Every path of the library that replaces a device allocation, on the MI355X: ONE context walks each of them at least twice --
first where the buffer has to grow, then where it has room -- and after every step a frame or a query result is compared with the
oracle, bit for bit and ray for ray, as the parity tests compare that scene kind (tests/test_parity_gpu.py, test_work_list_gpu.py,
test_ray_query_gpu.py).  A buffer that was freed while something still pointed at it, allocated too small, or not carried over a
reallocation shows as a wrong frame; a context that does not release what it holds shows, at the latest, in the second context of
the same process.  (No assertion on free device memory: the card is shared.)

The paths, by the names in rt_api.hip:  ensure_out (colour buffers) -- rt_write_spheres (cap_n) -- the hierarchy arrays of
rt_enqueue -- ensure_queue (variant 2) -- rt_write_cubemap_face -- ensure_fin (a textured sky over the hierarchy) -- grow_buf
(triangles, lookup table, nodes, corners, pair records, texture) -- the tile-cost and tile-order sets (kOrderMinTiles = 4,096
tiles) -- grow_staging (host queries above the 65,536-byte first size) -- rt_destroy and a second rt_create."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA
from helpers import diff_stats, leafy_scene, random_sky, tri_buffers
from query_common import camera_rays, check_triangle_hits

pytestmark = pytest.mark.gpu
B = 3


def resize(r, W, H):
    abi.check(r._lib.rt_resize(r._ctx, W, H), r._ctx)
    r.width, r.height = W, H


def write_sky(r, sky):
    for i, face in enumerate(sky.faces):
        f = np.ascontiguousarray(face, dtype=np.uint8)
        abi.check(r._lib.rt_write_cubemap_face(r._ctx, i, f.shape[1], f.shape[0], f.ctypes.data), r._ctx)
    r.skyboxMaterial = sky


def replace_scene(r, scene, mat=None):
    """a new scene in the same context: everything is written again by the next recalculateScene()"""
    r.scene, r.meshMaterial, r.loaded = scene, mat, False


class Frames:
    """render() and compare: the oracle's frame of a (scene, sky, size) is computed once and shared by the steps that repeat it"""
    def __init__(self, oracle, r):
        self.oracle, self.r, self.refs, self.steps = oracle, r, {}, 0

    def check(self, what, key, mat=None):
        r, scene, sky = self.r, self.r.scene, self.r.skyboxMaterial
        r.render()
        img, st = r.read_pixels(), r.stats()
        key = (key, r.width, r.height)
        if key not in self.refs:
            p = scene.pack_params(B)
            if scene.hasTriangles:
                ref, _, rays = self.oracle.render_tri(p, tri_buffers(scene, mat), sky.faces, r.width, r.height)
            else:
                ref, _, rays = self.oracle.render(p, scene.pack_spheres(), sky.faces, r.width, r.height)
            self.refs[key] = (ref, rays)
        ref, rays = self.refs[key]
        assert np.array_equal(img, ref), (what, diff_stats(img, ref))
        assert st["rays"] == rays, (what, st["rays"], rays)
        self.steps += 1
        return st


def test_one_context_through_every_reallocating_path(oracle):
    flat = rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)
    spheres = {n: rt.synthetic_scene(n, 40 + n) for n in (8, 200, 100, 400)}
    r = rt.RendererRaytracing(41, 23, spheres[8], maxBounces=B).initialize(flat)
    f = Frames(oracle, r)
    try:
        # ---- colour buffers (ensure_out): grow, shrink (room), grow beyond the largest so far
        for W, H in ((41, 23), (64, 40), (41, 23), (72, 48)):
            resize(r, W, H)
            f.check(("colour", W, H), "s8")
        # ---- spheres at 64 x 40, variant 0: cap_n at 8 -> 200 -> 400, room at 100; the hierarchy arrays at 200 (from 128
        # spheres on) and again at 400, no hierarchy at 100
        resize(r, 64, 40)
        for n, kid in ((8, 2), (200, 4), (100, 2), (400, 4)):
            replace_scene(r, spheres[n])
            st = f.check(("spheres", n), "s%d" % n)
            assert st["spheres"] == n and st["kernel_id"] == kid, st       # trace_pixels<filter> / bvh_pixels<8>
        # ---- the path queue (ensure_queue): variant 2 takes the two-kernel pipeline; first at 64 x 40, then with room
        r.set_variant(2)
        assert f.check("queue", "s400")["kernel_id"] == 3                   # first_bounce + trace_paths
        resize(r, 41, 23)
        assert f.check("queue, room", "s400")["kernel_id"] == 3
        r.set_variant(0)
        resize(r, 64, 40)
        # ---- the sky over the 200-sphere scene (room in cap_n and in the hierarchy arrays): face buffers at 1x1 -> 2x2 -> 4x4,
        # the same size again; the end-of-path records (ensure_fin) at the first textured frame, then with room
        replace_scene(r, spheres[200])
        for k, (w, seed) in enumerate(((2, 1), (4, 2), (4, 3))):
            write_sky(r, random_sky(seed, w, w))
            assert f.check(("sky", w, seed), "s200 sky%d" % k)["kernel_id"] == 4
        resize(r, 72, 48)                                                   # more pixel slots than the records hold
        f.check("sky, larger frame", "s200 sky2")
        resize(r, 64, 40)
        # ---- triangles (grow_buf): a hand-made scene, the same tree over twice the triangles and lookup slots, the first again
        mat = rt.Material(np.random.default_rng(4).integers(0, 256, (8, 8, 4), dtype=np.uint8))
        leafy = {k: leafy_scene(k) for k in (2, 4)}
        assert leafy[4].pack_triangles().shape[0] == 2 * leafy[2].pack_triangles().shape[0]
        for k in (2, 4, 2, 4):
            replace_scene(r, leafy[k], mat)
            assert f.check(("triangles", k), "t%d" % k, mat)["kernel_id"] == 8
        # ---- the work list: 64 x 64 = 4,096 tiles is kOrderMinTiles -- the first awaited frame allocates the stream's tile-cost
        # and tile-order sets, the second renders from the list; 65 x 64 tiles: both grow; 4,096 again: room.  The camera moves
        # with every frame: a tile a list skipped cannot pass on the pixels an earlier frame left in the colour buffer.
        for k, (W, H) in enumerate(((512, 512), (512, 512), (520, 512), (520, 512), (512, 512))):
            resize(r, W, H)
            leafy[4].camera.move(0.03, 0.02)
            f.check(("work list", k, W, H), "t4 step %d" % k, mat)
        resize(r, 64, 40)
        # ---- host queries (grow_staging): 16 rays fit the 65,536-byte first size, 5,000 rays (160,000 bytes) do not; 16 again
        buf = tri_buffers(leafy[4], mat)
        o, d = camera_rays(leafy[4], 100, 50)
        assert o.shape[0] == 5000
        few = np.arange(16) * 311 + 150
        for sel in (few, slice(None), few):
            hits = check_triangle_hits(oracle, buf, o[sel], d[sel], r.trace_rays(o[sel], d[sel]))
            assert hits > (1000 if sel is not few else 2), hits
        f.check("a frame after the queries", "t4 moved", mat)
    finally:
        r.close()
    assert f.steps == 24
    # ---- a second context in the same process, after the first has released everything
    r2 = rt.RendererRaytracing(41, 23, spheres[8], maxBounces=B).initialize(flat)
    try:
        Frames(oracle, r2).check("second context", "s8")
    finally:
        r2.close()
