"""Primary directions made once per 8x8 tile by all 64 lanes and handed to the lanes that take the tile's pixels (rt_bvh.hip:
tile_dir), pinned to the CPU oracle bit for bit -- frame AND ray count, never this library's own output.  A direction read
from the wrong slot, from a tile the cursor has left, or from the frame before shows as a wrong pixel.  Frames of 96x64, a
ragged 101x67, 13x11 (every tile ragged) and 8x8 (one tile); scenes of 130 to 9,000 spheres (every hierarchy form: the test
asserts the form the host planned), either node test, a flat and a 4x4 textured sky, bounce limits 0, 1 and 5, rank 3 of 8,
four frames in flight with the camera turning between them, a frame with one pixel whose direction is NaN (the flat sky's fog
colour travels with the path as one bit), and one 3840x2160 frame that is mostly sky -- the only shape in which a wave's
reservations grow past one tile -- compared in every 27th tile row (there the ray count is the whole frame's and is not compared)."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA, synthetic_spheres
from helpers import expected_sphere_form, oracle_render, random_sky
from test_shadow_decided_gpu import first_diff, render_and_compare

pytestmark = pytest.mark.gpu

B = 5
SIZES = [130, 1200, 1900, 3300, 9000]               # 8-wave, 12-wave, 12-wave with short lists, 16-wave, global nodes
FRAMES = [(96, 64), (101, 67), (13, 11), (8, 8)]
CAM = np.array([0.0593, 2.692, 3.293])


def scene_of(n, sgn=None, seed=7):
    s = synthetic_spheres(n, seed)
    if sgn == 0:                                      # one radius below 2^-30: the host plans the unsigned node test
        s[-1] = rt.Sphere(list(s[-1].center), 2.0 ** -31, list(s[-1].color))
    scene = rt.SceneRaytracing().createScene(s)
    scene.camera.position = list(CAM)
    scene.camera.update()
    return scene


def sky_of(tex, seed):
    return random_sky(seed, w=4, h=4) if tex else rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)


FULL = [(n, sgn, tex) for n in SIZES for sgn in (1, 0) for tex in (0, 1)]


@pytest.mark.parametrize("n,sgn,tex", FULL, ids=["n%d-sgn%d-%s" % (n, s, "tex" if t else "flat") for n, s, t in FULL])
def test_sizes_filters_and_skies(oracle, n, sgn, tex):
    scene, sky = scene_of(n, sgn), sky_of(tex, n)
    want = expected_sphere_form(scene, B, sky=sky)
    assert want.sgn == sgn and want.flat == (not tex), want
    render_and_compare(oracle, scene, sky, 101, 67, B, want)


def test_the_sizes_cover_every_form():
    forms = {(f.form, f.cap) for f in (expected_sphere_form(scene_of(n, 1), B, sky=sky_of(0, 0)) for n in SIZES)}
    assert forms == {("bvh8", 12), ("bvh12", 12), ("bvh12", 6), ("bvh16", 12), ("bvh_global", 8)}, forms


@pytest.mark.parametrize("w,h", [f for f in FRAMES if f != (101, 67)])
@pytest.mark.parametrize("n", SIZES)
def test_frame_shapes(oracle, n, w, h):
    sgn, tex = (SIZES.index(n) + w) % 2, (SIZES.index(n) + h // 8) % 2
    scene, sky = scene_of(n, sgn), sky_of(tex, n + w)
    render_and_compare(oracle, scene, sky, w, h, B, expected_sphere_form(scene, B, sky=sky))


@pytest.mark.parametrize("tex", [0, 1])
@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("n", [130, 3300])
def test_bounce_limits(oracle, n, bounces, tex):
    scene, sky = scene_of(n, (bounces + tex) % 2), sky_of(tex, 3)
    w, h = FRAMES[(bounces + 1) % 2]
    render_and_compare(oracle, scene, sky, w, h, bounces, expected_sphere_form(scene, bounces, sky=sky))


@pytest.mark.parametrize("n,sgn", [(130, 1), (1900, 0)])
def test_rank_3_of_8(oracle, n, sgn):
    scene, sky = scene_of(n, sgn), sky_of(sgn, 5)
    render_and_compare(oracle, scene, sky, 101, 192, B, expected_sphere_form(scene, B, sky=sky), rank=3, world=8)


@pytest.mark.parametrize("n,sgn,tex", [(130, 1, 0), (1900, 0, 1)])
def test_four_frames_in_flight_with_the_camera_turning(oracle, n, sgn, tex):
    W, H = 101, 67
    scene, sky = scene_of(n, sgn), sky_of(tex, 9)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky)
    try:
        host, refs = r.host_frames(4), []
        for f, (dx, dy) in enumerate([(0.0, 0.0), (23.0, -7.0), (-61.0, 11.0), (140.0, 3.0)]):
            r.scene.camera.spin(dx, dy)
            params = r.scene.pack_params(B)
            assert f == 0 or not np.array_equal(params, last), "the camera did not turn"
            last = params
            refs.append(oracle.render(params, r.scene.pack_spheres(), sky.faces, W, H))
            r.recalculateScene()
            r.enqueue()
        assert len({ref[0].tobytes() for ref in refs}) == 4, "the four frames are not four different pictures"
        for f in range(4):
            r.read_pixels_async(3 - f, host[f])
        r.wait()
        r.read_pixels_wait()
        st = r.stats()
        for f in range(4):
            assert np.array_equal(host[f], refs[f][0]), (f, first_diff(host[f], refs[f][0]))
        assert st["rays"] == refs[-1][2]
    finally:
        r.close()


@pytest.mark.parametrize("bounces", [0, 5])
def test_one_pixel_whose_direction_is_nan(oracle, bounces):
    """A flat sky's fog colour travels with the path as one bit: is the sample along the primary direction NaN?  With forwards = 0
    and an axis-aligned frame the pixel (48, 32) of a 96x64 frame has the direction 0 / |0|, and only that pixel."""
    scene, sky = scene_of(130, 1), sky_of(0, 0)
    scene.camera.forwards = np.zeros(3, np.float32)
    scene.camera.right = np.array([1, 0, 0], np.float32)
    scene.camera.up = np.array([0, 1, 0], np.float32)
    ref = oracle_render(oracle, scene, 96, 64, bounces, skybox=sky)[0]
    assert ref[32, 48].tolist() == [0, 0, 0, 255] and ref[32, 47].tolist() != [0, 0, 0, 255] and ref[31, 48].tolist() != [0, 0, 0, 255]
    render_and_compare(oracle, scene, sky, 96, 64, bounces, expected_sphere_form(scene, bounces, sky=sky))


def test_a_4k_frame_of_mostly_sky(oracle):
    """Cheap pixels: waves use up a reservation within two trips and double the next one, up to several tiles per atomic, so the
    cursor crosses tile edges inside a reservation.  The whole frame is rendered; every 27th tile row (ten of 270) is compared."""
    W, H, K, RANK = 3840, 2160, 27, 5
    scene, sky = scene_of(130, 1), sky_of(0, 0)
    scene.camera.position = list(CAM - 30.0 * np.asarray(scene.camera.forwards, float))      # the scene shrinks to the middle of the frame
    want = expected_sphere_form(scene, 1, sky=sky)
    ref, _, _ = oracle_render(oracle, scene, W, H, 1, skybox=sky, tile_first=RANK, tile_step=K)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=1).initialize(sky)
    try:
        r.render()
        img, st = r.read_pixels(), r.stats()
    finally:
        r.close()
    assert st["kernel_id"] == want.kernel_id, want
    rows = [y for y in range(H) if (y // 8) % K == RANK]
    img, ref = img[rows], ref[rows]
    sky_px = np.all(ref == ref[0, 0], axis=-1).mean()
    assert 0.5 < sky_px < 0.999, sky_px                    # mostly sky, and not only sky
    assert np.array_equal(img, ref), first_diff(img, ref)
