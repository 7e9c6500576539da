"""The root-free shadow_decided and the ended suspended shadow walks (rt_bvh.hip, claims D and D'), pinned to the CPU oracle
bit for bit -- frame AND ray count, never this library's own output: a lane the comparisons no longer decide walks its shadow
ray, a walk ended at a suspension is counted once, and neither may show.  Frames of 96x64 and a ragged 101x67; scenes of 130
to 9,000 spheres (every hierarchy form: the test asserts the form the host planned), either node test, a flat and a 4x4
textured sky, bounce limits 0, 1, 2 and 9, the light inside a sphere, far above the scene (most first shadow rays are then
settled by the sphere they start from) and below the ground, rank 3 of 8, and four frames in flight with the light moving."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA, synthetic_spheres
from helpers import expected_sphere_form, random_sky
from test_shadow_decided_gpu import first_diff, render_and_compare

pytestmark = pytest.mark.gpu

B = 5
SIZES = [130, 300, 1200, 1900, 3300, 9000]          # 8-wave, 8-wave, 12-wave, 12-wave with short lists, 16-wave, global nodes
FRAMES = [(96, 64), (101, 67)]
CAM = np.array([0.0593, 2.692, 3.293])


def scene_of(n, sgn=None, light=None, seed=7):
    s = synthetic_spheres(n, seed)
    if sgn == 0:                                      # one radius below 2^-30: the host plans the unsigned node test
        s[-1] = rt.Sphere(list(s[-1].center), 2.0 ** -31, list(s[-1].color))
    scene = rt.SceneRaytracing().createScene(s)
    scene.camera.position = list(CAM)
    scene.camera.update()
    if light == "inside":
        scene.light.position = list(np.asarray(s[5].center, float) + s[5].radius * np.array([0.3, -0.2, 0.4]))
    elif light == "far_above":
        scene.light.position = [40.0, 5000.0, -60.0]
    elif light == "below_ground":
        scene.light.position = [1.0, -2.0, -9.0]
    elif light is not None:
        scene.light.position = list(light)
    return scene


def sky_of(tex, seed):
    return random_sky(seed, w=4, h=4) if tex else rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)


FULL = [(n, sgn, tex) for n in SIZES for sgn in (1, 0) for tex in (0, 1)]


@pytest.mark.parametrize("n,sgn,tex", FULL, ids=["n%d-sgn%d-%s" % (n, s, "tex" if t else "flat") for n, s, t in FULL])
def test_sizes_filters_and_skies(oracle, n, sgn, tex):
    scene, sky = scene_of(n, sgn), sky_of(tex, n)
    want = expected_sphere_form(scene, B, sky=sky)
    assert want.sgn == sgn and want.flat == (not tex), want
    render_and_compare(oracle, scene, sky, 96, 64, B, want)


def test_the_sizes_cover_every_form():
    forms = {expected_sphere_form(scene_of(n, 1), B, sky=sky_of(0, 0)).form for n in SIZES}
    assert {"bvh8", "bvh12", "bvh16", "bvh_global"} <= forms, forms


@pytest.mark.parametrize("n", SIZES)
def test_ragged_frame(oracle, n):
    sgn, tex = (SIZES.index(n) + 1) % 2, SIZES.index(n) % 2
    scene, sky = scene_of(n, sgn), sky_of(tex, n + 1)
    render_and_compare(oracle, scene, sky, 101, 67, B, expected_sphere_form(scene, B, sky=sky))


@pytest.mark.parametrize("bounces", [0, 1, 2, 9])
@pytest.mark.parametrize("light", ["inside", "far_above", "below_ground"])
def test_bounce_limits_and_lights(oracle, light, bounces):
    scene, sky = scene_of(300, None, light), sky_of(bounces % 2, 3)
    w, h = FRAMES[bounces % 2]
    render_and_compare(oracle, scene, sky, w, h, bounces, expected_sphere_form(scene, bounces, sky=sky))


@pytest.mark.parametrize("n,light", [(1200, "far_above"), (1900, "inside"), (9000, "below_ground")])
def test_lights_in_the_larger_forms(oracle, n, light):
    scene, sky = scene_of(n, None, light), sky_of(0, 4)
    render_and_compare(oracle, scene, sky, 101, 67, B, expected_sphere_form(scene, B, sky=sky))


@pytest.mark.parametrize("n,sgn", [(300, 1), (1900, 0)])
def test_rank_3_of_8(oracle, n, sgn):
    scene, sky = scene_of(n, sgn), sky_of(sgn, 5)
    render_and_compare(oracle, scene, sky, 101, 192, B, expected_sphere_form(scene, B, sky=sky), rank=3, world=8)


@pytest.mark.parametrize("n,sgn,tex", [(300, 1, 0), (1900, 0, 1)])
def test_four_frames_in_flight_with_the_light_moving(oracle, n, sgn, tex):
    W, H = 101, 67
    scene, sky = scene_of(n, sgn), sky_of(tex, 9)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky)
    try:
        host, refs = r.host_frames(4), []
        for f, light in enumerate([[0.0, 5.0, 0.0], [-14.0, 0.9, -12.0], [40.0, 5000.0, -60.0], [1.0, -2.0, -9.0]]):
            r.scene.light.position = light
            refs.append(oracle.render(r.scene.pack_params(B), r.scene.pack_spheres(), sky.faces, W, H))
            r.recalculateScene()
            r.enqueue()
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
