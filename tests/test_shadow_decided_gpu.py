"""Shadow rays settled without a traversal (rt_bvh.hip, claim D: shadow_decided), pinned to the CPU oracle bit for bit --
frame AND ray count (the counter counts the reference's rays, settled ones included) -- in every hierarchy form (8, 12 and
16 waves with 12- and 6-entry lists, global nodes), under the signed and the unsigned node test and under a flat and a
textured sky, over scenes built to put shaded points at the predicate's edge: a low light (long terminators), spheres of
radius 0.002 to 0.02 in front of the camera, the light inside, on and far from spheres, coincident spheres, a huge ground
sphere, scenes moved 2^10 and 2^19 from the origin, zero radii; a NaN radius hands the frame to the literal kernel.  Then
bounce limits 0 to 9, rank 3 of 8, and frames in flight whose parameters differ from frame to frame."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA, synthetic_spheres
from helpers import diff_stats, expected_sphere_form, oracle_render, random_sky

pytestmark = pytest.mark.gpu

W, H, B = 96, 64, 5
# a sphere count inside each hierarchy form's range (tests/test_sphere_forms_cpu.py has the edges: 1184 / 1789 / 2106 / 4338 / 4724
# for synthetic_spheres; the scene classes below change the node count by a few per cent, the test asserts the form it got)
FORMS = {"bvh8-cap12": 1100, "bvh12-cap12": 1650, "bvh12-cap6": 1950, "bvh16-cap12": 3300, "bvh16-cap6": 4530, "bvh_global-cap8": 5200}
# scene class -> the node tests it can be rendered under (1 signed, 0 unsigned; a compact scene becomes unsigned by one radius below 2^-30)
CLASSES = {"low_light": (1, 0), "small_radii": (1, 0), "light_inside": (1, 0), "light_on_surface": (1, 0), "coincident": (1, 0),
           "light_far": (0,), "huge_ground": (0,), "offset_2^10": (0,), "offset_2^19": (0,), "zero_radii": (1, 0)}


def first_diff(img, ref):
    d = np.argwhere(np.any(img != ref, axis=-1))
    return None if d.size == 0 else (tuple(int(v) for v in d[0]), img[tuple(d[0])].tolist(), ref[tuple(d[0])].tolist())


def build_scene(kind, n, sgn, seed=7):
    rng = np.random.default_rng(seed)
    s = synthetic_spheres(n, seed)
    cam = np.array([0.0593, 2.692, 3.293])
    light = np.array([0.0, 5.0, 0.0])
    off = np.zeros(3)
    if kind == "low_light":
        light = np.array([-14.0, 0.9, -12.0])                    # beside the scene, below most sphere tops
    elif kind == "small_radii":                                   # a swarm of tiny spheres a few pixels wide just in front of the camera
        fw = np.array([0.0, -0.276, -0.961])
        for i in range(1, 161):
            p = cam + fw * rng.uniform(0.12, 0.6) + rng.normal(size=3) * 0.05
            s[i] = rt.Sphere(p, float(10 ** rng.uniform(np.log10(0.002), np.log10(0.02))), rng.uniform(0.2, 1.0, 3))
        light = cam + np.array([0.1, 0.4, -0.3])
    elif kind == "light_inside":
        c, r = np.asarray(s[5].center, float), s[5].radius
        light = c + r * np.array([0.3, -0.2, 0.4])
    elif kind == "light_on_surface":
        c, r = np.asarray(s[9].center, float), s[9].radius
        light = c + r * np.array([0.0, 1.0, 0.0])
    elif kind == "coincident":
        for i in range(1, 120):
            s[120 + i] = rt.Sphere(list(s[i].center), s[i].radius * (1.0 if i % 2 else 1.0 + 1e-6), list(s[120 + i].color))
    elif kind == "light_far":
        light = np.array([3000.0, 8000.0, -2000.0])
    elif kind == "huge_ground":
        s[0] = rt.Sphere([0.0, -1.0e4, 0.0], 1.0e4, [0.8, 0.8, 0.8])
    elif kind.startswith("offset_2^"):
        big = 2.0 ** int(kind.split("^")[1])
        off = np.array([big, -0.5 * big, 0.25 * big])
        s = [rt.Sphere(off + np.asarray(x.center, float), x.radius, list(x.color)) for x in s]
    elif kind == "zero_radii":
        for i in range(3, n, 5):
            s[i] = rt.Sphere(list(s[i].center), 0.0, list(s[i].color))
    else:
        raise KeyError(kind)
    if sgn == 0 and 1 in CLASSES[kind]:
        s[-1] = rt.Sphere(list(s[-1].center), 2.0 ** -31, list(s[-1].color))
    scene = rt.SceneRaytracing().createScene(s)
    scene.camera.position = list(off + cam)
    scene.camera.update()
    scene.light.position = list(off + light)
    return scene


def sky_of(tex, seed):
    return random_sky(seed) if tex else rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)


def render_and_compare(oracle, scene, sky, w, h, bounces, want, **part):
    ref, _, rays = oracle_render(oracle, scene, w, h, bounces, skybox=sky,
                                 **({"tile_first": part["rank"], "tile_step": part["world"]} if part else {}))
    r = rt.RendererRaytracing(w, h, scene, maxBounces=bounces, **part).initialize(sky)
    try:
        r.render()
        img, st = r.read_pixels(), r.stats()
    finally:
        r.close()
    if part:
        ref = ref[[y for y in range(h) if (y // 8) % part["world"] == part["rank"]]]
    assert st["kernel_id"] == want.kernel_id, want
    assert np.array_equal(img, ref), (want, first_diff(img, ref), diff_stats(img, ref))
    assert st["rays"] == rays, (want, st["rays"], rays)


CASES = [(form, kind, sgn, tex) for form in FORMS for kind, sgns in CLASSES.items() for sgn in sgns for tex in (0, 1)]


@pytest.mark.parametrize("form,kind,sgn,tex", CASES, ids=["%s-%s-sgn%d-%s" % (f, k, s, "tex" if t else "flat") for f, k, s, t in CASES])
def test_every_form_filter_sky_and_scene_class(oracle, form, kind, sgn, tex):
    n = FORMS[form]
    scene, sky = build_scene(kind, n, sgn), sky_of(tex, n)
    want = expected_sphere_form(scene, B, sky=sky)
    assert "%s-cap%d" % (want.form, want.cap) == form and want.sgn == sgn and want.flat == (not tex), want
    render_and_compare(oracle, scene, sky, W, H, B, want)


@pytest.mark.parametrize("n", [FORMS["bvh8-cap12"], FORMS["bvh16-cap12"]])
def test_nan_radius_goes_to_the_literal_kernel(oracle, n):
    s = synthetic_spheres(n, 7)
    for i in range(4, n, 97):
        s[i] = rt.Sphere(list(s[i].center), float("nan"), list(s[i].color))
    scene = rt.SceneRaytracing().createScene(s)
    sky = sky_of(0, 0)
    want = expected_sphere_form(scene, B, sky=sky)
    assert want.form.startswith("literal"), want
    render_and_compare(oracle, scene, sky, W, H, B, want)


@pytest.mark.parametrize("bounces", range(10))
@pytest.mark.parametrize("kind,sgn", [("low_light", 1), ("small_radii", 0)])
def test_bounce_limits(oracle, kind, sgn, bounces):
    scene, sky = build_scene(kind, 1024, sgn), sky_of(bounces % 2, 3)
    render_and_compare(oracle, scene, sky, 157, 91, bounces, expected_sphere_form(scene, bounces, sky=sky))


@pytest.mark.parametrize("form,sgn", [("bvh8-cap12", 1), ("bvh12-cap6", 0), ("bvh16-cap12", 1)])
def test_rank_3_of_8(oracle, form, sgn):
    scene, sky = build_scene("low_light", FORMS[form], sgn), sky_of(sgn, 5)
    render_and_compare(oracle, scene, sky, 160, 192, B, expected_sphere_form(scene, B, sky=sky), rank=3, world=8)


@pytest.mark.parametrize("sgn,tex", [(1, 0), (0, 1)])
def test_frames_in_flight_with_different_parameters(oracle, sgn, tex):
    """Eight frames enqueued without a wait; camera, light and minIntensity change from frame to frame."""
    scene, sky = build_scene("low_light", 1024, sgn), sky_of(tex, 9)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(sky)
    try:
        for batch in range(2):
            host, refs = r.host_frames(4), []
            for f in range(4):
                r.scene.camera.move(0.05, -0.03 * f)
                r.scene.light.position = [-14.0 + 3.0 * f + batch, 0.9 + 0.7 * f, -12.0 + f]
                r.scene.light.minIntensity = 0.1 + 0.1 * f
                refs.append(oracle.render(r.scene.pack_params(B), r.scene.pack_spheres(), sky.faces, W, H))
                r.recalculateScene()
                r.enqueue()
            for f in range(4):
                r.read_pixels_async(3 - f, host[f])
            r.wait()
            r.read_pixels_wait()
            st = r.stats()
            for f in range(4):
                assert np.array_equal(host[f], refs[f][0]), (batch, f, first_diff(host[f], refs[f][0]))
            assert st["rays"] == refs[-1][2]
            assert st["kernel_id"] == expected_sphere_form(r.scene, B, sky=sky, in_flight=True).kernel_id
    finally:
        r.close()
