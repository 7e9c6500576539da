"""The scenes of tests/test_sphere_forms_gpu.py sit in the cells they are meant for, checked without a GPU: the model of the
sphere dispatcher (tests/helpers.py: expected_sphere_form, over the library's own rt_filter_plan and rt_build_hierarchy) puts
each case in its form, with its SGN, FLAT and list capacity, and the count on the other side of the form's nearest LDS
boundary in the next form -- so that no scene drifts out of its cell unnoticed, and no boundary moves without a case on each
side."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from helpers import (CROWDED_CASES, KID_BRUTE_PIPELINE, KID_BRUTE_SINGLE, KID_HIERARCHY_8, KID_LITERAL, SPHERE_CASES, bvh_room, crowded_case,
                     expected_sphere_form, filter_plan, lds_fits, non_cube_sky, random_sky, sky_is_flat,
                     unsigned_ground_spheres, unsigned_tiny_spheres)
from compute_raytracer_amd.scene_raytracing import synthetic_spheres

KIDS = {"literal8": KID_LITERAL, "literal16_w": KID_LITERAL, "literal16": KID_LITERAL, "literal_global": KID_LITERAL,
        "single": KID_BRUTE_SINGLE, "brute_global": KID_BRUTE_SINGLE, "pipe8": KID_BRUTE_PIPELINE, "pipe16": KID_BRUTE_PIPELINE,
        "pipe8_global": KID_BRUTE_PIPELINE, "v2": KID_BRUTE_PIPELINE, "v3": KID_BRUTE_PIPELINE,
        "bvh8": 4, "bvh12": 5, "bvh16": 6, "bvh_global": 7}


@pytest.mark.parametrize("case", SPHERE_CASES, ids=lambda c: c.name)
def test_case_sits_in_its_cell(case):
    scene = case.scene()
    assert len(scene.spheres) == case.n
    f = case.expected(scene=scene)
    assert f is not None and f.form == case.form, f
    assert f.kernel_id == KIDS[case.form]
    if case.cap is not None:
        assert f.cap == case.cap
    ok, sgn = filter_plan(scene, case.B)
    assert ok == (not case.far)
    if case.sgn is not None:
        assert f.sgn == sgn == case.sgn
    assert f.flat == (case.sky_kind == "flat")
    assert f.resolve == (f.form.startswith("bvh") and case.sky_kind != "flat")
    n2, form2 = case.beside[0], case.beside[1]
    g = case.expected(n=n2)
    if form2 is None:
        assert g is None, g
    else:
        assert g is not None and g.form == form2, g
        if len(case.beside) > 2:
            assert g.cap == case.beside[2]


def test_every_instantiation_has_a_case():
    """Each form under both filters and both skies (literal forms: both skies, SGN is no template argument of theirs), both
    unsigned scene builders, a non-cube sky, and the 16-wave literal forms also from a fast-mode frame beyond the filter's range."""
    cells = {(c.form, c.cap, c.sgn, c.sky_kind == "flat") for c in SPHERE_CASES if not c.far}
    for form, cap in (("single", None), ("pipe8", None), ("pipe16", None), ("pipe8_global", None), ("brute_global", None),
                      ("v2", None), ("v3", None), ("bvh8", 12), ("bvh12", 12), ("bvh12", 6), ("bvh16", 12), ("bvh16", 6),
                      ("bvh_global", 8)):
        for sgn in (0, 1):
            for flat in (True, False):
                assert (form, cap, sgn, flat) in cells, (form, cap, sgn, flat)
    for form in ("literal8", "literal16_w", "literal16", "literal_global"):
        for flat in (True, False):
            assert (form, None, None, flat) in cells
    far = {(c.form, c.sky_kind == "flat") for c in SPHERE_CASES if c.far}
    assert far == {("literal16_w", True), ("literal16_w", False), ("literal16", True), ("literal16", False)}
    assert {c.unsigned for c in SPHERE_CASES if c.sgn == 0} == {"ground", "tiny"}
    assert any(c.sky_kind == "noncube" for c in SPHERE_CASES)


def test_unsigned_builders_take_the_unsigned_filter_at_any_size():
    for n in (3, 100, 2000, 5000):
        for build in (unsigned_ground_spheres, unsigned_tiny_spheres):
            scene = rt.SceneRaytracing().createScene(build(n, 3))
            assert filter_plan(scene, 4) == (True, 0), (build.__name__, n)
        assert filter_plan(rt.synthetic_scene(n, 3), 4) == (True, 1)


def test_skies():
    assert sky_is_flat(rt.CubemapMaterial.constant([10, 20, 30, 255]))
    assert not sky_is_flat(random_sky(1)) and not sky_is_flat(non_cube_sky(1))
    assert non_cube_sky(1).faces[0].shape == (5, 6, 4)
    m = rt.CubemapMaterial.constant([10, 20, 30, 255])
    m.faces = [f.copy() for f in m.faces]
    m.faces[3][0, 0, 3] = 7                          # alpha is not part of the library's flat test
    assert sky_is_flat(m)
    m.faces[3][0, 0, 1] = 21
    assert not sky_is_flat(m)


def test_scheduling_thresholds():
    """72 <= N < 128: one frame at a time the single brute-force kernel, once frames are in flight the 8-wave hierarchy; and
    variant 5 stays brute force, strict mode literal, below 320 spheres a single kernel."""
    scene = rt.synthetic_scene(100, 7)
    assert expected_sphere_form(scene, 4).kernel_id == KID_BRUTE_SINGLE
    assert expected_sphere_form(scene, 4, in_flight=True).kernel_id == KID_HIERARCHY_8
    assert expected_sphere_form(rt.synthetic_scene(71, 7), 4, in_flight=True).kernel_id == KID_BRUTE_SINGLE
    assert expected_sphere_form(rt.synthetic_scene(128, 7), 4).kernel_id == KID_HIERARCHY_8
    assert expected_sphere_form(rt.synthetic_scene(319, 7), 4, variant=5).form == "single"
    assert expected_sphere_form(rt.synthetic_scene(320, 7), 4, variant=5).form == "pipe8"
    assert expected_sphere_form(scene, 4, strict=True).form == "literal8"


def test_hierarchy_room_rules():
    """The restated LDS rules agree with their documented edges: lds_fits hands out 1280-byte granules (53,760 bytes fit three
    times, 53,761 do not), and every form's room grows with the node count."""
    assert lds_fits(3, 53760) and not lds_fits(3, 53761)
    for waves, cap in ((8, 12), (12, 12), (12, 6), (16, 12), (16, 6)):
        rooms = [bvh_room(n, waves, cap) for n in range(100, 8000, 37)]
        assert all(a <= b for a, b in zip(rooms, rooms[1:]))


@pytest.mark.parametrize("n,form,cap,sgn,sky", CROWDED_CASES)
def test_crowded_scene_sits_in_its_cell(n, form, cap, sgn, sky):
    scene, s = crowded_case(n, sgn, sky)
    f = expected_sphere_form(scene, 4, sky=s)
    assert (f.form, f.cap, f.sgn, f.flat) == (form, cap, sgn, sky == "flat"), f
