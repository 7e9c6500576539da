"""Every sphere kernel form, pinned to the CPU oracle bit for bit: the four literal forms (strict mode, and the 16-wave ones
for fast-mode frames beyond the filter's range), the brute-force forms of rt_kernels.hip (single kernel, the three pipeline
pairs, the global-memory form, variants 2 and 3) and the hierarchy forms of rt_bvh.hip (8, 12 and 16 waves with 12- and
6-entry lists, global nodes), each under the signed and the unsigned filter and under a flat and a textured sky, at the
counts where each form's LDS runs out (tests/test_sphere_forms_cpu.py shows each scene in its cell).  Then the paths that
change a form's schedule -- frames in flight, a rank of a partition -- and the variants that cannot take a scene: refused
before anything of the frame is enqueued, the context still renders."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.scene_raytracing import synthetic_spheres
from helpers import (CROWDED_CASES, KID_BRUTE_SINGLE, KID_HIERARCHY_8, SPHERE_CASES, crowded_case, diff_stats,
                     expected_sphere_form, oracle_render, unsigned_ground_spheres)

pytestmark = pytest.mark.gpu


def first_diff(img, ref):
    d = np.argwhere(np.any(img != ref, axis=-1))
    return None if d.size == 0 else (tuple(int(v) for v in d[0]), img[tuple(d[0])].tolist(), ref[tuple(d[0])].tolist())


@pytest.mark.parametrize("case", SPHERE_CASES, ids=lambda c: c.name)
def test_form_is_the_oracles(oracle, case):
    scene, sky = case.scene(), case.sky()
    want = expected_sphere_form(scene, case.B, case.strict, case.variant, sky)
    ref, _, rays = oracle_render(oracle, scene, case.W, case.H, case.B, skybox=sky)
    r = rt.RendererRaytracing(case.W, case.H, scene, maxBounces=case.B).initialize(sky)
    try:
        r.set_mode(case.strict)
        r.set_variant(case.variant)
        r.render()
        img, st = r.read_pixels(), r.stats()
    finally:
        r.close()
    assert st["kernel_id"] == want.kernel_id, (case.name, want)
    assert np.array_equal(img, ref), (case.name, want, first_diff(img, ref), diff_stats(img, ref))
    assert st["rays"] == rays


@pytest.mark.parametrize("n,form,cap,sgn,sky", CROWDED_CASES)
def test_crowded_scene_fills_the_lists(oracle, n, form, cap, sgn, sky):
    """Every primary ray crosses dozens of overlapping spheres: the 12- and 16-wave forms' candidate lists fill to their last
    row (six or twelve entries per lane) and drain again."""
    W, H, B = 160, 96, 4
    scene, s = crowded_case(n, sgn, sky)
    want = expected_sphere_form(scene, B, sky=s)
    ref, _, rays = oracle_render(oracle, scene, W, H, B, skybox=s)
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize(s)
    try:
        r.render()
        img, st = r.read_pixels(), r.stats()
    finally:
        r.close()
    assert st["kernel_id"] == want.kernel_id, want
    assert np.array_equal(img, ref), (want, first_diff(img, ref), diff_stats(img, ref))
    assert st["rays"] == rays


def _batch(r, oracle, moves, B):
    """Enqueues one frame per camera step without waiting, reads each back through the streaming read-back, returns
    [(frame, oracle frame, oracle rays)]."""
    host = r.host_frames(len(moves))
    refs = []
    for f, (fw, rt_) in enumerate(moves):
        r.scene.camera.move(fw, rt_)
        refs.append(oracle.render(r.scene.pack_params(B), r.scene.pack_spheres(), r.skyboxMaterial.faces, r.width, r.height))
        r.recalculateScene()
        r.enqueue()
    for f in range(len(moves)):
        r.read_pixels_async(len(moves) - 1 - f, host[f])
    r.wait()
    r.read_pixels_wait()
    return [(host[f], refs[f][0], refs[f][2]) for f in range(len(moves))]


def test_pipelined_hint_moves_a_small_scene_to_the_hierarchy(oracle):
    """100 spheres: an awaited frame, and the first batch in flight, take the single brute-force kernel; once the library has
    seen that batch in flight (pipelined_hint) the next batch takes the 8-wave hierarchy on a quarter of the chip each."""
    W, H, B = 157, 91, 4
    scene = rt.SceneRaytracing().createScene(synthetic_spheres(100, 7))
    assert expected_sphere_form(scene, B).kernel_id == KID_BRUTE_SINGLE
    assert expected_sphere_form(scene, B, in_flight=True).kernel_id == KID_HIERARCHY_8
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize()
    try:
        ref, _, rays = oracle_render(oracle, scene, W, H, B)
        r.render()
        assert np.array_equal(r.read_pixels(), ref) and r.stats()["rays"] == rays
        assert r.stats()["kernel_id"] == KID_BRUTE_SINGLE
        for batch, kid in ((0, KID_BRUTE_SINGLE), (1, KID_HIERARCHY_8)):
            out = _batch(r, oracle, [(0.05 * (batch + 1), -0.02 * f) for f in range(4)], B)
            st = r.stats()
            assert st["kernel_id"] == kid, batch
            for f, (img, ref, _) in enumerate(out):
                assert np.array_equal(img, ref), (batch, f, first_diff(img, ref))
            assert st["rays"] == out[-1][2]
        assert st["grid_share"] == 4
    finally:
        r.close()


def test_large_hierarchy_form_in_flight(oracle):
    """The 16-wave form with 12-entry lists, four frames in flight (grid_share 4: a quarter of the chip's workgroups each),
    unsigned filter, textured sky (sky_resolve behind every frame)."""
    case = next(c for c in SPHERE_CASES if c.name == "bvh16-cap12-sgn0-noncube")
    scene, sky = case.scene(), case.sky()
    r = rt.RendererRaytracing(case.W, case.H, scene, maxBounces=case.B).initialize(sky)
    try:
        for batch in range(2):
            out = _batch(r, oracle, [(0.04, 0.03 * f) for f in range(4)], case.B)
            for f, (img, ref, _) in enumerate(out):
                assert np.array_equal(img, ref), (batch, f, first_diff(img, ref))
            st = r.stats()
            assert st["kernel_id"] == case.expected(scene=scene).kernel_id and st["rays"] == out[-1][2]
        assert st["grid_share"] == 4
    finally:
        r.close()


@pytest.mark.parametrize("sgn", [1, 0])
def test_hierarchy_form_as_rank_3_of_8(oracle, sgn):
    """The 12-wave form with 6-entry lists as rank 3 of 8: awaited, then frames in flight, where a share this small walks with
    the small-share tail (launch_bvh_as: 12 lanes); each frame is the oracle's rows of that rank."""
    W, H, B, rank, world = 160, 192, 4, 3, 8
    spheres = (synthetic_spheres if sgn else unsigned_ground_spheres)(2106, 7)
    scene = rt.SceneRaytracing().createScene(spheres)
    want = expected_sphere_form(scene, B)
    assert (want.form, want.cap, want.sgn) == ("bvh12", 6, sgn)
    rows = [y for y in range(H) if (y // 8) % world == rank]
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B, rank=rank, world=world).initialize()
    try:
        for step in range(6):                     # one awaited frame, then a batch of four, then a batch of one
            r.scene.camera.move(0.05, 0.02)
            ref, _, rays = oracle_render(oracle, r.scene, W, H, B, tile_first=rank, tile_step=world)
            r.recalculateScene()
            r.enqueue()
            if step in (0, 4, 5):
                img = r.read_pixels()
                st = r.stats()
                assert st["kernel_id"] == want.kernel_id
                assert np.array_equal(img, ref[rows]), (step, first_diff(img, ref[rows]))
                assert st["rays"] == rays
    finally:
        r.close()


@pytest.mark.parametrize("variant,n", [(1, 2177), (2, 3265), (3, 3265)])
def test_variant_that_cannot_take_the_scene_is_refused(oracle, variant, n):
    """A brute-force variant none of whose forms holds the scene in LDS: rt_render fails with RT_ERR_UNSUPPORTED and names
    the cause before it enqueues anything; the frames in flight before it complete and are counted, the stats keep the last
    frame's form, and the context renders the next frame of another variant as the oracle does."""
    W, H, B = 160, 96, 3
    scene = rt.synthetic_scene(n, 7)
    assert expected_sphere_form(scene, B, variant=variant) is None
    r = rt.RendererRaytracing(W, H, scene, maxBounces=B).initialize()
    try:
        r.render()                                               # variant 0: the hierarchy
        kid = r.stats()["kernel_id"]
        assert kid == expected_sphere_form(scene, B).kernel_id
        r.scene.camera.move(0.1, 0.0)
        ref, _, rays = oracle_render(oracle, r.scene, W, H, B)
        r.recalculateScene()
        r.enqueue(); r.enqueue()                                 # two frames in flight
        r.set_variant(variant)
        with pytest.raises(abi.RtError) as e:
            r.enqueue()
        assert e.value.code == abi.RT_ERR_UNSUPPORTED
        assert ("variant %d" % variant) in str(e.value) and ("%d spheres" % n) in str(e.value)
        r.wait()
        st = r.stats()
        assert st["frames"] == 3 and st["kernel_id"] == kid and st["rays"] == rays
        assert np.array_equal(r.read_pixels(), ref)
        with pytest.raises(abi.RtError):                         # an awaited frame is refused alike
            r.render()
        assert r.stats()["frames"] == 3
        r.set_variant(0)
        r.scene.camera.move(0.1, 0.05)
        ref, _, rays = oracle_render(oracle, r.scene, W, H, B)
        r.render()
        st = r.stats()
        assert np.array_equal(r.read_pixels(), ref) and st["rays"] == rays and st["frames"] == 4 and st["kernel_id"] == kid
    finally:
        r.close()
