"""Frames through the OPTIMISED sphere hierarchy (rt_bvh_build.h: Builder::optimise) against the oracle, bit for bit, in the
three forms that keep the nodes in LDS (8-, 12- and 16-wave workgroups): the reinsertion pass regroups spheres, the walk only
selects candidates, so no pixel and no ray count may change.  Scenes are random (not the benchmark's seeds) and each is
checked to be one the pass actually changed."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from compute_raytracer_amd.scene_raytracing import synthetic_spheres
from helpers import diff_stats, expected_sphere_form, gpu_render, oracle_render
from test_hierarchy_opt_cpu import abi_passes, build_ex

pytestmark = pytest.mark.gpu
BVH = 4


def moves_of(scene):
    """reinsertions kept by the build the renderer runs (RT355_HIERARCHY_PASSES passes)"""
    rec = np.ascontiguousarray(scene.pack_spheres(), np.float32).reshape(-1, 8)
    return int(build_ex(rec, abi_passes())[3][1])


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    spheres = [rt.Sphere([0.0, -100.0, 0.0], 100.0, [0.8, 0.8, 0.8])]
    spheres += [rt.Sphere([rng.normal() * 5.0, 0.2 + abs(rng.normal()) * 2.0, -12.0 + rng.normal() * 5.0], float(rng.uniform(0.05, 0.5)),
                          rng.uniform(0.2, 1.0, 3)) for _ in range(n - 1)]
    return spheres


@pytest.mark.parametrize("n,seed,kernel,kind", [(300, 901, "hierarchy_8", "synthetic"), (700, 902, "hierarchy_8", "cloud"),
                                                (1450, 903, "hierarchy_12", "synthetic"), (1300, 904, "hierarchy_12", "cloud"),
                                                (3000, 905, "hierarchy_16", "synthetic"), (2600, 906, "hierarchy_16", "cloud")])
def test_optimised_hierarchy_frames_are_the_oracles(oracle, n, seed, kernel, kind):
    scene = rt.SceneRaytracing().createScene(synthetic_spheres(n, seed) if kind == "synthetic" else cloud(n, seed))
    W, H, B = 168, 104, 5
    assert moves_of(scene) > 0                                     # the pass changed this scene's tree
    assert abi.KERNEL_IDS[expected_sphere_form(scene, B, variant=BVH).kernel_id] == kernel
    ref, _, rays = oracle_render(oracle, scene, W, H, B)
    img, st = gpu_render(scene, W, H, B, strict=False, variant=BVH)
    assert np.array_equal(img, ref), diff_stats(img, ref)
    assert st["rays"] == rays
    assert abi.KERNEL_IDS[st["kernel_id"]] == kernel
