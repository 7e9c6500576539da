"""AddressSanitizer + UndefinedBehaviorSanitizer over the host side of the closest-point queries (compute_raytracer_amd/csrc/
rt_closest.h: the leaf function, the per-instance constants, the bounds, the walk and all of rt_closest_points_model), in a
stand-alone program with its own main (tests/c/closest_test.cpp): the seed-3 scene's buffers with the records the numpy brute force
expects, hand-made trees deeper than the stacks, indices beyond every array, garbage floats, the bad arguments."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from closest_common import F, brute, make_points, mixed_radii
from helpers import tri_buffers, triangle_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_scene_file(path, buf, points, want):
    arrays = [np.ascontiguousarray(buf[k], F).reshape(-1) for k in ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")]
    counts = np.array([points.shape[0], arrays[0].size // 40, arrays[1].size, arrays[2].size // 8, arrays[3].size // 20, arrays[4].size],
                      np.uint32)
    with open(path, "wb") as f:
        f.write(counts.tobytes())
        f.write(np.ascontiguousarray(points, F).tobytes())
        for a in arrays:
            f.write(a.tobytes())
        f.write(np.ascontiguousarray(want).tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_closest_model_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "closest_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "c", "closest_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "cannot find -lasan" in (r.stderr + r.stdout):
        pytest.skip("libasan not installed")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    scene, mat = triangle_scene(seed=3, n_models=5)
    buf = tri_buffers(scene, mat)
    points = mixed_radii(make_points(buf, 200, 21), 22)
    path = str(tmp_path / "seed3.bin")
    write_scene_file(path, buf, points, brute(buf, points))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "closest ok" in r.stdout and "scene file: 200 points" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in (r.stdout + r.stderr) and "AddressSanitizer" not in r.stderr
