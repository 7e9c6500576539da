"""AddressSanitizer + UndefinedBehaviorSanitizer over the arithmetic and the serial model of device mesh deformation
(compute_raytracer_amd/csrc/rt_deform.h: every word rt_deform_triangles stores, and all of rt_deform_triangles_model), in a
stand-alone program with its own main (tests/c/deform_test.cpp) -- soups and indexed meshes in arrays of exactly the size a call may
touch, indices beyond V, V == 1, ranges at either end of the buffer, NaN / infinite / zero-area input, the call shape."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_deform_model_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "deform_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "deform_test.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "cannot find -lasan" in (r.stderr + r.stdout):
        pytest.skip("libasan not installed")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "deform ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in (r.stdout + r.stderr) and "AddressSanitizer" not in r.stderr
