"""AddressSanitizer + UndefinedBehaviorSanitizer over the host model of the device top-level build (compute_raytracer_amd/csrc/
rt_tlas_build.h: the arithmetic the kernel calls, the argument checks of rt_build_tlas and all of rt_build_tlas_host, and
rt_blas_build.h's serial SAH driver under it), in a stand-alone program with its own main (tests/c/tlas_build_test.cpp) --
builder-sized instance sets, coincident instances, singular matrices, a spine deeper than twenty levels, the bad arguments, a
capacity one node short, garbage floats."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tlas_build_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tlas_build_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "c", "tlas_build_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "cannot find -lasan" in (r.stderr + r.stdout):
        pytest.skip("libasan not installed")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "tlas build ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in (r.stdout + r.stderr) and "AddressSanitizer" not in r.stderr
