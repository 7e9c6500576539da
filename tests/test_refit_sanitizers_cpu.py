"""AddressSanitizer + UndefinedBehaviorSanitizer over the host walk of the BLAS refit (compute_raytracer_amd/csrc/rt_refit_plan.h:
what rt_refit_blas validates before it launches anything, and all of rt_refit_plan), in a stand-alone program with its own main
(tests/c/refit_plan_test.cpp) -- builder trees, the bad trees of tests/refit_common.py, a spine of 100,000 levels, garbage."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_refit_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "refit_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "refit_plan_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "cannot find -lasan" in (r.stderr + r.stdout):
        pytest.skip("libasan not installed")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "refit plan ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in (r.stdout + r.stderr) and "AddressSanitizer" not in r.stderr
