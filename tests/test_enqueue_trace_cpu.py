"""The host side of a frame without a GPU: every HIP call and kernel launch that rt_api.hip makes for it, in order, held against a
recorded trace.  rt_api.hip holds no device code, so it is compiled with the Makefile's flags plus --cuda-host-only and linked --
without the HIP runtime and without RCCL -- against tests/c/enqueue_trace.cpp, which defines every HIP entry point and every
rt_launch_* function the object leaves undefined (a launch added later fails the link), prints one line per call and drives the
C ABI through every branch of rt_enqueue, rt_render, rt_render_to and rt_wait (DESIGN.md 4.7g lists them).  A missing
hipStreamWaitEvent or a step moved across the slot of the event ring is a race that the bit-exact GPU suites pass almost every
time; here it is a changed line.  tests/golden/enqueue_trace.txt.gz was recorded with this program from the sources as they stood
before rt_enqueue was taken apart into a plan and steps."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import compute_raytracer_amd as rt
from helpers import leafy_scene, tri_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
# the Makefile's HIPFLAGS and rt_api.o's own, for the host side alone
HOST_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
              "--cuda-host-only"]


def write_scene(d):
    """The buffers of the triangle steps, as the renderer would write them (float32, tri_buffers' arrays)."""
    b = tri_buffers(leafy_scene(2), rt.Material.white())
    for name in ("triangles", "nodes", "blas", "tri_lookup", "blas_lookup"):
        np.ascontiguousarray(b[name], dtype=np.float32).tofile(os.path.join(d, name + ".bin"))


def build_trace_program(tmp_path, extra=()):
    objs = []
    for src in (os.path.join(ROOT, "compute_raytracer_amd", "csrc", "rt_api.hip"), os.path.join(ROOT, "tests", "c", "enqueue_trace.cpp")):
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        r = subprocess.run([HIPCC] + HOST_FLAGS + list(extra) + ["-x", "hip", "-c", src, "-o", obj], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(obj)
    exe = str(tmp_path / "enqueue_trace")
    # every symbol the object leaves undefined is the program's to define: no HIP runtime, no RCCL, nothing left unresolved
    r = subprocess.run([os.path.join(ROCM, "llvm", "bin", "clang++")] + list(extra) + objs + ["-o", exe, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_calls_of_a_frame_are_the_recorded_ones(tmp_path):
    exe = build_trace_program(tmp_path)
    write_scene(str(tmp_path))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-2000:])
    got = r.stdout.splitlines()
    # 4,534 lines, kept compressed (gzip -n -9; `zcat` shows them): recorded output is compared, not read
    want = gzip.open(os.path.join(ROOT, "tests", "golden", "enqueue_trace.txt.gz"), "rt").read().splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d, after %s:\nrecorded: %s\nthis tree: %s" % (k + 1, [x for x in got[:k] if x.startswith("#")][-2:], want[max(0, k - 6):k + 3], got[max(0, k - 6):k + 3])
    assert len(got) == len(want)
    assert got[-1] == "# live allocations: 0"
