"""The owners of a context's HIP resources without a GPU: compute_raytracer_amd/csrc/rt_own.h is host-only and includes nothing of
the project, so tests/c/own_test.cpp compiles it alone, under g++, against stand-ins for the eight HIP entry points it calls
(malloc behind them, calls and live objects counted per kind, allocations above a limit refused).  The program prints one line
per case; here every line is held against the expectation written out.  made / released: calls since the previous line of that
kind; live: objects of that kind alive."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def buffer_lines(kind):
    """DevBuf and PinnedBuf alike: (case, made, released, live, p, cap, err)"""
    rows = [
        ("replace empty", 1, 0, 1, 1, 100, 0),           # one allocation, nothing to free
        ("replace larger", 1, 1, 1, 1, 1000, 0),         # one allocation, one free
        ("replace smaller", 1, 1, 1, 1, 10, 0),          # exactly what was asked for, never "large enough already"
        ("replace refused", 1, 1, 0, 0, 0, 1),           # the old block freed once, the buffer empty, the error returned
        ("replace after refusal", 1, 0, 1, 1, 7, 0),     # ... and nothing freed twice
        ("reset", 0, 1, 0, 0, 0, 0),
        ("reset again", 0, 0, 0, 0, 0, 0),
        ("scope exit", 0, 0, 0, 0, 0, 0),                # an empty buffer frees nothing
        ("move construct", 1, 0, 1, 1, 100, 0),
        ("moved from", 0, 0, 1, 0, 0, 0),
        ("target made", 1, 0, 2, 1, 200, 0),
        ("move assign", 0, 1, 1, 1, 100, 0),             # the overwritten block freed once
        ("moved from", 0, 0, 1, 0, 0, 0),
        ("scope exit", 0, 1, 0, 0, 0, 0),                # one block left, freed once: the moved-from objects free nothing
        ("arrays made", 8, 0, 8, 1, 128, 0),
        ("array move assign", 0, 4, 4, 1, 128, 0),
        ("moved from", 0, 0, 4, 0, 0, 0),
        ("scope exit", 0, 4, 0, 0, 0, 0),
    ]
    return ["%s %s: made=%d released=%d live=%d p=%d cap=%d err=%d" % ((kind,) + r) for r in rows]


def handle_lines(kind, flags):
    """Event and Stream alike: (case, made, released, live, h, flags of the last one made, err)"""
    rows = [
        ("fresh", 0, 0, 0, 0, 0, 0),
        ("ensure", 1, 0, 1, 1, flags, 0),
        ("ensure again", 0, 0, 1, 1, flags, 0),          # created once; the same handle
        ("converts", 0, 0, 1, 1, flags, 0),              # to the raw handle
        ("move construct", 0, 0, 1, 1, flags, 0),
        ("moved from", 0, 0, 1, 0, flags, 0),
        ("move assign", 1, 1, 1, 1, 0, 0),               # the target's own (default flags) destroyed once
        ("moved from", 0, 0, 1, 0, 0, 0),
        ("ensure refused", 1, 0, 1, 0, flags, 1),        # stays empty
        ("scope exit", 0, 1, 0, 0, flags, 0),
        ("array move assign", 8, 4, 4, 1, flags, 0),
        ("scope exit", 0, 4, 0, 0, flags, 0),
    ]
    return ["%s %s: made=%d released=%d live=%d h=%d flags=%d err=%d" % ((kind,) + r) for r in rows]


def test_the_owners_release_once_and_only_what_they_hold(tmp_path):
    exe = str(tmp_path / "own_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                        os.path.join(ROOT, "tests", "c", "own_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr          # (the program's static_asserts: none of the four types is copyable)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = buffer_lines("DevBuf") + buffer_lines("PinnedBuf") + handle_lines("Event", 2) + handle_lines("Stream", 1) + [      # hipEventDisableTiming, hipStreamNonBlocking
        "used: moved=48 from=0 replaced=0 refused=0 as=1",
        "live: dev=0 pinned=0 events=0 streams=0",
    ]
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want) == 62
