"""Ray queries (include/rt355.h: rt_trace_rays, rt_trace_rays_host, rt_pick) on a machine without a GPU: the header declares
them, the library exports them, the rt_hit record has the header's layout in C and in the ctypes mirror, and the entry points
reject what they must reject before they need a device."""
import ctypes
import os
import re
import subprocess

import numpy as np

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_SYMBOLS = ["rt_trace_rays", "rt_trace_rays_host", "rt_pick"]
FIELDS = ["t", "u", "v", "prim", "instance", "normal"]


def test_header_declares_and_library_exports_the_query_entry_points():
    text = open(os.path.join(ROOT, "include", "rt355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = abi.load()
    for name in QUERY_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/rt355.h does not declare %s" % name
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert re.search(r"typedef\s+struct\s+rt_hit\s*\{", code)
    assert lib.rt_abi_version() == 4                     # additive: the ABI version stays


def test_rt_hit_layout_matches_the_header(tmp_path):
    """sizeof(rt_hit) == 32 and every field's offset, as a C compiler lays the header's struct out, equals the ctypes mirror's and
    the numpy record's."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt355.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rt_hit));\n' +
                   "".join('    printf(" %%zu", offsetof(rt_hit, %s));\n' % f for f in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size == 32 == ctypes.sizeof(abi.RtHit) == np.dtype(abi.HIT_DTYPE).itemsize
    assert offsets == [getattr(abi.RtHit, f).offset for f in FIELDS] == [np.dtype(abi.HIT_DTYPE).fields[f][1] for f in FIELDS]
    assert offsets == [0, 4, 8, 12, 16, 20]


def test_null_context_and_pointers_are_rejected():
    lib = abi.load()
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros(4, dtype=abi.HIT_DTYPE)
    xy = np.zeros((4, 2), np.uint32)
    assert lib.rt_trace_rays(None, rays.ctypes.data, 4, hits.ctypes.data, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays(None, None, 0, None, None) == abi.RT_ERR_INVALID_ARG     # the context is checked first
    assert lib.rt_trace_rays_host(None, rays.ctypes.data, 4, hits.ctypes.data) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays_host(None, None, 4, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_pick(None, xy.ctypes.data, 4, hits.ctypes.data) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_pick(None, None, 1, None) == abi.RT_ERR_INVALID_ARG
    assert b"NULL" in lib.rt_last_error(None)


def test_queries_have_no_cpu_path():
    """Without a device there is no context to query: rt_create fails and the renderer's initialize() raises, whatever the
    scene; an ordinal beyond the devices fails on any machine."""
    import torch
    lib = abi.load()
    ctx = ctypes.c_void_p()
    assert lib.rt_create(1 << 20, ctypes.byref(ctx)) == abi.RT_ERR_NO_DEVICE and not ctx.value
    if torch.cuda.is_available():
        return
    assert lib.rt_create(0, ctypes.byref(ctx)) == abi.RT_ERR_NO_DEVICE and not ctx.value
    r = rt.RendererRaytracing(16, 16, rt.synthetic_scene(3, 1))
    try:
        r.initialize()
    except abi.RtError as e:
        assert e.code == abi.RT_ERR_NO_DEVICE
    else:
        raise AssertionError("initialize() succeeded without a device")
