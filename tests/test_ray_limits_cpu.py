"""Bounded and occlusion ray queries (include/rt355.h: RT_QUERY_LIMITS, rt_trace_rays_ex, rt_trace_rays_host_ex, rt_occluded,
rt_occluded_host) on a machine without a GPU: the header declares them with the signatures abi.py binds, the library exports
them, and the argument checks that need no device refuse what they must."""
import ctypes
import os
import re

import numpy as np

from compute_raytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_trace_rays_ex", "rt_trace_rays_host_ex", "rt_occluded", "rt_occluded_host"]
# C parameter types -> the ctypes abi.py must bind them with
CTYPE = {"rt_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "rt_hit*": ctypes.c_void_p,
         "uint8_t*": ctypes.c_void_p, "void*": ctypes.c_void_p}


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt355.h")).read(), flags=re.S)


def declaration(code, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, "include/rt355.h does not declare %s" % name
    types = []
    for p in m.group(1).split(","):
        words = p.replace("*", " * ").split()
        types.append(" ".join(words[:-1]).replace(" *", "*"))     # drop the parameter's name
    return types


def test_header_declares_and_library_exports_the_new_entry_points():
    code = header_code()
    lib = abi.load()
    for name in NEW:
        declaration(code, name)
        assert name in abi.SYMBOLS and hasattr(lib, name)
    m = re.search(r"#define\s+RT_QUERY_LIMITS\s+(\w+)", code)
    assert m and int(m.group(1).rstrip("uU"), 0) == 1 == abi.RT_QUERY_LIMITS
    assert lib.rt_abi_version() == 4                     # additive: the ABI version stays


def test_abi_signatures_match_the_header():
    code = header_code()
    lib = abi.load()
    for name in NEW:
        types = declaration(code, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert [CTYPE[t] for t in types] == list(fn.argtypes), name
    # the device forms take the stream last; the flags come right after n everywhere
    assert declaration(code, "rt_occluded")[-2:] == ["uint8_t*", "void*"]
    assert declaration(code, "rt_trace_rays_ex")[2:5] == ["uint32_t", "uint32_t", "rt_hit*"]


def test_null_context_pointers_and_unknown_flags_are_rejected():
    lib = abi.load()
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros(4, dtype=abi.HIT_DTYPE)
    occ = np.zeros(4, np.uint8)
    L = abi.RT_QUERY_LIMITS
    calls = {
        "rt_trace_rays_ex": lambda f, r, o: lib.rt_trace_rays_ex(None, r, 4, f, o, None),
        "rt_trace_rays_host_ex": lambda f, r, o: lib.rt_trace_rays_host_ex(None, r, 4, f, o),
        "rt_occluded": lambda f, r, o: lib.rt_occluded(None, r, 4, f, o, None),
        "rt_occluded_host": lambda f, r, o: lib.rt_occluded_host(None, r, 4, f, o),
    }
    for name, call in calls.items():
        out = occ.ctypes.data if "occluded" in name else hits.ctypes.data
        for flags in (0, L):
            assert call(flags, rays.ctypes.data, out) == abi.RT_ERR_INVALID_ARG
            assert b"NULL" in lib.rt_last_error(None) and name.encode() in lib.rt_last_error(None)
            assert call(flags, None, None) == abi.RT_ERR_INVALID_ARG
        # unknown bits are refused before anything else is looked at
        for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
            assert call(flags, rays.ctypes.data, out) == abi.RT_ERR_INVALID_ARG
            assert b"flag" in lib.rt_last_error(None), (name, flags)
    # n == 0 with unknown bits: still refused
    assert lib.rt_occluded_host(None, None, 0, 4, None) == abi.RT_ERR_INVALID_ARG


def test_ray_packing_puts_the_limits_in_words_3_and_7():
    import compute_raytracer_amd as rt
    o = np.arange(12, dtype=np.float32).reshape(4, 3)
    d = -o - 1.0
    rays = rt.RendererRaytracing._pack_rays(o, d, 0.25, np.array([1, 2, 3, 4], np.float32))
    assert rays.shape == (4, 8) and rays.dtype == np.float32
    assert np.array_equal(rays[:, 0:3], o) and np.array_equal(rays[:, 4:7], d)
    assert np.all(rays[:, 3] == np.float32(0.25)) and np.array_equal(rays[:, 7], [1, 2, 3, 4])
    for bad in (np.zeros(3), np.zeros((4, 1))):
        try:
            rt.RendererRaytracing._pack_rays(o, d, bad, 1.0)
        except ValueError:
            pass
        else:
            raise AssertionError("a limit of shape %s was accepted" % (bad.shape,))
