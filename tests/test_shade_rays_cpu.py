"""Shaded ray queries (include/rt355.h: rt_shade_rays, rt_shade_rays_host, RT_SHADE_COMPOSE) on a machine without a GPU: the
header declares them with the signatures abi.py binds, the library exports them, rt_shade has the header's layout in C and in the
ctypes / numpy mirrors, the argument checks that need no device refuse what they must -- and the method the triangle tests of
tests/test_shade_rays_gpu.py rest on, proved on the sphere oracle where both sides exist."""
import ctypes
import os
import re
import subprocess

import numpy as np

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import random_sky
from shade_common import F, OracleRays, compose_np, same, settled_unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_shade_rays", "rt_shade_rays_host"]
FIELDS = ["r", "g", "b", "dist"]
# C parameter types -> the ctypes abi.py must bind them with
CTYPE = {"rt_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "rt_shade*": ctypes.c_void_p,
         "void*": ctypes.c_void_p}


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


def test_header_library_and_binding_agree(tmp_path):
    code = header_code()
    lib = abi.load()
    for name in NEW:
        types = declaration(code, name)
        assert name in abi.SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert [CTYPE[t] for t in types] == list(fn.argtypes), name
    assert declaration(code, "rt_shade_rays") == ["rt_ctx*", "const float*", "uint32_t", "uint32_t", "rt_shade*", "void*"]
    assert declaration(code, "rt_shade_rays_host") == ["rt_ctx*", "const float*", "uint32_t", "uint32_t", "rt_shade*"]
    m = re.search(r"#define\s+RT_SHADE_COMPOSE\s+(\w+)", code)
    assert m and int(m.group(1).rstrip("uU"), 0) == 1 == abi.RT_SHADE_COMPOSE
    assert lib.rt_abi_version() == 4                     # additive: the ABI version stays
    # sizeof(rt_shade) == 16 and every field's offset, as a C compiler lays the header's struct out
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt355.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rt_shade));\n' +
                   "".join('    printf(" %%zu", offsetof(rt_shade, %s));\n' % f for f in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size == 16 == ctypes.sizeof(abi.RtShade) == np.dtype(abi.SHADE_DTYPE).itemsize
    assert offsets == [getattr(abi.RtShade, f).offset for f in FIELDS] == [np.dtype(abi.SHADE_DTYPE).fields[f][1] for f in FIELDS]
    assert offsets == [0, 4, 8, 12]


def test_null_context_pointers_and_unknown_flags_are_rejected():
    lib = abi.load()
    rays = np.zeros((4, 8), F)
    out = np.zeros(4, dtype=abi.SHADE_DTYPE)
    calls = {
        "rt_shade_rays": lambda f, r, o, n=4: lib.rt_shade_rays(None, r, n, f, o, None),
        "rt_shade_rays_host": lambda f, r, o, n=4: lib.rt_shade_rays_host(None, r, n, f, o),
    }
    for name, call in calls.items():
        for flags in (0, abi.RT_SHADE_COMPOSE):
            assert call(flags, rays.ctypes.data, out.ctypes.data) == abi.RT_ERR_INVALID_ARG
            assert b"NULL" in lib.rt_last_error(None) and name.encode() in lib.rt_last_error(None)
            assert call(flags, None, out.ctypes.data) == abi.RT_ERR_INVALID_ARG
            assert call(flags, rays.ctypes.data, None) == abi.RT_ERR_INVALID_ARG
            # n == 0 with NULL pointers: the context is looked at before n, as in query_device
            assert call(flags, None, None, 0) == abi.RT_ERR_INVALID_ARG
            assert b"ctx" in lib.rt_last_error(None)
        # unknown bits are refused before anything else is looked at, n == 0 included
        for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
            for n in (4, 0):
                assert call(flags, rays.ctypes.data, out.ctypes.data, n) == abi.RT_ERR_INVALID_ARG
                assert b"flag" in lib.rt_last_error(None), (name, flags)


def test_a_one_pixel_oracle_frame_is_the_compose_of_ray_color(oracle):
    """What the triangle tests compare composed results with: the oracle's frame of ONE pixel whose camera sits at the ray's origin
    and looks along its direction (cameraPos = origin, forwards = d, right = up = 0).  Pixel (0, 0) of a 1x1 frame has hc = -1 and
    vc = 1, so its direction is normalize((d + -1 * 0) + 1 * 0) = normalize(d) -- d itself for a d that normalisation leaves as it
    is (settled_unit: one normalisation alone does not always give one; rays without such a d are left out), given components that
    are not zero (no signed zero enters).  On the sphere oracle both sides exist: oracle.pixel of that camera must be, bit for bit, pixelColor (RK:91-96)
    restated in numpy float32 over oracle.ray_color(origin, d) and oracle.cube_sample(d)."""
    scene = rt.synthetic_scene(37, 11)
    sky = random_sky(5)
    params = np.asarray(scene.pack_params(3), F)
    sp = np.asarray(scene.pack_spheres(), F).reshape(-1, 8)
    rng = np.random.default_rng(21)
    n = 220
    o = (params[0:3] + rng.uniform(-6.0, 6.0, (n, 3))).astype(F)
    o[:, 1] = np.abs(o[:, 1]) + F(0.5)                       # above the ground sphere
    target = sp[rng.integers(0, sp.shape[0], n), 0:3] + rng.normal(scale=1.5, size=(n, 3))
    d, ok = settled_unit((target - o).astype(F))
    o, d = o[ok], d[ok]
    n = o.shape[0]
    assert n >= 180 and np.all(d != 0) and np.all(o != 0)
    orc = OracleRays(oracle, params, sp, sky.faces)
    rgbd, cnt = orc.ray_color(o, d)
    want = compose_np(rgbd, orc.sky(d), params[20])
    got = np.zeros((n, 3), F)
    for i in range(n):
        p = params.copy()
        p[0:3], p[4:7] = o[i], d[i]
        p[8:11] = 0.0
        p[12:15] = 0.0
        got[i], rays = oracle.pixel(p, sp, sky.faces, 1, 1, 0, 0)
        assert rays == cnt[i]
    assert same(got, want), "%d of %d one-pixel frames differ from the restated compose" % (
        int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()), n)
    # the rays do exercise the compose: paths that hit and paths that miss, fog factors inside (0, 1)
    assert (rgbd[:, 3] > 0).sum() >= 50 and (rgbd[:, 3] == 0).sum() >= 10
    assert not same(want, rgbd[:, 0:3])
