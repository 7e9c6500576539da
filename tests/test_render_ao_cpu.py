"""Ambient-occlusion frames (include/rt355.h: rt_render_ao, rt_render_ao_host) on a machine without a GPU: the header, the library
and abi.py agree; ao_directions gives what it promises; the basis of the float32 restatement (tests/ao_common.py) is orthonormal to
float32 rounding; render_ao refuses bad arguments before it touches the library; the checks of the C ABI that need no device come in
the header's order; and the radius chosen for the triangle scenes of tests/test_render_ao_gpu.py gives, by the CPU oracle alone,
pixels of every kind."""
import ctypes
import re

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from ao_common import ao_basis, ao_rays, counts_from, cpu_occluded, cpu_primary_hits
from helpers import tri_buffers
from query_common import F, camera_rays
from test_render_samples_cpu import declaration, header_code
from test_render_samples_gpu import TRI

W, H = 41, 23
N = W * H
NEW = ["rt_render_ao", "rt_render_ao_host"]
CTYPE = {"rt_ctx*": ctypes.c_void_p, "const uint32_t*": ctypes.POINTER(ctypes.c_uint32), "const float*": ctypes.POINTER(ctypes.c_float),
         "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "const rt_ao*": ctypes.POINTER(abi.RtAo), "size_t": ctypes.c_size_t,
         "void*": ctypes.c_void_p}

# The triangle scenes whose trees a builder made, the radius of their rays (tmin 0.001, ao_directions(5)), and what the CPU oracle
# alone finds among the 943 pixels: (count == 0, 0 < count < 5, count == 5); the rest are misses (TRI_HITS of test_gbuffer_gpu.py).
CPU_CASES = {"ref": (1.0, (470, 93, 3)), "inst3": (2.0, (549, 14, 0)), "inst13": (1.0, (483, 86, 3)), "inst17": (1.0, (496, 79, 1))}
CPU_K = 5


def cpu_counts(oracle, name):
    """The flat count plane of scene `name` at CPU_K rays and its radius, and the pick-style primary hits, without a device"""
    scene, mat = TRI[name]()
    buf = tri_buffers(scene, mat)
    o, d = camera_rays(scene, W, H)
    h = cpu_primary_hits(oracle, buf, o, d)
    hit, rays = ao_rays(h, o, d, rt.ao_directions(CPU_K), 0.001, CPU_CASES[name][0])
    return counts_from(N, hit, cpu_occluded(oracle, buf, rays.reshape(-1, 8)), CPU_K), h


def test_header_library_and_binding_agree():
    code = header_code()
    lib = abi.load()
    for name in NEW:
        types = declaration(code, name)
        assert name in abi.SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert [CTYPE[t] for t in types] == list(fn.argtypes), name
    host = ["rt_ctx*", "const uint32_t*", "const float*", "uint32_t", "float", "float", "const rt_ao*", "size_t"]
    assert declaration(code, "rt_render_ao_host") == host and declaration(code, "rt_render_ao") == host + ["void*"]
    m = re.search(r"typedef\s+struct\s+rt_ao\s*\{(.*?)\}\s*rt_ao\s*;", code, flags=re.S)
    assert m, "include/rt355.h does not define rt_ao"
    fields = [" ".join(f.replace("*", " * ").split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint8_t * count", "float * ao"]
    assert [f[0] for f in abi.RtAo._fields_] == ["count", "ao"] == list(abi.AO_PLANES)
    assert ctypes.sizeof(abi.RtAo) == 16
    assert re.search(r"#define\s+RT355_MAX_AO_RAYS\s+64u", code) and abi.RT355_MAX_AO_RAYS == 64
    assert lib.rt_abi_version() == 4                     # additive: the ABI version stays


def test_checks_that_need_no_device_come_in_the_headers_order():
    lib = abi.load()
    dirs = rt.ao_directions(4)
    dp = dirs.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    plane = np.zeros((4, 4), F)
    full = abi.RtAo(ao=plane.ctypes.data)
    calls = {"rt_render_ao": lambda c, q, k, o: lib.rt_render_ao(c, None, q, k, 0.001, 1.0, o, 16, None),
             "rt_render_ao_host": lambda c, q, k, o: lib.rt_render_ao_host(c, None, q, k, 0.001, 1.0, o, 16)}
    for name, call in calls.items():
        # k first, whatever else is NULL
        for k in (0, 65, 0xFFFFFFFF):
            for c_dirs, out in ((None, None), (dp, ctypes.byref(full))):
                assert call(None, c_dirs, k, out) == abi.RT_ERR_INVALID_ARG
                assert b"k = " in lib.rt_last_error(None) and name.encode() + b":" in lib.rt_last_error(None)
        # then the context
        for k in (1, 64):
            assert call(None, dp, k, ctypes.byref(full)) == abi.RT_ERR_INVALID_ARG and b"ctx is NULL" in lib.rt_last_error(None)
            assert call(None, None, k, None) == abi.RT_ERR_INVALID_ARG and b"ctx is NULL" in lib.rt_last_error(None)


@pytest.mark.parametrize("k", [1, 5, 16, 64])
def test_ao_directions(k):
    d = rt.ao_directions(k)
    assert d.shape == (k, 3) and d.dtype == np.float32
    assert np.all(d[:, 2] > 0)
    # A unit vector rounded to float32: each component x (1 + e), |e| <= 2^-24, so the squared norm -- summed here in float64, whose
    # own rounding is 2^-29 of that -- is within 2 * 2^-24 + 2^-48 of 1.  2^-22: "a few ulp", with room for the float64 steps.
    n2 = (d.astype(np.float64) ** 2).sum(axis=1)
    assert np.all(np.abs(n2 - 1.0) <= 2.0 ** -22), np.abs(n2 - 1.0).max()
    again = rt.ao_directions(k)
    assert again is not d and np.array_equal(again.view(np.uint32), d.view(np.uint32))
    assert len(np.unique(d, axis=0)) == k


def test_ao_directions_is_the_default_and_rejects_nonsense():
    with pytest.raises(ValueError):
        rt.ao_directions(0)
    assert "ao_directions" in rt.__all__


def unit_normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, -0.0], [0, 1, -0.0]], F)
    near = np.array([[1e-4, 0, -1], [0, 1e-4, -1], [1e-4, 1e-4, 1]], np.float64)          # close to both poles
    near = (near / np.linalg.norm(near, axis=1)[:, None]).astype(F)
    return np.concatenate([axes, near, v])


def test_the_basis_is_orthonormal_to_float32_rounding():
    n = unit_normals(4000, 3)
    assert np.signbit(n[6, 2]) and n[6, 2] == 0                     # n.z = -0 is among them
    T, B = ao_basis(n)
    assert T.dtype == np.float32 and B.dtype == np.float32 and np.all(np.isfinite(T)) and np.all(np.isfinite(B))
    # n.z = -0 takes the branch of +0: s = +1
    assert np.array_equal(T[6].view(np.uint32), ao_basis(np.array([[1, 0, 0.0]], F))[0][0].view(np.uint32))
    # Every entry of T and B is a handful of float32 operations on numbers of magnitude at most 2 (|a| <= 1: s + n.z is at least 1
    # in magnitude), each rounding by at most 2^-24 relative, and n itself is a unit vector only to 2 * 2^-24: a dot product of two
    # of the three vectors, taken in float64, is off by a few dozen 2^-24 at the most.  2^-18 is sixty-four of them.
    tol = 2.0 ** -18
    T64, B64, n64 = T.astype(np.float64), B.astype(np.float64), n.astype(np.float64)
    for a, b, want in ((T64, T64, 1.0), (B64, B64, 1.0), (n64, n64, 1.0), (T64, B64, 0.0), (T64, n64, 0.0), (B64, n64, 0.0)):
        err = np.abs((a * b).sum(axis=1) - want)
        assert np.all(err <= tol), err.max()
    # right-handed: T x B = n
    assert np.all(np.abs(np.cross(T64, B64) - n64) <= tol)


def test_a_nan_normal_gives_nan_rays_and_no_exception():
    hits = {"t": np.array([2.0, 3.0], F), "prim": np.array([0, 4], np.int32), "normal": np.array([[np.nan, 0, 0], [0, 0, np.nan]], F)}
    o, d = np.zeros((2, 3), F), np.array([[0, 0, -1], [0, 1, 0]], F)
    hit, rays = ao_rays(hits, o, d, rt.ao_directions(3), 0.001, 1.0)
    assert list(hit) == [0, 1] and rays.shape == (2, 3, 8)
    assert np.all(np.isnan(rays[:, :, 4:7]))
    assert np.all(np.isfinite(rays[:, :, 0:4])) and np.all(rays[:, :, 7] == 1.0)
    # NaN >= 0 is false: s = -1
    T, _ = ao_basis(np.array([[0.0, 0.0, np.nan]], F))
    assert np.isnan(T[0, 0]) and T[0, 2] == 0


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("render_ao touched the library (%s) before it refused its arguments" % name)


def test_render_ao_rejects_bad_arguments_before_touching_the_library():
    r = object.__new__(rt.RendererRaytracing)
    r.width, r.height, r.device = W, H, 0
    r._lib, r._ctx = _Untouchable(), None
    r.recalculateScene = lambda: (_ for _ in ()).throw(AssertionError("render_ao wrote the scene before it refused its arguments"))
    for planes in ((), ("depth",), ("ao", "ao"), ("count", "normal"), "both"):
        with pytest.raises(ValueError):
            r.render_ao(planes=planes)
    for rect in ((0, 0, 1), (-1, 0, 1, 1), (0, 0, 1 << 32, 1)):
        with pytest.raises(ValueError):
            r.render_ao(rect=rect)
    for dirs in (np.zeros((0, 3), F), np.zeros((65, 3), F), np.zeros((4, 2), F), np.zeros(3, F), np.zeros((2, 2, 3), F)):
        with pytest.raises(ValueError):
            r.render_ao(dirs)
    for k in (0, 65):
        with pytest.raises(ValueError):
            r.render_ao(k=k)
    for out in ({}, {"depth": None}, []):
        with pytest.raises(ValueError):
            r.render_ao(out=out)


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_the_chosen_radius_gives_pixels_of_every_kind(oracle, name):
    """What tests/test_render_ao_gpu.py relies on, shown here by the CPU alone: at the scene's radius there are pixels with no
    occluded ray, pixels with some and not all, and misses."""
    count, h = cpu_counts(oracle, name)
    hit = h["prim"] >= 0
    kinds = (int((count[hit] == 0).sum()), int(((count[hit] > 0) & (count[hit] < CPU_K)).sum()), int((count[hit] == CPU_K).sum()))
    assert kinds == CPU_CASES[name][1], kinds
    assert kinds[0] > 0 and kinds[1] > 0 and 0 < int(hit.sum()) < N
    assert np.all(count[~hit] == 0)
