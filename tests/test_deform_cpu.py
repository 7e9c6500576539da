"""Device mesh deformation (include/rt355.h: rt_deform_triangles, rt_deform_triangles_host, rt_deform_triangles_model,
rt_update_triangles_device, rt_read_triangles) on a machine without a GPU: the serial model -- the same inline arithmetic as the
kernel (csrc/rt_deform.h) -- against a numpy float32 restatement of the deformed record, bit for bit; the call shape, check by
check in the documented order; and the model against the packer, on the two deformations of tests/refit_common.py."""
import ctypes

import numpy as np
import pytest

from compute_raytracer_amd import abi
from deform_common import F, FLAT, NAN_PAYLOAD, NRM_WORDS, all_cases, bits, check_records, indexed, mesh_vertices, model, numpy_deform
from refit_common import deform, mesh_ranges, view_scene

T = 300
CASES = all_cases(T)


def base_records(seed=5, n=T):
    """records whose every word is distinct noise: a word written by mistake, or left by mistake, shows"""
    return np.random.default_rng(seed).standard_normal((n, 40)).astype(F)


@pytest.mark.parametrize("name,first,n,case", CASES, ids=[c[0] for c in CASES])
def test_the_model_is_the_numpy_restatement(name, first, n, case):
    before = base_records()
    rc, got = model(before, first, n, **case)
    assert rc == abi.RT_OK, abi.load().rt_last_error(None)
    check_records(name, got, before, first, n, case)
    assert not np.array_equal(bits(got[first:first + n]), bits(before[first:first + n]))


def test_the_cases_hold_what_they_are_for():
    """the clamp, repeated indices, a zero-area triangle, a NaN with a payload and an infinity are in the inputs and show in the
    outputs"""
    shapes = {(first, n) for _, first, n, _ in CASES}
    assert {n for _, n in shapes} >= {1, 64, 65, 257} and any(first + n == T for first, n in shapes) and any(first > 0 for first, _ in shapes)
    before = base_records()
    for name, first, n, case in CASES:
        v, f = case["vertices"], case["faces"]
        if f is not None:
            assert (f >= v.shape[0]).any() and (f == 0xFFFFFFFF).any() and (n <= 2 or len(set(f[0])) == 1), name
        got = model(before, first, n, **case)[1][first:first + n]
        assert (bits(got[:, [1, 13, 25]]) == NAN_PAYLOAD).any(), name                     # the NaN vertex arrived, payload kept
        assert np.isinf(got[:, [2, 14, 26]]).any(), name
        if n > 2 and case["flags"] & FLAT:
            assert np.isnan(got[1, NRM_WORDS]).all(), name                                 # 0 / 0: no guard
            ok = np.isfinite(got[:, NRM_WORDS]).all(axis=1)
            lens = np.sqrt((got[ok][:, [4, 5, 6]].astype(np.float64) ** 2).sum(axis=1))
            assert ok.sum() >= n // 2 and np.abs(lens - 1.0).max() < 1e-6, name
    one = [c for c in CASES if c[0] == "V 1"][0]
    got = model(before, one[1], one[2], **one[3])[1][one[1]:one[1] + one[2]]
    assert all(np.array_equal(bits(got[:, 12 * c:12 * c + 3]), np.broadcast_to(bits(one[3]["vertices"][0]), (one[2], 3))) for c in range(3))


def test_flat_normals_follow_the_winding():
    """one triangle by hand: counter-clockwise in the xy plane looks along +z; the other winding along -z"""
    tri = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], F)
    before = base_records(n=2)
    got = model(before, 1, 1, tri, flags=FLAT)[1]
    assert np.array_equal(got[1, NRM_WORDS].reshape(3, 3), np.broadcast_to(np.array([0, 0, 1], F), (3, 3)))
    got = model(before, 1, 1, tri[[0, 2, 1]], flags=FLAT)[1]
    assert np.array_equal(got[1, NRM_WORDS].reshape(3, 3), np.broadcast_to(np.array([0, 0, -1], F), (3, 3)))
    assert np.array_equal(bits(got[0]), bits(before[0]))


def test_call_shape_of_the_model():
    """every check of include/rt355.h, in its order: each call below fails the named check and would fail a later one too"""
    inv, state, ok = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_STATE, abi.RT_OK
    L = abi.load()
    t = base_records(n=10)
    v = np.zeros((30, 3), F)
    nr = np.zeros((30, 3), F)
    f = np.zeros((10, 3), np.uint32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(tri=t, n_tri=10, first=0, n=10, vertices=v, V=30, faces=None, normals=None, flags=0):
        before = t.copy()
        rc = L.rt_deform_triangles_model(P(tri), n_tri, first, n, P(vertices), V, P(faces), P(normals), flags)
        if rc != ok:
            assert np.array_equal(bits(t), bits(before)) and b"rt_deform_triangles_model" in L.rt_last_error(None)
        return rc

    # 1. flags, before anything else
    assert call(flags=2, tri=None) == inv and call(flags=0x80000000) == inv and call(flags=FLAT | 4) == inv
    assert call(flags=FLAT, normals=nr, tri=None) == inv
    # 2. no triangles
    assert call(tri=None, first=11) == state and call(n_tri=0, first=11) == state
    # 3. the range, in 64 bits, before n == 0 and before the arrays
    assert call(first=1, vertices=None) == inv and call(first=11, n=0) == inv and call(first=0xFFFFFFFF, n=2, vertices=None) == inv
    assert call(first=0xFFFFFFFF, n=0xFFFFFFFF) == inv
    # 4. n == 0: nothing else is looked at
    assert call(first=10, n=0, vertices=None, V=0) == ok and call(first=0, n=0) == ok
    # 5. the arrays
    assert call(vertices=None) == inv and call(V=0) == inv and call(V=29) == inv
    assert call(V=1, faces=f) == ok and call(V=29, faces=f) == ok and call(V=30) == ok and call(first=9, n=1, V=3) == ok
    assert call(flags=FLAT) == ok and call(normals=nr) == ok


def test_call_shape_without_a_context():
    """the context entry points: a NULL context is the first check of each"""
    L = abi.load()
    inv = abi.RT_ERR_INVALID_ARG
    v = np.zeros((3, 3), F)
    p = ctypes.c_void_p(v.ctypes.data)
    for name in ("rt_deform_triangles", "rt_deform_triangles_host", "rt_deform_triangles_model", "rt_update_triangles_device", "rt_read_triangles"):
        assert name in abi.SYMBOLS and hasattr(L, name)
    assert L.rt_deform_triangles(None, 0, 1, p, 3, None, None, 0, None) == inv and b"rt_deform_triangles: ctx is NULL" in L.rt_last_error(None)
    assert L.rt_deform_triangles(None, 0, 0, None, 0, None, None, 0, None) == inv
    assert L.rt_deform_triangles_host(None, 0, 1, p, 3, None, None, 0) == inv and b"rt_deform_triangles_host: ctx is NULL" in L.rt_last_error(None)
    assert L.rt_update_triangles_device(None, 0, 1, p, None) == inv and b"rt_update_triangles_device" in L.rt_last_error(None)
    assert L.rt_read_triangles(None, 0, 1, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == inv and b"rt_read_triangles" in L.rt_last_error(None)
    assert abi.RT_DEFORM_FLAT_NORMALS == 1 and L.rt_abi_version() == 4


@pytest.mark.parametrize("kind", ["grow", "shrink"])
def test_the_model_gives_the_packers_records(kind):
    """The corners refit_common.deform() gives a mesh, handed over as vertex arrays -- as the (T, 3, 3) soup and through an index
    table --, leave exactly the records deform() makes of the packed scene (SoupMesh.pack's layout, everything but the corners
    kept); with the mesh's own normals handed back, too."""
    scene, _ = view_scene()
    tris = np.ascontiguousarray(scene.pack_triangles(), F)
    for root, first, count in mesh_ranges(scene)[0:2]:
        want = deform(tris, first, count, kind)
        corners = mesh_vertices(tris, first, count, kind)
        rc, got = model(tris, first, count, corners)
        assert rc == abi.RT_OK and np.array_equal(bits(got), bits(want))
        verts, faces = indexed(corners)
        assert verts.shape[0] < 3 * count                                   # the mesh shares vertices
        rc, got = model(tris, first, count, verts, faces)
        assert rc == abi.RT_OK and np.array_equal(bits(got), bits(want))
        smooth = np.stack([tris[first:first + count, 12 * c + 4:12 * c + 7] for c in range(3)], axis=1)
        rc, got = model(tris, first, count, corners, normals=smooth)
        assert rc == abi.RT_OK and np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(numpy_deform(tris, first, count, corners)), bits(want))
