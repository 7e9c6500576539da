"""Shared by the device mesh deformation tests (test infrastructure; tests/test_deform_cpu.py, tests/test_deform_gpu.py):
rt_deform_triangles_model through the C ABI, the deformed record restated in numpy float32 (include/rt355.h: rt_deform_triangles;
csrc/rt_deform.h is the definition), the argument combinations and shapes both suites run, and the vertex arrays of
refit_common's two deformations."""
import ctypes

import numpy as np

from compute_raytracer_amd import abi
from refit_common import CORNER_COLS, deform

F = np.float32
FLAT = abi.RT_DEFORM_FLAT_NORMALS
POS_WORDS = [12 * c + k for c in range(3) for k in range(3)]
NRM_WORDS = [12 * c + 4 + k for c in range(3) for k in range(3)]
NAN_PAYLOAD = 0x7FC01234                             # a NaN that only a bit-for-bit copy keeps


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """equal bits, or a NaN in both (a NaN the arithmetic makes -- 0 / 0 of a zero-area triangle -- has no promised sign or payload)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def prepared(vertices, faces, normals):
    """the arrays as the C ABI takes them: float32 (V, 3), uint32 (n, 3), float32 (V, 3)"""
    v = None if vertices is None else np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = None if faces is None else np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nr = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
    return v, f, nr


def model(triangles, first, n, vertices, faces=None, normals=None, flags=0, V=None):
    """rt_deform_triangles_model on a copy of `triangles` -> (status, (T, 40) float32)"""
    L = abi.load()
    t = np.array(triangles, F).reshape(-1, 40).copy()
    v, f, nr = prepared(vertices, faces, normals)
    V = (0 if v is None else v.shape[0]) if V is None else V
    rc = L.rt_deform_triangles_model(_ptr(t), t.shape[0], int(first), int(n), _ptr(v), V, _ptr(f), _ptr(nr), int(flags))
    return rc, t


def numpy_deform(triangles, first, n, vertices, faces=None, normals=None, flags=0):
    """The records after the call, restated: gathers through the clamped indices, positions and caller normals copied as bits,
    flat normals in float32 with one rounding per operation in the order of include/rt355.h."""
    t = np.array(triangles, F).reshape(-1, 40).copy()
    v, f, nr = prepared(vertices, faces, normals)
    V = v.shape[0]
    k = np.arange(3 * n, dtype=np.int64).reshape(n, 3) if f is None else np.minimum(f[:n].astype(np.int64), V - 1)
    rec = bits(t)                                    # a view: stores of bits
    p = v[k]                                         # (n, 3 corners, 3)
    for c in range(3):
        rec[first:first + n, 12 * c:12 * c + 3] = bits(p[:, c])
        if nr is not None:
            rec[first:first + n, 12 * c + 4:12 * c + 7] = bits(nr[k[:, c]])
    if flags & FLAT:
        with np.errstate(all="ignore"):
            e1, e2 = (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F)
            x = (e1[:, 1] * e2[:, 2]).astype(F) - (e1[:, 2] * e2[:, 1]).astype(F)
            y = (e1[:, 2] * e2[:, 0]).astype(F) - (e1[:, 0] * e2[:, 2]).astype(F)
            z = (e1[:, 0] * e2[:, 1]).astype(F) - (e1[:, 1] * e2[:, 0]).astype(F)
            ln = np.sqrt(((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)
            nrm = np.stack([x / ln, y / ln, z / ln], axis=1).astype(F)
        for c in range(3):
            t[first:first + n, 12 * c + 4:12 * c + 7] = nrm
    return t


# ---- the argument combinations and shapes: (first, n) inside T triangles, faces or none, normals absent / given / flat ----
def shapes(T):
    """n = 1, 64, 65 and 257 (where T allows): a range at the start, ranges with first > 0, one ending at the last triangle"""
    out = [(0, 1), (3, 64), (T - 65, 65)]
    if T >= 258:
        out.append((1, 257))
    return [(first, n) for first, n in out if first >= 0]


MODES = ("none", "given", "flat")


def make_case(seed, n, use_faces, mode, V=None):
    """-> dict(vertices, faces, normals, flags) for a call over n triangles.  With faces: V about n / 2 shared vertices, repeated
    indices, indices >= V (0xFFFFFFFF among them) for the clamp; always one zero-area triangle (where n > 2), one NaN vertex with
    a payload and one infinite one."""
    rng = np.random.default_rng(seed)
    if use_faces:
        V = max(1, n // 2 + 3) if V is None else V
        faces = rng.integers(0, V, (n, 3)).astype(np.uint32)
        faces[0] = [min(1, V - 1)] * 3                               # one vertex three times
        faces[n - 1, 2] = V + 5                                      # beyond V: reads vertex V - 1
        faces[n // 2, 0] = 0xFFFFFFFF
        if n > 2:
            faces[1] = [0, 0, min(2, V - 1)]                         # zero area
    else:
        V = 3 * n + 2 if V is None else V                            # two vertices more than the call reads
        faces = None
    vertices = rng.uniform(-3, 3, (V, 3)).astype(F)
    if not use_faces and n > 2:
        vertices[4] = vertices[3]                                    # triangle 1: zero area
    last = V - 1 if use_faces else 3 * n - 1                         # the last vertex the call reads (with faces: through the clamp)
    vertices[last // 2, 2] = np.inf
    bits(vertices)[last, 1] = NAN_PAYLOAD
    if use_faces:
        faces[n // 2, 1] = last // 2
    normals = rng.uniform(-1, 1, (V, 3)).astype(F) if mode == "given" else None
    if normals is not None:
        bits(normals)[0, 0] = NAN_PAYLOAD
    return dict(vertices=vertices, faces=faces, normals=normals, flags=FLAT if mode == "flat" else 0)


def all_cases(T):
    """[(name, first, n, case)] -- every shape with every argument combination"""
    out = []
    for si, (first, n) in enumerate(shapes(T)):
        for use_faces in (False, True):
            for mi, mode in enumerate(MODES):
                name = "first %d n %d %s %s" % (first, n, "faces" if use_faces else "soup", mode)
                out.append((name, first, n, make_case(1000 + 10 * si + 3 * int(use_faces) + mi, n, use_faces, mode)))
    out.append(("V 1", 2, 5, make_case(77, 5, True, "given", V=1)))
    return out


def check_records(name, got, before, first, n, case):
    """`got` against the numpy restatement: the copied words bit for bit, flat normals with NaNs equal, everything else untouched"""
    want = numpy_deform(before, first, n, case["vertices"], case["faces"], case["normals"], case["flags"])
    assert got.shape == want.shape, name
    assert np.array_equal(bits(got[:, POS_WORDS]), bits(want[:, POS_WORDS])), name
    if case["flags"] & FLAT:
        assert same(got[:, NRM_WORDS], want[:, NRM_WORDS]), name
    else:
        assert np.array_equal(bits(got[:, NRM_WORDS]), bits(want[:, NRM_WORDS])), name
    written = POS_WORDS + (NRM_WORDS if case["normals"] is not None or case["flags"] & FLAT else [])
    other = np.setdiff1d(np.arange(40), written)
    assert np.array_equal(bits(got[:, other]), bits(before[:, other])), name
    outside = np.r_[0:first, first + n:got.shape[0]]
    assert np.array_equal(bits(got[outside]), bits(before[outside])), name


# ---- refit_common's deformations as vertex arrays ----
def mesh_vertices(triangles, first, count, kind, phase=0.0):
    """(count, 3, 3) float32: the corners refit_common.deform() gives triangles [first, first + count)"""
    t = deform(triangles, first, count, kind, phase)
    return np.ascontiguousarray(np.stack([t[first:first + count, c] for c in CORNER_COLS], axis=1), F)


def indexed(corners):
    """(T, 3, 3) corners -> ((V, 3) unique vertices, (T, 3) uint32 faces): the same positions through an index table"""
    flat = np.ascontiguousarray(corners, F).reshape(-1, 3)
    uniq, inverse = np.unique(bits(flat), axis=0, return_inverse=True)
    return np.ascontiguousarray(uniq).view(F), np.ascontiguousarray(inverse.reshape(-1, 3).astype(np.uint32))
