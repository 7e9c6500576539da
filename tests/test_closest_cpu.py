"""Closest-point queries (include/rt355.h: rt_closest_points, rt_closest_points_host, rt_closest_points_model) on a machine without a
GPU: the host model -- the kernel's own inline arithmetic and walk (csrc/rt_closest.h), run serially -- against the numpy brute
force over every (instance, slot) pair (tests/closest_common.py), bit for bit on every field; ties, masks, the radii, that the
pruning prunes, and the status codes that need no device."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from closest_common import (ALL, F, RADII, assert_same, brute, leaf, make_points, mixed_radii, model, n_pairs, shear_records, twin_scene,
                            with_radius, world_corners)
from helpers import tri_buffers, triangle_scene
from tlas_common import tight_buffers

N_POINTS = 500


def seed3():
    scene, mat = triangle_scene(seed=3, n_models=5)
    return scene, tri_buffers(scene, mat)


def scene_buffers(name):
    if name == "seed3":
        return seed3()[1]
    if name == "sheared":
        return shear_records(seed3()[1])
    if name == "tight":
        scene, buf = seed3()
        return tight_buffers(scene, buf)[0]
    scene, mat = triangle_scene(seed=4, n_models=20)
    return tri_buffers(scene, mat)


@pytest.fixture(scope="module", params=["seed3", "sheared", "tight", "21 instances"])
def case(request):
    """(buffers, points (n, 3), brute force under an infinite radius) -- computed once, shared, left unchanged"""
    buf = scene_buffers(request.param)
    pts = make_points(buf, N_POINTS, 5)
    return buf, pts, brute(buf, with_radius(pts, np.inf))


def test_the_model_is_the_brute_force(case):
    buf, pts, want = case
    rc, got, tests = model(buf, with_radius(pts, np.inf))
    assert rc == abi.RT_OK and tests > 0
    assert_same(got, want, "infinite radius")
    assert (want["prim"] >= 0).all()                                        # an unbounded search always finds something
    on_corner = want["dist2"][::5] == 0
    assert on_corner.all(), "every fifth point sits on a corner: %d do not" % int((~on_corner).sum())
    # the records are what they say: barycentrics rebuild the point to float32 accuracy, dist2 is the distance to it
    e = pts.astype(np.float64) - want["point"].astype(np.float64)
    assert np.allclose((e * e).sum(axis=1), want["dist2"], rtol=1e-5, atol=1e-9)
    assert ((want["u"] >= 0) & (want["v"] >= 0) & (want["u"] + want["v"] <= 1 + 1e-6)).all()


def test_every_radius(case):
    buf, pts, unbounded = case
    points = mixed_radii(pts, 6)
    want = brute(buf, points)
    rc, got, _ = model(buf, points)
    assert rc == abi.RT_OK
    assert_same(got, want, "mixed radii")
    radius = points[:, 3]
    with np.errstate(invalid="ignore"):
        r2 = (radius * radius).astype(F)
        inside = (radius >= 0) & (unbounded["dist2"] <= r2)
    assert np.array_equal(want["prim"] >= 0, inside)                         # a hit exactly where the unbounded answer is within r2
    assert_same(want[inside], unbounded[inside], "within the radius the answer is the unbounded one")
    miss = want[~inside]
    assert (miss["dist2"] == -1).all() and (miss["instance"] == -1).all() and not miss["point"].any() and not miss["u"].any()
    for r in RADII:                                                          # every radius of the list met hits and misses as it should
        sel = (radius == r) if r == r else np.isnan(radius)
        assert sel.sum() > 20
        if r == np.inf:
            assert inside[sel].all()
        elif not r >= 0:
            assert not inside[sel].any()
        elif r == 0:
            assert inside[sel].any() and not inside[sel].all()               # the points on corners are at distance zero
        else:
            assert inside[sel].any()


def test_ties_resolve_by_index():
    scene, mat = twin_scene()
    buf = tri_buffers(scene, mat)
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    assert np.array_equal(blas[1], blas[3]) and not np.array_equal(blas[0], blas[1])
    pts = make_points(buf, 300, 7)
    points = with_radius(pts, np.inf)
    want = brute(buf, points)
    rc, got, _ = model(buf, points)
    assert rc == abi.RT_OK
    assert_same(got, want, "coincident instances")
    assert (want["instance"] == 1).sum() > 30 and not (want["instance"] == 3).any()
    # hiding instance 1 shows the tie: its twin answers with the same bits
    hidden = brute(buf, points, masks=[ALL, 0, ALL, ALL])
    sel = want["instance"] == 1
    assert np.isin(hidden["instance"][sel], (2, 3)).all()                   # (2: the floor, which the mesh stands on, ties at its lowest vertex)
    sel &= hidden["instance"] == 3
    assert sel.sum() > 30
    for f in ("dist2", "u", "v", "prim", "point"):
        assert np.array_equal(hidden[f][sel].view(np.uint32), want[f][sel].view(np.uint32)), f
    # a point on a vertex several triangles share: the lowest prim among those at distance zero
    wc = world_corners(buf)
    shared = 0
    for i in np.nonzero(want["dist2"] == 0)[0]:
        bi = int(want["instance"][i])
        _, prims, w = wc[bi]
        touching = np.nonzero((w == pts[i]).all(axis=2).any(axis=1))[0]
        # (a zero-area triangle of the mesh's poles gives a NaN distance and is no candidate)
        with np.errstate(all="ignore"):
            at_zero = [int(prims[j]) for j in touching if leaf([pts[i:i + 1, k] for k in range(3)], w[j, 0], w[j, 1], w[j, 2])[0][0] == 0]
        if len(at_zero) > 1:
            shared += 1
            assert want["prim"][i] == min(at_zero)
    assert shared > 10


def test_masks_hide_instances(case):
    buf, pts, unbounded = case
    n_blas = np.asarray(buf["blas"]).reshape(-1, 20).shape[0]
    winner = int(np.bincount(unbounded["instance"], minlength=n_blas).argmax())           # the instance most points are nearest to
    masks = np.full(n_blas, 0x6, np.uint32)
    masks[winner] = 0x1
    points = with_radius(pts, np.inf)
    want = brute(buf, points, masks=masks, ray_mask=0x4)
    assert not (want["instance"] == winner).any() and (want["prim"] >= 0).all()
    moved = (unbounded["instance"] == winner).sum()
    assert moved > 20
    rc, got, _ = model(buf, points, masks=masks, ray_mask=0x4)
    assert rc == abi.RT_OK
    assert_same(got, want, "the winner's instance hidden")
    rc, got, _ = model(buf, points, masks=masks[:winner + 1], ray_mask=0x1)                # records beyond the table: all ones
    assert rc == abi.RT_OK
    assert_same(got, brute(buf, points, masks=masks[:winner + 1], ray_mask=0x1), "a short table")
    rc, got, tests = model(buf, points, masks=masks, ray_mask=0)
    assert rc == abi.RT_OK and tests == 0
    assert (got["dist2"] == -1).all() and (got["prim"] == -1).all() and (got["instance"] == -1).all()
    assert not got["point"].any() and not got["u"].any() and not got["v"].any()


def test_the_pruning_prunes():
    """The unmodified seed-3 scene under the reference's placeholder top-level boxes, 300 points uniform in
    [-8, -1, -13] .. [8, 5, 1], infinite radius: at most a quarter of the 642 pairs per point (the float64 recipe of the issue
    measured 0.045 x 642; a walk that prunes nothing tests all 642)."""
    _, buf = seed3()
    assert n_pairs(buf) == 642
    rng = np.random.default_rng(11)
    pts = rng.uniform([-8.0, -1.0, -13.0], [8.0, 5.0, 1.0], (300, 3)).astype(F)
    points = with_radius(pts, np.inf)
    rc, got, tests = model(buf, points)
    assert rc == abi.RT_OK
    print("candidate tests per point: %.2f of 642" % (tests / 300.0))
    assert tests / 300.0 <= 0.25 * 642
    assert_same(got, brute(buf, points), "the pruned search")


def test_status_codes_without_a_device():
    L = abi.load()
    _, buf = seed3()
    pts = with_radius(np.zeros((2, 3), F), 1.0)
    out = np.zeros(2, dtype=abi.CLOSEST_DTYPE)
    arr = {k: np.ascontiguousarray(buf[k], F) for k in ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")}
    per = dict(triangles=40, tri_lookup=1, nodes=8, blas=20, blas_lookup=1)
    order = ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")

    def call(points=pts, n=2, result=out, null=None, empty=None, masks=None, n_masks=0):
        args = []
        for k in order:
            args += [None if k == null else ctypes.c_void_p(arr[k].ctypes.data), 0 if k == empty else arr[k].size // per[k]]
        return L.rt_closest_points_model(None if points is None else ctypes.c_void_p(points.ctypes.data), n, *args, masks, n_masks, ALL,
                                         None if result is None else ctypes.c_void_p(result.ctypes.data), None)

    assert call() == abi.RT_OK                                               # (tests may be NULL)
    assert call(points=None, n=0, result=None) == abi.RT_OK                  # n == 0 comes first
    assert call(points=None) == abi.RT_ERR_INVALID_ARG and b"rt_closest_points_model" in L.rt_last_error(None)
    assert call(result=None) == abi.RT_ERR_INVALID_ARG
    for k in order:
        assert call(null=k) == abi.RT_ERR_INVALID_ARG, k
        assert call(empty=k) == abi.RT_ERR_STATE, k
    assert call(masks=None, n_masks=3) == abi.RT_ERR_INVALID_ARG
    # the context forms: the context is checked before anything needs a device -- and before n == 0
    vp = ctypes.c_void_p
    assert L.rt_closest_points(None, vp(pts.ctypes.data), 2, vp(out.ctypes.data), None) == abi.RT_ERR_INVALID_ARG
    assert L.rt_last_error(None) == b"rt_closest_points: ctx is NULL"
    assert L.rt_closest_points(None, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
    assert L.rt_closest_points_host(None, vp(pts.ctypes.data), 2, vp(out.ctypes.data)) == abi.RT_ERR_INVALID_ARG
    assert L.rt_last_error(None) == b"rt_closest_points_host: ctx is NULL"
    assert L.rt_closest_points_host(None, None, 0, None) == abi.RT_ERR_INVALID_ARG
    ctx = vp()
    if L.rt_create(0, ctypes.byref(ctx)) != abi.RT_OK:                       # no device here: nothing was made, and the calls still answer
        assert not ctx.value
        assert L.rt_closest_points_host(ctx, vp(pts.ctypes.data), 2, vp(out.ctypes.data)) == abi.RT_ERR_INVALID_ARG
    else:
        L.rt_destroy(ctx)


def test_the_record_layout():
    assert np.dtype(abi.CLOSEST_DTYPE).itemsize == 32 == ctypes.sizeof(abi.RtClosest)
    for (name, _, *_), (cname, _) in zip(abi.CLOSEST_DTYPE, abi.RtClosest._fields_):
        assert name == cname and np.dtype(abi.CLOSEST_DTYPE).fields[name][1] == getattr(abi.RtClosest, cname).offset
    assert hasattr(rt.RendererRaytracing, "closest_points")
