"""Instance visibility masks (include/rt355.h: rt_write_instance_masks, rt_set_query_masks) on a machine without a GPU: the header
declares the two functions and the library exports them, they reject a NULL context before they need a device, the Python packing
helper takes what it should and refuses the rest, and the reference of the GPU tests -- the twin scene of tests/mask_common.py --
is held against the float32 brute force filtered by visibility, with the trials shown to move the reference's answers."""
import os
import re

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import tri_buffers
from mask_common import TRIALS, assert_trials_move, filter_hits, instance_masks, nearest_of, twin, visible
from query_common import F, all_triangle_hits, bits, camera_rays, random_rays, scene_box
from test_ray_query_gpu import tri_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_SYMBOLS = ["rt_write_instance_masks", "rt_set_query_masks"]
CASES = tri_cases()


def test_header_declares_and_library_exports_the_mask_entry_points():
    text = open(os.path.join(ROOT, "include", "rt355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = abi.load()
    for name in MASK_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/rt355.h does not declare %s" % name
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert re.search(r"\bint\s+rt_write_instance_masks\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*const\s+uint32_t\s*\*\s*masks\s*,\s*uint32_t\s+n\s*\)", code)
    assert re.search(r"\bint\s+rt_set_query_masks\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+nearest\s*,\s*uint32_t\s+occlusion\s*\)", code)
    assert lib.rt_abi_version() == 4                     # additive: the ABI version stays
    assert re.search(r"#define\s+RT355_ABI_VERSION\s+4\b", code)


def test_a_null_context_is_rejected_by_name():
    lib = abi.load()
    masks = np.array([1, 2, 3], np.uint32)
    as_u32 = masks.ctypes.data_as(abi.ctypes.POINTER(abi.ctypes.c_uint32))
    assert lib.rt_write_instance_masks(None, as_u32, 3) == abi.RT_ERR_INVALID_ARG
    assert b"rt_write_instance_masks" in lib.rt_last_error(None)
    assert lib.rt_write_instance_masks(None, None, 0) == abi.RT_ERR_INVALID_ARG     # the context is checked first
    assert b"rt_write_instance_masks" in lib.rt_last_error(None)
    assert lib.rt_write_instance_masks(None, None, 3) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_last_error(None) == b"rt_write_instance_masks: ctx is NULL"
    assert lib.rt_set_query_masks(None, 1, 2) == abi.RT_ERR_INVALID_ARG
    assert b"rt_set_query_masks" in lib.rt_last_error(None)


def test_the_packing_helper():
    pack = rt.RendererRaytracing._pack_masks
    for empty in (None, [], (), np.zeros(0, np.int64)):
        m = pack(empty)
        assert m.dtype == np.uint32 and m.shape == (0,)
    want = np.array([0, 1, 0x80000004, 0xFFFFFFFF], np.uint32)
    for given in ([0, 1, 0x80000004, 0xFFFFFFFF], (0, 1, 0x80000004, 0xFFFFFFFF), want, want.astype(np.uint64), want.astype(np.int64),
                  np.array([0, 1, 0x80000004, 0xFFFFFFFF], object), want[::-1][::-1]):
        m = pack(given)
        assert m.dtype == np.uint32 and m.shape == (4,) and m.flags["C_CONTIGUOUS"] and np.array_equal(m, want)
    strided = np.arange(10, dtype=np.uint32)[::3]
    assert np.array_equal(pack(strided), [0, 3, 6, 9]) and pack(strided).flags["C_CONTIGUOUS"]
    assert np.array_equal(pack(np.array([7], np.uint8)), [7]) and pack(np.array([7], np.uint8)).dtype == np.uint32
    assert np.array_equal(pack(instance_masks(5)), instance_masks(5))
    for bad in ([-1], [2 ** 32], [1, 2 ** 40], [1.0, 2.0], np.array([1.0]), [[1, 2], [3, 4]], np.zeros((2, 2), np.uint32), 5, np.uint32(5),
                "12", b"12", [1, "2"], [None], [True, False], [1, 2.5], np.array([-5], np.int32)):
        with pytest.raises(ValueError):
            pack(bad)


def test_the_masks_of_the_trials():
    assert list(instance_masks(3)) == [1, 0x80000002, 4]
    assert list(instance_masks(5)) == [1, 0, 4, 0x80000001, 2]
    assert list(instance_masks(7)[3:]) == [0x80000001, 2, 0x80000004, 1]
    for n in (1, 3, 5, 17):
        assert not visible(instance_masks(n), 0).any() and not visible(instance_masks(n), 0x7FFFFFF8).any()
        assert visible(instance_masks(n), 0xFFFFFFFF).sum() == (n if n < 4 else n - 1)
    assert list(visible([0, 0], 1, 4)) == [False, False, True, True]      # records beyond the table are visible
    assert list(visible([5, 5, 5], 4, 2)) == [True, True]


def scene_rays(buf, scene):
    lo, hi = scene_box(buf, scene)
    o1, d1 = camera_rays(scene, 96, 64)
    o2, d2 = random_rays(lo, hi, 3000, 7)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


@pytest.mark.parametrize("name", ["inst5", "inst17", "ref"])
def test_the_twin_is_the_brute_force_filtered_by_visibility(oracle, name):
    scene, mat = CASES[name]()
    buf = tri_buffers(scene, mat)
    o, d = scene_rays(buf, scene)
    if name == "ref":                                   # (the brute force over the reference scene's triangles: fewer rays)
        o, d = o[::6], d[::6]
    n_blas = np.asarray(buf["blas"]).reshape(-1, 20).shape[0]
    masks = instance_masks(n_blas)
    with np.errstate(all="ignore"):
        cand = all_triangle_hits(buf, o, d)
    kept = dict((k, np.array(np.asarray(v), copy=True)) for k, v in buf.items())
    seen = set()
    for trial in TRIALS:
        vis = visible(masks, trial, n_blas)
        tw = twin(buf, vis)
        t = oracle.trace_tri_rays(tw, o, d)
        with np.errstate(all="ignore"):
            want = nearest_of(o.shape[0], filter_hits(cand, vis))
        assert np.array_equal(bits(t), bits(want)), "trial 0x%x: the twin and the filtered brute force differ on %d rays" % (
            trial, int((bits(t) != bits(want)).sum()))
        if not vis.any():
            assert np.all(t == F(-1.0))
        seen.add(vis.tobytes())
    assert len(seen) >= (3 if n_blas >= 3 else 2)       # the trials are different visibility sets
    for k, v in kept.items():                           # twin() left the buffers as they were
        assert np.array_equal(np.asarray(buf[k]), v)
    assert np.array_equal(bits(oracle.trace_tri_rays(twin(buf, np.ones(n_blas, bool)), o, d)), bits(oracle.trace_tri_rays(buf, o, d)))


@pytest.mark.parametrize("name", list(CASES))
def test_the_trials_move_the_reference(oracle, name):
    scene, mat = CASES[name]()
    buf = tri_buffers(scene, mat)
    o, d = scene_rays(buf, scene)
    n_blas = np.asarray(buf["blas"]).reshape(-1, 20).shape[0]
    if n_blas >= 3:
        moved = assert_trials_move(oracle, buf, o, d, instance_masks(n_blas))
    else:
        from mask_common import moving_trials
        moved = moving_trials(oracle, buf, o, d, instance_masks(n_blas))
    hidden = dict((m[0], m[1]) for m in moved)
    assert hidden[0] == 0 and hidden[0x7FFFFFF8] == 0   # these two hide everything
