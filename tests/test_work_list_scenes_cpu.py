"""The scenes of tests/test_work_list_gpu.py really split their work lists.

The GPU tests can show that a list split tiles only where trace_roles ran (rt_stats.kernel_id 10); the forms that take
trace_triangles say nothing about it.  Here every scene and camera pose those tests rely on goes through the work-list rule
(rt_triangles.hip: order_hist, restated in helpers.model) with the MI355X's 5,120 wave slots (256 CUs x 20, rt_api.hip: wave_slots),
on a stand-in for the tiles' times: the oracle's per-pixel work -- traversals, BLAS inner-node visits, triangle tests -- summed per
8 x 8 tile.  The GPU's tile times are clock ticks, not work: this guards the shape of the scenes (some tiles many times as long
as the mean), not what a given GPU frame's list holds."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA
from helpers import (RAGGED_STEP, WL_BOUNCES, WL_H, WL_W, WORK_LIST_CASES, WorkListCase, model, ragged_edge_case, spine_scene,
                     tile_work)

WAVE_SLOTS = 256 * 20
SKY = rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)


def split_counts(oracle, case, W=WL_W, H=WL_H, B=WL_BOUNCES, rank=0, world=1):
    return model(tile_work(oracle, case.scene, case.mat, SKY, W, H, B, world, rank), WAVE_SLOTS)


@pytest.mark.parametrize("name", list(WORK_LIST_CASES))
def test_every_form_s_scene_splits_its_list(oracle, name):
    """The first pose with a list (after four frames) and the last of the twelve-frame path."""
    case = WorkListCase(name)
    for f in range(12):
        case.advance()
        if f in (4, 11):
            q4, q16, _ = split_counts(oracle, case)
            assert q4 > 0 and q16 > 0, (name, f, q4, q16)


@pytest.mark.parametrize("depth", [21, 33])
def test_deep_spines_split_their_list(oracle, depth):
    case = WorkListCase("form1")
    case.scene = spine_scene(depth)
    q4, q16, _ = split_counts(oracle, case)
    assert q4 > 0 and q16 > 0


def test_the_longest_tiles_lie_in_the_ragged_last_column_and_row(oracle):
    case = ragged_edge_case()
    for f in range(10):
        case.advance(*RAGGED_STEP)
        if f in (4, 9):
            q4, q16, cls = split_counts(oracle, case)
            assert q4 > 0 and q16 > 0
            # the tiles of classes above the last split tile's class are split whatever the order within a class
            last = np.sort(cls)[::-1][q4 + q16 - 1]
            split = (cls > last).reshape((WL_H + 7) // 8, (WL_W + 7) // 8)
            assert split[:, -1].sum() > 0 and split[-1, :].sum() > 0, f


def test_a_close_up_of_the_floor_splits_nothing(oracle):
    """The uniform view of the kernel-switch test, straight down at the floor: every tile alike, the rule splits nothing."""
    case = WorkListCase("form1")
    case.scene.camera.spin(0.0, 100.0)
    case.advance(forwards=0.01, right=0.01)
    assert split_counts(oracle, case, W=525)[:2] == (0, 0)


@pytest.mark.parametrize("W,H,rank,world", [(512, 512, 0, 1), (1024, 516, 0, 1), (WL_H, WL_W, 0, 1), (1024, 1036, 1, 2),
                                            (1024, 520, 0, 2), (1024, 520, 1, 2), (1024, 776, 2, 3), (2048, 1032, 7, 8),
                                            (1024, 1024, 1, 2)])
def test_the_sizes_and_ranks_split_their_lists(oracle, W, H, rank, world):
    """The frame sizes and the ranks' strided tile sets of the threshold, resize and partition tests."""
    case = WorkListCase("form1")
    for _ in range(5):
        case.advance()
    q4, q16, _ = split_counts(oracle, case, W, H, rank=rank, world=world)
    assert q4 > 0 and q16 > 0
