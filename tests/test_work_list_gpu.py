"""Awaited triangle frames rendered from a work list that splits tiles, in every form of the kernel such a frame can take.

From 4,096 tiles on, an awaited frame renders its tiles in the order the previous frame on the same stream left behind
(rt_api.hip: order_set; rt_triangles.hip: order_hist / order_scatter), the longest of them as four 4x4 quarters or sixteen 2x2
sixteenths.  The first such frame of a context (and the first after a change of the tile count) renders without a list.  Where that list splits tiles the forms 1 and 3 take trace_roles (kernel id 10), whose idle lanes trace the next
reflection ray while the owners trace the shadow ray; every other form takes trace_triangles (8) over the same list.

Every frame here is compared bit for bit with the CPU oracle, and its ray count with the oracle's.  The scene turns and the camera
moves on every frame, so a part a list skipped cannot pass on the pixels an earlier frame left in the colour buffer.  The
scenes do split their lists: tests/test_work_list_scenes_cpu.py checks that on the oracle's work."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi, tiles
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA
from helpers import (RAGGED_STEP, ROLES_CASES, WL_BOUNCES, WL_H, WL_W, WORK_LIST_CASES, WorkListCase, diff_stats, ragged_edge_case, random_sky,
                     spine_scene, tri_buffers)

pytestmark = pytest.mark.gpu
ROLES, TRIANGLES, HEATMAP = 10, 8, 9


def flat_sky():
    return rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)


def tiny_sky():
    """Six 1x1 faces of different colours: not the flat sky the library compiles a form of its own for (rt_api.hip: sky_flat)."""
    m = rt.CubemapMaterial()
    m.faces = [np.array([[[40 * k + 10, 200 - 30 * k, 90 + 25 * k, 255]]], np.uint8) for k in range(6)]
    return m


SKIES = {"flat": flat_sky, "textured": lambda: random_sky(5), "tiny": tiny_sky}


def check(oracle, r, scene, mat, sky, B, W, H, what, tile_first=0, tile_step=1):
    """The frame just rendered against the oracle: pixels (this rank's rows) and rays.  -> rt_stats."""
    img = r.read_pixels()
    ref, _, rays = oracle.render_tri(scene.pack_params(B), tri_buffers(scene, mat), sky.faces, W, H, tile_first, tile_step)
    if tile_step > 1:
        ref = ref[[y for y in range(H) if (y // 8) % tile_step == tile_first]]
    st = r.stats()
    assert np.array_equal(img, ref), (what, diff_stats(img, ref))
    assert st["rays"] == rays, (what, st["rays"], rays)
    return st


def resize(r, W, H):
    abi.check(r._lib.rt_resize(r._ctx, W, H), r._ctx)
    r.width, r.height = W, H


def partition(r, rank, world):
    abi.check(r._lib.rt_set_partition(r._ctx, rank, world), r._ctx)
    r.rank, r.world = rank, world


def renderer(case, sky, W=WL_W, H=WL_H, B=WL_BOUNCES, **kw):
    r = rt.RendererRaytracing(W, H, case.scene, maxBounces=B, **kw).initialize(sky, case.mat)
    r.set_variant(case.variant)
    return r


# ---- a. every awaited form over a list that splits tiles ------------------------------------------------------------------------
@pytest.mark.parametrize("name,sky", [(n, s) for n in WORK_LIST_CASES for s in ("flat", "textured")] + [(n, "tiny") for n in ROLES_CASES])
def test_every_awaited_form_over_a_splitting_list(oracle, name, sky):
    case, sk = WorkListCase(name), SKIES[sky]()
    r = renderer(case, sk)
    kernels, forms = [], []
    try:
        for f in range(12):                      # the first frame without a list, then eleven from lists
            case.advance()
            r.render()
            st = check(oracle, r, case.scene, case.mat, sk, WL_BOUNCES, WL_W, WL_H, (name, sky, f))
            kernels.append(st["kernel_id"]); forms.append(st["tri_form"])
            assert st["tri_form"] == case.form(), (f, st["tri_form"], case.form())
    finally:
        r.close()
    print(name, sky, "kernels", kernels, "forms", forms)
    if name in ROLES_CASES:
        assert ROLES in kernels[1:], kernels
        assert set(kernels) <= {ROLES, TRIANGLES}
    else:
        assert set(kernels) == {TRIANGLES}, kernels


# ---- b. bounce limits through trace_roles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROLES_CASES)
def test_bounce_limits_through_the_roles_kernel(oracle, name):
    """maxBounces travels with every frame's parameters: after four frames at 3 the lists split tiles, and the next frames run
    trace_roles at 0 (a helper never receives a ray), 6 (owners leave the loop while their helpers still walk), 1 and 2 -- five
    frames each: the first from a list made at another limit, the others from lists made at that limit."""
    case, sky = WorkListCase(name), flat_sky()
    r = renderer(case, sky)
    try:
        for f in range(4):
            case.advance()
            r.render()
            check(oracle, r, case.scene, case.mat, sky, 3, WL_W, WL_H, (name, 3, f))
        for B in (0, 6, 1, 2):
            r.maxBounces = B
            kernels = []
            for f in range(5):
                case.advance()
                r.render()
                kernels.append(check(oracle, r, case.scene, case.mat, sky, B, WL_W, WL_H, (name, B, f))["kernel_id"])
            assert ROLES in kernels, (B, kernels)
    finally:
        r.close()


# ---- c. the longest tiles at the ragged edge ------------------------------------------------------------------------------------
def test_split_parts_at_the_ragged_edges(oracle):
    """The camera turned so that the meshes sit in the ragged last column and the ragged last row (helpers.ragged_edge_case):
    split parts whose owners fall outside the frame leave together with their helpers (rt_triangles.hip: trace_roles)."""
    for sky in (flat_sky(), random_sky(7)):
        case = ragged_edge_case()
        r = renderer(case, sky)
        kernels = []
        try:
            for f in range(10):
                case.advance(*RAGGED_STEP)
                r.render()
                kernels.append(check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, WL_W, WL_H, f)["kernel_id"])
        finally:
            r.close()
        assert ROLES in kernels, kernels


# ---- d. the stack clamp inside split parts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [21, 33])
def test_stack_overflow_inside_split_parts(oracle, depth):
    """A BLAS spine deeper than the reference's twenty stack slots (helpers.spine_scene): the clamp of the BLAS stack runs inside
    the quarters and sixteenths of trace_roles."""
    scene = spine_scene(depth)
    mat = rt.Material(np.random.default_rng(depth).integers(0, 256, (8, 8, 4), dtype=np.uint8))
    sky = random_sky(depth)
    r = rt.RendererRaytracing(WL_W, WL_H, scene, maxBounces=3).initialize(sky, mat)
    kernels = []
    try:
        for f in range(10):
            scene.camera.move(0.02, 0.01)
            r.render()
            kernels.append(check(oracle, r, scene, mat, sky, 3, WL_W, WL_H, (depth, f))["kernel_id"])
    finally:
        r.close()
    assert ROLES in kernels, kernels


# ---- e. the kernel switch in both directions ------------------------------------------------------------------------------------
def test_the_kernel_switch_in_both_directions(oracle):
    """The host picks the kernel from whether the stream's list splits tiles (a pinned word, maybe a frame old).  A camera that
    looks at the meshes, then straight down at the floor (every tile alike), then back at the meshes: the floor's lists split
    nothing, and the first frame back renders the meshes from such a list with trace_triangles, the next ones from lists that
    split with trace_roles: the sequence shows the switch 10 -> 8 and 8 -> 10.
    A change of view alone does not clear a splitting list: the parts of a split tile leave their times scaled to a whole tile
    (rt_triangles.hip: cost_mul4 / cost_mul16), and on a view of like tiles that keeps them above the rule's threshold.  The floor
    is therefore rendered at another tile count (66 x 64): its first frame takes no list, and the lists after it are the floor's."""
    case, sky = WorkListCase("form1"), random_sky(11)
    r = renderer(case, sky)
    seq = []
    try:
        for view, W, n in (("mesh", WL_W, 6), ("floor", 525, 6), ("mesh", 525, 6)):
            if W != r.width:
                resize(r, W, WL_H)
            case.scene.camera.spin(0.0, 100.0 if view == "floor" else (-74.0 if seq else 0.0))
            for f in range(n):
                case.advance(forwards=0.01, right=0.01)
                r.render()
                seq.append((view, check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, W, WL_H, (view, f))["kernel_id"]))
    finally:
        r.close()
    kernels = [k for _, k in seq]
    print("kernel switch", kernels)
    assert TRIANGLES in kernels[7:12], kernels             # the floor: lists that split nothing
    pairs = set(zip(kernels, kernels[1:]))
    assert (ROLES, TRIANGLES) in pairs and (TRIANGLES, ROLES) in pairs, kernels
    assert kernels[12] == TRIANGLES and ROLES in kernels[13:], kernels


# ---- f. the threshold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,listed", [(520, 504, False), (512, 512, True), (WL_W, WL_H, True)])
def test_the_work_list_threshold(oracle, W, H, listed):
    """4,095 tiles: no list, never trace_roles; exactly 4,096 and 4,160 (ragged): lists, and trace_roles over them."""
    case, sky = WorkListCase("form1"), flat_sky()
    r = renderer(case, sky, W, H)
    kernels = []
    try:
        for f in range(8):
            case.advance()
            r.render()
            kernels.append(check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, W, H, f)["kernel_id"])
    finally:
        r.close()
    assert (ROLES in kernels) == listed, kernels


# ---- g. resize and partition changes between awaited frames ---------------------------------------------------------------------
def test_resize_and_partition_changes_between_awaited_frames(oracle):
    """One context: 4,160 tiles; grown to 8,320 (the cost and list buffers reallocated); shrunk back (reused); the same tile
    count in a new shape (the streams' old lists applied to new geometry); grown to 16,640 and then halved by a partition
    change, and the other rank of that partition (the same tile count: the lists made for one rank's tiles on the other's)."""
    case, sky = WorkListCase("form1"), flat_sky()
    r = renderer(case, sky)
    try:
        steps = [("start", WL_W, WL_H, None), ("grow", 1024, 516, None), ("shrink", WL_W, WL_H, None),
                 ("reshape", WL_H, WL_W, None), ("grow again", 1024, 1036, None), ("rank 1 of 2", 1024, 1036, (1, 2)),
                 ("rank 0 of 2", 1024, 1036, (0, 2))]
        for what, W, H, part in steps:
            if (W, H) != (r.width, r.height):
                resize(r, W, H)
            if part:
                partition(r, *part)
            rank, world = part or (0, 1)
            kernels = []
            for f in range(6):
                case.advance()
                r.render()
                kernels.append(check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, W, H, (what, f), rank, world)["kernel_id"])
            assert ROLES in kernels[1:], (what, kernels)
    finally:
        r.close()


# ---- h. triangle scenes as ranks of a partition ---------------------------------------------------------------------------------
PARTITION_SIZES = {2: (1024, 520), 3: (1024, 776), 8: (2048, 1032)}     # every rank's share: 4,096 tiles or more


@pytest.mark.parametrize("world", [2, 3, 8])
def test_awaited_triangle_frames_as_ranks_of_a_partition(oracle, world):
    """Each rank renders its strided tile set from lists of its own (trace_roles over a strided set); with two and three ranks
    every rank plays along and the ranks' last frames, laid out as the all-gather would and put together by rt_assemble_frame,
    are the oracle's whole frame, their ray counts its count."""
    import torch
    W, H = PARTITION_SIZES[world]
    ranks = list(range(world)) if world <= 3 else [0, world - 1]
    cases = {k: WorkListCase("form1") for k in ranks}        # the same scene and path for every rank
    sky = random_sky(13)
    rs = {k: renderer(cases[k], sky, W, H, rank=k, world=world) for k in ranks}
    msg = tiles.message_bytes(W, H, world)
    gathered = torch.zeros(world * msg, dtype=torch.uint8, device="cuda")
    try:
        kernels = {k: [] for k in ranks}
        for f in range(7):
            for k in ranks:
                c = cases[k]
                c.advance()
                rs[k].render()
                kernels[k].append(check(oracle, rs[k], c.scene, c.mat, sky, WL_BOUNCES, W, H, (k, f), k, world)["kernel_id"])
        for k in ranks:
            assert ROLES in kernels[k], (k, kernels[k])
        if world > 3:
            return
        stream = torch.cuda.current_stream().cuda_stream
        rays = 0
        for k in ranks:
            cases[k].advance()
            rs[k].render_to(gathered[k * msg:(k + 1) * msg].data_ptr(), msg, stream)
            rs[k].wait()
            rays += rs[k].stats()["rays"]
        frame = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
        rs[ranks[-1]].assemble_frame(gathered.data_ptr(), frame.data_ptr(), world, stream)
        torch.cuda.synchronize()
        c = cases[0]
        ref, _, ref_rays = oracle.render_tri(c.scene.pack_params(WL_BOUNCES), tri_buffers(c.scene, c.mat), sky.faces, W, H)
        got = frame.cpu().numpy().reshape(H, W, 4)
        assert np.array_equal(got, ref), diff_stats(got, ref)
        assert rays == ref_rays
    finally:
        for x in rs.values():
            x.close()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_triangle_frames_in_flight_as_ranks_of_a_partition(oracle, world):
    """Frames in flight take no list and render their tiles in the XCD-row order over a grid padded to eight rows (rt_triangles.hip:
    xcd_rows): each rank enqueues four frames without waiting into its slot of four all-gather layouts; every frame, put
    together, is the oracle's."""
    import torch
    W, H, B = 333, 8 * 43 - 3, 3                        # 42 x 43 tiles: ragged column and row, no rank's row count a multiple of 8
    N = 4
    msg = tiles.message_bytes(W, H, world)
    gathered = [torch.zeros(world * msg, dtype=torch.uint8, device="cuda") for _ in range(N)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    sky, rays, refs = random_sky(17), [0] * N, []
    last = None
    for k in range(world):
        case = WorkListCase("form1")
        r = renderer(case, sky, W, H, rank=k, world=world)
        r.render()                                     # the scene resident; then frames in flight
        for f in range(N):
            case.advance()
            if k == 0:
                ref, _, ref_rays = oracle.render_tri(case.scene.pack_params(B), tri_buffers(case.scene, case.mat), sky.faces, W, H)
                refs.append((ref, ref_rays))
            r.render_to(gathered[f][k * msg:(k + 1) * msg].data_ptr(), msg, streams[f % 2].cuda_stream)
        r.wait()
        torch.cuda.synchronize()
        rays[N - 1] += r.stats()["rays"]
        if last is not None:
            last.close()
        last = r
    try:
        frame = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
        for f in range(N):
            last.assemble_frame(gathered[f].data_ptr(), frame.data_ptr(), world, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = frame.cpu().numpy().reshape(H, W, 4)
            assert np.array_equal(got, refs[f][0]), (f, diff_stats(got, refs[f][0]))
        assert rays[N - 1] == refs[N - 1][1]
    finally:
        last.close()


def test_one_context_alternating_between_two_ranks_of_equal_share(oracle):
    """1024 x 1024 over two ranks: 8,192 tiles each.  One context switches rank every three frames: the first frame after each
    switch renders from the list made for the other rank's tiles."""
    W, H = 1024, 1024
    case, sky = WorkListCase("form1"), flat_sky()
    r = renderer(case, sky, W, H, rank=0, world=2)
    kernels = []
    try:
        for f in range(12):
            rank = (f // 3) % 2
            if rank != r.rank:
                partition(r, rank, 2)
            case.advance()
            r.render()
            kernels.append(check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, W, H, f, rank, 2)["kernel_id"])
    finally:
        r.close()
    assert ROLES in kernels[1:], kernels


# ---- i. the heatmap ---------------------------------------------------------------------------------------------------------------
def test_heatmap_frames_between_listed_frames(oracle):
    """Heatmap frames take no list (kernel 9) and leave the streams' lists as they were; the raytracer frames after them, which
    render from those older lists, are the oracle's."""
    case, sky = WorkListCase("form1"), flat_sky()
    r = renderer(case, sky)
    try:
        for mode, n in (("rt", 6), ("heatmap", 5), ("rt", 6)):
            (r.showHeatmap if mode == "heatmap" else r.showRaytracer)()
            kernels = []
            for f in range(n):
                case.advance()
                r.render()
                if mode == "heatmap":
                    ref, _ = oracle.heatmap_tri(case.scene.pack_params(WL_BOUNCES), tri_buffers(case.scene, case.mat), WL_W, WL_H)
                    img = r.read_pixels()
                    assert np.array_equal(img, ref), (f, diff_stats(img, ref))
                    kernels.append(r.stats()["kernel_id"])
                else:
                    kernels.append(check(oracle, r, case.scene, case.mat, sky, WL_BOUNCES, WL_W, WL_H, (mode, f))["kernel_id"])
            if mode == "heatmap":
                assert set(kernels) == {HEATMAP}, kernels
            else:
                assert ROLES in kernels, kernels
    finally:
        r.close()
