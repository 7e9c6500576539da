"""The refit of moved spheres (rt_bvh.hip: bvh_refit) restated in numpy (helpers.refit_model), checked without a GPU.

After rt_write_spheres with an unchanged count a frame keeps the device's hierarchy topology and refits its inner nodes
on the device; tests/test_moving_spheres_gpu.py compares what the device writes with refit_model bit for bit.  Here the
model itself is pinned: against a scalar, lane-by-lane transcription of the kernel (the 64-lane member stride, each lane's
first strict maximum, the lowest lane that holds the wave's maximum), and its records against the walk's slack bound
(check_tree(tight=False)) on topologies built for OTHER positions -- the device's situation -- at the inputs where a
bound goes wrong: nodes wider than a wave, two-member nodes, coincident centres, zero and tiny radii, NaN coordinates,
far offsets with wide radius ratios, exact ties for the farthest member, and a topology of a different arrangement."""
import math

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import synthetic_spheres
from helpers import (BVH_SIGMA, FILTER_EPS, FILTER_KAPPA, FILTER_SCALE, LEAF, MOVING_BOUNDARY_MOTIONS, SPHERE_CASES,
                     build_hierarchy, check_tree, drift_spheres, expected_sphere_form, leaf_records, refit_model,
                     teleport_spheres)


def records(centres, radii):
    """(n, 8) float32 records {cx, cy, cz, 0, r, g, b, radius}"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    rec = np.zeros((c.shape[0], 8), np.float32)
    rec[:, 0:3] = c
    rec[:, 4:7] = 0.5
    rec[:, 7] = np.broadcast_to(np.asarray(radii, np.float64), (c.shape[0],))
    return rec


def synthetic(n, seed):
    return np.ascontiguousarray(rt.SceneRaytracing().createScene(synthetic_spheres(n, seed)).pack_spheres(), np.float32).reshape(-1, 8)


def refit_scalar(link, rec, i):
    """bvh_refit for inner node i, lane by lane, in Python floats (IEEE f64, math.sqrt correctly rounded): the kernel's loop
    nest as written, without the model's vectorisation."""
    def member(j):
        l = int(link[j])
        if not l & LEAF:
            return None
        s = rec[l & 0x7FFFFFFF]
        c = [float(v) if v == v else 0.0 for v in s[0:3]]
        r = abs(float(s[7]))
        return c, (r if r == r else 0.0)

    first, end = i + 1, int(link[i]) >> 2
    lanes = [[m for m in (member(j) for j in range(first + lane, end, 64)) if m is not None] for lane in range(64)]

    def radius_at(P):
        best, bc = [-1.0] * 64, [[0.0, 0.0, 0.0]] * 64
        for lane in range(64):
            for c, r in lanes[lane]:
                dx, dy, dz = c[0] - P[0], c[1] - P[1], c[2] - P[2]
                d = math.sqrt(dx * dx + dy * dy + dz * dz) + r
                if d > best[lane]:
                    best[lane], bc[lane] = d, c
        R = max(best)
        return R, bc[min(l for l in range(64) if best[l] == R)]

    mn = [min(c[a] - r for ms in lanes for c, r in ms) for a in range(3)]
    mx = [max(c[a] + r for ms in lanes for c, r in ms) for a in range(3)]
    P = [0.5 * (mn[a] + mx[a]) for a in range(3)]
    Rp, far = radius_at(P)
    for _ in range(32):
        s = [far[a] - P[a] for a in range(3)]
        ln = math.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
        if not ln > 1e-12:
            break
        Q = [P[a] + s[a] / ln * 0.05 * Rp for a in range(3)]
        Rq, farq = radius_at(Q)
        if not Rq < Rp:
            break
        P, Rp, far = Q, Rq, farq
    C = np.array(P, np.float32)
    Cd = [float(v) for v in C]
    R = radius_at(Cd)[0] * BVH_SIGMA
    c2 = Cd[0] * Cd[0] + Cd[1] * Cd[1] + Cd[2] * Cd[2]
    k = c2 * (1.0 - FILTER_EPS) - R * R * (1.0 + FILTER_KAPPA)
    return np.array([C[0] * np.float32(FILTER_SCALE), C[1] * np.float32(FILTER_SCALE), C[2] * np.float32(FILTER_SCALE),
                     np.float32(k * FILTER_SCALE ** 2)], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def members_of(link, i):
    end = int(link[i]) >> 2
    return int(((link[i + 1:end] & LEAF) != 0).sum())


def refit_and_check(topology_of, moved, scalar_nodes=0):
    """the topology of `topology_of`, refitted for `moved`: the slack bound, the leaves, the sentinel, and (for the first
    `scalar_nodes` inner nodes, all of them with -1) the scalar transcription bit for bit"""
    out, link, m = build_hierarchy(topology_of)
    fit = refit_model(out, link, moved)
    check_tree(moved, fit, link, m, tight=False)
    leaf = (link[:m] & LEAF) != 0
    assert np.array_equal(bits(fit[:m][leaf]), bits(leaf_records(moved)[link[:m][leaf] & 0x7FFFFFFF]))
    assert np.array_equal(bits(fit[m]), bits(out[m]))                                      # sentinel as built
    inner = np.nonzero(~leaf)[0]
    for i in inner if scalar_nodes < 0 else inner[:scalar_nodes]:
        assert np.array_equal(bits(fit[i]), bits(refit_scalar(link, moved, i))), i
    return out, fit, link, m


def test_model_is_the_kernel_lane_by_lane():
    """Every inner node of a 300-sphere scene moved away from its topology (root-level nodes of 70-80 members: two trips of
    the 64-lane stride) equals the scalar transcription bit for bit."""
    base = synthetic(300, 11)
    _, _, link, m = refit_and_check(base, drift_spheres(base, 2, 5), scalar_nodes=-1)
    assert max(members_of(link, i) for i in range(m) if not link[i] & LEAF) > 64


def test_nodes_wider_than_a_wave():
    base = synthetic(1024, 12)
    _, _, link, m = refit_and_check(base, drift_spheres(base, 3, 6), scalar_nodes=8)
    wide = [i for i in range(m) if not link[i] & LEAF and members_of(link, i) > 64]
    assert len(wide) >= 4 and max(members_of(link, i) for i in wide) > 128


def test_two_member_nodes():
    """Five spheres: four top-level parts, one of them an inner node of two (the least a node covers)."""
    rec = records([[0, 1, -5], [2, 1, -6], [-3, 0.5, -8], [4, 2, -12], [0.5, 1.2, -5.2]], [0.5, 0.25, 0.3, 0.7, 0.2])
    _, _, link, m = refit_and_check(rec, records([[3, 0, -2], [-1, 4, -9], [0, 0, 0], [8, 1, -3], [-6, 2, -20]],
                                                 [0.1, 1.5, 0.3, 0.0, 2.0]), scalar_nodes=-1)
    assert m == 6 and sorted(members_of(link, i) for i in range(m) if not link[i] & LEAF) == [2]
    base = synthetic(64, 13)                                    # groups of two inside a larger tree
    _, _, link, m = refit_and_check(base, drift_spheres(base, 1, 7), scalar_nodes=-1)
    assert any(members_of(link, i) == 2 for i in range(m) if not link[i] & LEAF)


def test_coincident_centres():
    """All members on one point: the box centre is that point, the greedy walk stops at once (len <= 1e-12)."""
    rec = records([[0, 1, -6]] * 9, [0.1 * 2 ** k for k in range(9)])
    refit_and_check(records(np.random.default_rng(1).normal(size=(9, 3)), 0.3), rec, scalar_nodes=-1)
    rec = records([[1e5, -3e4, 2e5]] * 5, 0.0)
    refit_and_check(records(np.random.default_rng(2).normal(size=(5, 3)), 0.3), rec, scalar_nodes=-1)


def test_zero_and_tiny_radii():
    rng = np.random.default_rng(3)
    c = rng.normal(size=(40, 3)) * np.array([4.0, 1.0, 4.0]) + np.array([0.0, 1.0, -10.0])
    r = np.where(np.arange(40) % 3 == 0, 0.0, np.where(np.arange(40) % 3 == 1, 2.0 ** -31, 0.2))
    base = records(c, r)
    refit_and_check(base, drift_spheres(base, 2, 8, keep=()), scalar_nodes=-1)
    refit_and_check(base, records(c * 1e-7, r), scalar_nodes=-1)        # a whole node smaller than its members' f32 spacing


def test_one_nan_coordinate():
    """A NaN coordinate orders as 0 (the host build, bvh_refit: sphere): the node covers that member at the origin."""
    base = synthetic(200, 14)
    moved = drift_spheres(base, 1, 9)
    moved[37, 1] = np.nan
    refit_and_check(base, moved, scalar_nodes=-1)
    moved = drift_spheres(base, 1, 9)
    moved[120, 7] = np.nan
    refit_and_check(base, moved, scalar_nodes=-1)


@pytest.mark.parametrize("seed", range(6))
def test_far_offsets_and_wide_radius_ratios(seed):
    """The ranges of tests/test_filter_fuzz_gpu.py fuzz_scene: scene sizes 0.01-1000, offsets up to 1e5, radius ratios up to
    300, half of them with a ground-like sphere 10-100 scene sizes large."""
    rng = np.random.default_rng(100 + seed)
    scale = float(10 ** rng.uniform(-2, 3))
    off = [1e5, 3000.0, 1e5, 300.0, 1e5, 0.0][seed] * rng.choice([-1, 1])
    centre = np.array([off, off * 0.5, -off * 0.25])
    n = [17, 64, 200, 200, 300, 64][seed]
    ratio = 300.0 if seed % 2 == 0 else float(10 ** rng.uniform(1, 2.5))
    radii = scale * 0.25 / ratio * 10 ** rng.uniform(0, np.log10(ratio), n)
    c = centre + rng.normal(size=(n, 3)) * scale
    if seed % 2:
        R = scale * float(10 ** rng.uniform(1, 2))
        c = np.vstack([c, centre + np.array([0, -R - scale, 0])])
        radii = np.append(radii, R)
    base = records(c, radii)
    moved = base.copy()
    moved[:, 0:3] = (c + rng.normal(size=c.shape) * 0.3 * scale).astype(np.float32)
    moved[:, 7] = (radii * 10 ** rng.uniform(-0.3, 0.3, len(radii))).astype(np.float32)
    refit_and_check(base, moved, scalar_nodes=-1 if n <= 200 else 16)


def one_node(n):
    """a hand-made topology the host build never makes: one inner node over all n spheres (members 0..n-1 at node
    indices 1..n, so member k sits on lane k % 64), and the sentinel"""
    link = np.array([4 * (n + 1)] + [LEAF | k for k in range(n)] + [4 * (n + 1)], np.uint32)
    rec4 = np.zeros((n + 2, 4), np.float32)
    rec4[n + 1, 3] = np.inf
    return rec4, link, n + 1


def test_exact_ties_for_the_farthest_member():
    """Two members exactly as far from the box centre, A = (1, 0.5, 0) on lane 1 (member 1) and B = (1, -0.5, 0) on lane 0
    (member 64, behind a nearer member 0): the lowest LANE holding the maximum speaks, so the centre walks towards B, not
    towards the first member A -- and swapping the two mirrors the record.  Then symmetric scenes (a ring, a cube's corners)
    where many members tie, through the host's topologies."""
    def scene(a_at, b_at):
        c = np.zeros((70, 3))
        r = np.full(70, 0.1)
        c[5], r[5] = [-0.5, 0.0, 0.0], 0.5                  # the box's -x face: centre x = 0, farthest distance 1 < |A|
        c[a_at], r[a_at] = [1.0, 0.5, 0.0], 0.0
        c[b_at], r[b_at] = [1.0, -0.5, 0.0], 0.0
        return records(c, r)
    rec4, link, m = one_node(70)
    fits = []
    for rec in (scene(1, 64), scene(64, 1)):
        fit = refit_model(rec4, link, rec)
        check_tree(rec, fit, link, m, tight=False)
        assert np.array_equal(bits(fit[0]), bits(refit_scalar(link, rec, 0)))
        fits.append(fit[0])
    assert fits[0][1] < 0 < fits[1][1]                                  # towards B = (1, -0.5, 0) first, then its mirror
    assert np.array_equal(bits(fits[0] * np.float32([1, -1, 1, 1])), bits(fits[1]))
    ring = [[math.cos(2 * math.pi * k / 70) * 5.0, 1.0, math.sin(2 * math.pi * k / 70) * 5.0 - 10.0] for k in range(70)]
    cube = [[x, y, z] for x in (-1.0, 1.0) for y in (0.5, 2.5) for z in (-4.0, -6.0)]
    for rec in (records(ring, 0.25), records(cube, 0.5), records(cube + [[0.0, 1.5, -5.0]], [0.5] * 8 + [0.1])):
        refit_and_check(rec, rec, scalar_nodes=-1)
        refit_and_check(records(np.random.default_rng(4).normal(size=(rec.shape[0], 3)), 0.2), rec, scalar_nodes=-1)
        fit = refit_model(*one_node(rec.shape[0])[:2], rec)
        assert np.array_equal(bits(fit[0]), bits(refit_scalar(one_node(rec.shape[0])[1], rec, 0)))


def test_teleport_keeps_a_valid_tree():
    """A topology built for a completely different arrangement of the same count: meaningless groups, still bounds."""
    base = synthetic(1024, 15)
    refit_and_check(base, teleport_spheres(base, 10), scalar_nodes=8)
    base = synthetic(300, 16)
    refit_and_check(base, teleport_spheres(base, 11), scalar_nodes=-1)


@pytest.mark.parametrize("name", sorted(MOVING_BOUNDARY_MOTIONS))
def test_recorded_motion_crosses_the_form_boundary(name):
    """tests/test_moving_spheres_gpu.py forces a handoff to a topology built for these motions: its fresh build must land on
    the other side of the cell's LDS edge, and the cell's own refitted topology stays valid for the moved records."""
    seed, step, other = MOVING_BOUNDARY_MOTIONS[name]
    case = next(c for c in SPHERE_CASES if c.name == name)
    scene = case.scene()
    base = np.ascontiguousarray(scene.pack_spheres(), np.float32).reshape(-1, 8)
    _, _, m0 = build_hierarchy(base)
    moved = drift_spheres(base, step, seed)
    _, _, m1 = build_hierarchy(moved)
    here = expected_sphere_form(scene, case.B, sky=case.sky(), nodes=m0)
    there = expected_sphere_form(scene, case.B, sky=case.sky(), nodes=m1)
    assert (here.form, here.cap) == (case.form, case.cap)
    assert (there.form, there.cap) == other and there.kernel_id != here.kernel_id
    refit_and_check(base, moved)
