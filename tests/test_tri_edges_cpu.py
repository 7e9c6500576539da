"""The inputs of the triangle edge-case tests (tests/tri_edge_common.py) really produce the cases they are made for, counted by a
numpy float32 restatement of the box test and of the triangle test over everything the walk can reach; and on the cases with
finite geometry and honest boxes the C oracle's nearest hit is the float32 brute force's, bit for bit, on every ray.  No GPU.

A floor is 50 occurrences per case, and 20 on either side where the case is a threshold.  Where the counter belongs to a class
of several scenes (the magnitudes: six scales and two translations) the floor is on their sum.

Two things the counters show about the reference itself (RK = the reference's ray-tracing kernel):
  * A ray that lies in the plane of a box face, with a zero direction component on that axis, misses that box: one slab product
    is 0 * inf = NaN, min / max drop it, and the other product's +-inf decides.  The walk therefore misses triangles on the
    shared edges of leaves whose boxes meet there, which a brute force over all pairs hits.  This is the reference's own
    behaviour (RK:395-410), the oracle restates it and so does the device: the brute force here counts only what the box
    tests let the walk reach (query_common.reach), and with that it agrees with the oracle on every ray.
  * det < 0.00001 (RK:359) and t > 0.001 (RK:315) are absolute: below a scale of about 2^-9 no triangle is ever accepted, whatever
    the direction's length.  Accepted hits with subnormal terms therefore come from subnormal offsets about the vertex at the
    origin (the threshold case), and the scaled-down scenes pin that both sides reject alike."""
import numpy as np
import pytest

import query_common as qc
import tri_edge_common as te
from query_common import F, bits

FLOOR, SIDE = 50, 20


FRAMES = ((72, 40), (144, 80))              # the frames tests/test_tri_edges_gpu.py shades: its own, and the supersampled one's samples


@pytest.fixture(scope="module")
def counts():
    """{case: count_hazards(case)}, computed once"""
    return {name: te.count_hazards(te.case(name)) for name in te.CASES}


def test_every_case_is_small():
    for name in te.CASES:
        c = te.case(name)
        # (four instances at most, but for the matrix class: its ten kinds of record are one record each)
        assert c.o.shape[0] <= 4000 and c.buf["triangles"].shape[0] <= 200 and c.buf["blas"].shape[0] <= (10 if name == "matrices" else 4), name
        assert c.buf["mesh_tex"].shape[0:2] == ((16, 16) if name == "uv16" else (16, 24))
        w = c.buf["triangles"][:, 39]
        assert (w == 1).any() and (w < 1).any()


def test_boxes_reach_nan_products_and_both_infinities(counts):
    k = counts["boxes"]
    print("boxes", k)
    assert k["slab_nan"] >= FLOOR and k["inv_pos_inf"] >= FLOOR and k["inv_neg_inf"] >= FLOOR
    c = te.case("boxes")
    assert (np.signbit(c.d) & (c.d == 0)).sum() >= FLOOR and (~np.signbit(c.d) & (c.d == 0)).sum() >= FLOOR     # -0.0 and +0.0
    nodes = c.buf["nodes"]
    flat = (nodes[:, 0:3] == nodes[:, 4:7]).any(axis=1) & (nodes[:, 0:3] != nodes[:, 4:7]).any(axis=1)
    assert (flat & (nodes[:, 7] == 0)).sum() >= 2 and (flat & (nodes[:, 7] > 0)).sum() >= 10                   # flat inner nodes and leaves


def test_thresholds_are_met_exactly_and_straddled(counts):
    k = counts["thresholds"]
    print("thresholds", k)
    assert k["u_zero"] >= FLOOR and k["u_det"] >= FLOOR and k["uv_det"] >= FLOOR
    assert k["det_below"] >= SIDE and k["det_above"] >= SIDE and k["det_below"] + k["det_above"] >= FLOOR
    assert k["t_min_below"] >= SIDE and k["t_min_above"] >= SIDE and k["t_min_below"] + k["t_min_above"] >= FLOOR
    assert k["t_ties"] >= FLOOR and k["t_near_nearest"] >= FLOOR          # ... and of the running nearest hit
    # a finite tmax (and tmin) one value below, at and above the nearest t: what limits_about gives the device tests
    assert min(k["limit_below"], k["limit_at"], k["limit_above"]) >= SIDE
    assert k["subnormal_accepted"] >= FLOOR and k["slab_subnormal"] >= FLOOR
    c = te.case("thresholds")                            # back faces: rays from behind the grid, and the quad that faces -z
    assert (c.d[:, 2] > 0).sum() >= FLOOR


def test_ties_and_near_ties_keep_the_hit_the_walk_meets_first(oracle):
    """The rays whose nearest hit is one of the coplanar copies (prims 76 / 77 in one leaf, 78 / 79 in two) or of the three
    triangles an ulp apart (80 - 82), through the walk restated ray by ray (nearest_by_walk): its t is the oracle's, the strict
    `<` of RK:380 keeps the lower slot inside a leaf, and across the two leaves the one the walk enters first -- 78."""
    c = te.case("thresholds")
    t_ref = oracle.trace_tri_rays(c.buf, c.o, c.d)
    _, inst, prim = te.nearest_hits(c)
    rays = np.nonzero((prim >= 76) & (prim <= 82) & (inst == 0))[0]
    won = {}
    for i in rays:
        t, bi, p = te.nearest_by_walk(c.buf, c.o[i], c.d[i])
        assert bits(F(t)) == bits(t_ref[i]) and bi == 0, i
        won[p] = won.get(p, 0) + 1
    print("winners", won)
    assert won.get(76, 0) >= FLOOR and won.get(78, 0) >= FLOOR and 77 not in won and 79 not in won
    assert won.get(81, 0) >= SIDE and won.get(80, 0) >= SIDE                 # an ulp nearer wins; where t rounds alike, the first met


def test_magnitudes_go_subnormal_and_overflow(counts):
    names = [n for n in te.CASES if te.HAZARD_CLASS[n] == 3]
    assert len(names) == 8
    total = {key: sum(counts[n][key] for n in names) for key in counts[names[0]]}
    print("magnitudes", {n: counts[n] for n in names})
    assert total["subnormal_terms"] >= FLOOR and total["overflowed"] >= FLOOR and total["slab_subnormal"] >= FLOOR
    assert counts["scale-60"]["hits"] == 0 and counts["scale+20"]["hits"] >= FLOOR and counts["far23"]["hits"] >= SIDE
    for n in names:                                      # direction lengths from 2^-40 to 2^40 on top of each scene's scale
        c = te.case(n)
        if n.startswith("scale"):
            s = 2.0 ** int(n[5:])
            with np.errstate(all="ignore"):
                ln = np.abs(c.d.astype(np.float64)).max(axis=1) / s
            assert ln.min() <= 2.0 ** -39 and ln.max() >= 2.0 ** 39


def test_matrices_cull_by_mirror_and_bring_nan_normals(counts):
    k = counts["matrices"]
    print("matrices", k)
    assert k["mirror_culled"] >= FLOOR
    for w, h in FRAMES:                                  # NaN normals a bounce reflects about: on the rays that are shaded
        shaded = te.shaded_hazards(te.case("matrices"), w, h)
        print("matrices", (w, h), shaded)
        assert shaded["nan_normal_hits"] >= FLOOR
    assert k["inv_pos_inf"] >= FLOOR and k["slab_nan"] >= FLOOR and k["nan_compare"] >= FLOOR
    m = te.case("matrices").buf["blas"]
    assert np.isnan(m[:, 0:16]).any(axis=1).sum() == 2 and np.isinf(m[:, 0:16]).any(axis=1).sum() == 1
    assert (m[:, [3, 7, 11]] != 0).any(axis=1).sum() >= 3                                                    # row 3 in use
    lin = m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        rank = [np.linalg.matrix_rank(a) if np.isfinite(a).all() else -1 for a in lin]
        dets = [np.linalg.det(a) if np.isfinite(a).all() else 0.0 for a in lin]
    assert 2 in rank and 0 in rank and min(dets) < 0
    scales = np.abs(lin[np.isfinite(lin).all(axis=(1, 2))]).max()
    assert scales >= 2.0 ** 12


def test_degenerate_geometry_reaches_nan_comparisons(counts):
    k = counts["degenerate"]
    print("degenerate", k)
    assert k["nan_compare"] >= FLOOR and k["overflowed"] >= FLOOR and k["slab_nan"] >= FLOOR
    c = te.case("degenerate")
    nodes, tris = c.buf["nodes"], c.buf["triangles"]
    corners = tris[:, [0, 1, 2, 12, 13, 14, 24, 25, 26]]
    assert np.isnan(corners).any() and np.isposinf(corners).any() and np.isneginf(corners).any() and (np.abs(corners) == F(3e38)).any()
    assert np.isnan(nodes[:, [0, 1, 2, 4, 5, 6]]).any() and (nodes[:, 0:3] > nodes[:, 4:7]).any()
    words = nodes[:, [3, 7]]
    assert np.isnan(words).any() and (words < 0).any() and (words != np.floor(words))[~np.isnan(words)].any() and (words >= 2.0 ** 32).any()


@pytest.mark.parametrize("name", ["uv24", "uv16"])
def test_texture_coordinates_take_both_clamps_and_nan(name):
    """Counted on the rays the device shades -- the camera rays of its frames, at their primary hits -- not on the constructed rays,
    which only the unshaded queries trace."""
    for w, h in FRAMES:
        k = te.shaded_hazards(te.case(name), w, h)
        print(name, (w, h), k)
        assert k["tex_clamp_hi"] >= FLOOR and k["tex_clamp_lo"] >= FLOOR and k["tex_nan"] >= FLOOR


@pytest.mark.parametrize("name", [n for n in te.CASES if te.HAZARD_CLASS[n] != 5])
def test_the_oracle_is_the_brute_force(oracle, name):
    """Every ray: the C oracle's nearest t against the float32 brute force over every (triangle, instance) pair the box tests let
    the walk reach.  (Without the box tests the brute force hits triangles on box faces the reference's walk misses: see above.)"""
    c = te.case(name)
    assert c.honest
    t_ref = oracle.trace_tri_rays(c.buf, c.o, c.d)
    with np.errstate(all="ignore"):
        best = qc.brute_triangles(c.buf, c.o, c.d, te.T_MIN, te.T_MAX, boxes=True)
    want = np.where(np.isfinite(best), best, F(-1.0)).astype(F)
    bad = bits(want) != bits(t_ref)
    assert not bad.any(), "%d of %d rays, first %s" % (int(bad.sum()), bad.size, np.nonzero(bad)[0][:5])


def test_the_plain_brute_force_sees_what_the_walk_misses(oracle):
    """The finding above, pinned: on the box case the brute force without box tests finds hits the oracle's walk does not, and
    every one of them is a ray with a zero direction component whose origin lies in a box's face plane."""
    c = te.case("boxes")
    t_ref = oracle.trace_tri_rays(c.buf, c.o, c.d)
    with np.errstate(all="ignore"):
        plain = qc.brute_triangles(c.buf, c.o, c.d, te.T_MIN, te.T_MAX)
    more = np.isfinite(plain) & ((t_ref == F(-1.0)) | (plain < t_ref))
    assert more.sum() >= FLOOR
    assert np.all((c.d[more] == 0).any(axis=1))
    assert not ((t_ref != F(-1.0)) & (~np.isfinite(plain) | (plain > t_ref))).any()      # never the other way round


def test_the_comparison_rule():
    cmp = te.Comparator()
    a = np.array([0.0, -0.0, np.nan, 1.0, np.nan], F)
    b = np.array([0.0, 0.0, -np.nan, 1.0, 1.0], F)
    assert cmp.differ(a, b).tolist() == [False, True, False, False, True] and cmp.nan_matches == 1
    payload = np.array([0x7FC00001, 0xFFC00000], np.uint32).view(F)
    assert cmp.same(payload, payload[::-1]) and cmp.nan_matches == 3
