"""Claim D of rt_bvh.hip without root or quotient, exercised without a GPU.  shadow_decided no longer forms
t_k = (-b - sqrt(disc)) / (2a): it decides `0.001 < t_k`, `t_k < 9999` and `t_k + d_a <= l_lo` by comparing products and
squares of -b, disc and 2a.  The new predicate is restated here in fp32, operation for operation, and held against

  * the reference's full evaluation of RK:147-165 over ALL spheres (never a yes where the reference says `lit`), and
  * the literal predicate it replaces (tests/test_shadow_decided_cpu.py: decided) -- never a yes where that one says no,

on the thirteen scene classes of that test and on points built AT the new predicate's edges: t_k within a few ulps of
l_lo - d_a, of 0.001 and of 9999, rays that graze (disc around 0), and records with NaN and infinite entries.  With the
comparison margins set to zero the same points must give yeses the literal predicate does not give; with claim A's margin
gone as well, yeses where the reference says `lit`.  The share of literal yeses that the one-sided form gives up is printed
per class and bounded where the class is not built to sit on an edge.

The suspended-walk predicate (shadow_blocked: a shadow ray that already holds a literal hit at t with (t + d)^2 <= |P - L|^2
is over) is held against the reference the same way, for every literally accepted sphere of every point."""
import numpy as np
import pytest

from test_shadow_decided_cpu import CLASSES, DEC_DELTA, DEC_REL, cloud, decided, dot32, literal, points_on, reference_lit, shadow_ray, unit

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")      # the non-finite records overflow and cancel on purpose
f32, f64 = np.float32, np.float64
U = 2.0 ** -24
# rt_bvh.hip: RT_BVH_CMP_*
CMP_REL, CMP_DISC, CMP_TMIN, CMP_TMAX, CMP_DISC_MIN = f32(2.0 ** -19), f32(2.0 ** -21), f32(0.0010001), f32(9998.0), f32(2.0 ** -100)
MARGINS = dict(rel=CMP_REL, dsc=CMP_DISC, tmin=CMP_TMIN, dmin=CMP_DISC_MIN, delta=DEC_DELTA, drel=DEC_REL)
# the comparisons bare: the bounds of the literal predicate, nothing for the roundings of root, quotient, product and square
NO_CMP_MARGINS = dict(rel=DEC_REL, dsc=f32(0.0), tmin=f32(0.001), dmin=f32(0.0), delta=DEC_DELTA, drel=DEC_REL)
NO_MARGINS = dict(rel=f32(0.0), dsc=f32(0.0), tmin=f32(0.001), dmin=f32(0.0), delta=f32(0.0), drel=f32(0.0))


def fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds once there and once to float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def l1_of(L):
    return f32(f32(abs(L[0]) + abs(L[1])) + abs(L[2]))


def compared(C, r2, k, L, s, ln, rel, dsc, tmin, dmin, delta, drel):
    """shadow_decided (rt_bvh.hip), fp32, statement for statement, for the points' own spheres k"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        a2 = dot32(s, s)
        oc = (L[None, :] - C[k]).astype(f32)
        b = (f32(2.0) * dot32(s, oc)).astype(f32)
        cc = (dot32(oc, oc) - r2[k]).astype(f32)
        disc = ((b * b).astype(f32) - ((f32(4.0) * a2).astype(f32) * cc).astype(f32)).astype(f32)
        A, nb = (f32(2.0) * a2).astype(f32), -b
        d_a = fma32((ln + l1_of(L)).astype(f32), drel, delta)
        B = fma32(ln, f32(f32(1.0) - rel), -d_a)
        v = fma32(-A, tmin, nb)
        w = fma32(-A, B, nb)
        accepted = (disc > dmin) & (b < 0)
        above = (v > 0) & ((v * v).astype(f32) > (disc * f32(f32(1.0) + dsc)).astype(f32))
        below = (B < CMP_TMAX) & ((w <= 0) | ((w * w).astype(f32) <= (disc * f32(f32(1.0) - dsc)).astype(f32)))
        return accepted & above & below


def blocked(L, P, t, rel=CMP_REL, delta=DEC_DELTA):
    """shadow_blocked (rt_bvh.hip), fp32: t (N, S) are literal hits of the rays towards P (N, 3)"""
    with np.errstate(invalid="ignore", over="ignore"):
        dl = (P - L[None, :]).astype(f32)
        l1 = ((np.abs(dl[:, 0]) + np.abs(dl[:, 1])).astype(f32) + np.abs(dl[:, 2])).astype(f32)
        d = fma32((l1 + l1_of(L)).astype(f32), rel, delta)
        x = (t + d[:, None]).astype(f32)
        return (x * x).astype(f32) < dot32(dl, dl)[:, None]


def judge(name, C, r, L, P, k):
    """-> dict of counts for points P with own spheres k in the scene (C, r) lit from L"""
    C, r, L, P = np.asarray(C, f32), np.asarray(r, f32), np.asarray(L, f32), np.asarray(P, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = (r * r).astype(f32)
    s, ln = shadow_ray(L, P)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        hit, t = literal(C, r2, L, s)
        lit = reference_lit(hit, t, L, s, P)
    old = decided(C, r2, k, L, s, ln)
    new = compared(C, r2, k, L, s, ln, **MARGINS)
    bare = compared(C, r2, k, L, s, ln, **NO_CMP_MARGINS)
    none = compared(C, r2, k, L, s, ln, **NO_MARGINS)
    blk = blocked(L, P, t) & hit
    blk0 = blocked(L, P, t, rel=f32(0.0), delta=f32(0.0)) & hit
    res = dict(n=len(P), old=int(old.sum()), new=int(new.sum()), lost=int((old & ~new).sum()),
               yes_lit=int((new & lit).sum()), yes_old_no=int((new & ~old).sum()),
               bare_old_no=int((bare & ~old).sum()), none_lit=int((none & lit).sum()),
               blocked=int(blk.any(axis=1).sum()), blocked_lit=int((blk.any(axis=1) & lit).sum()), blocked0_lit=int((blk0.any(axis=1) & lit).sum()))
    print("%-22s %5d points: literal yes %5d, compared yes %5d, given up %4d (%.2f %% of the literal yeses); yes & lit %d, yes & literal no %d; "
          "bare comparisons: yes & literal no %d; no margins: yes & lit %d; blocked %d, & lit %d, without margin & lit %d"
          % (name, res["n"], res["old"], res["new"], res["lost"], 100.0 * res["lost"] / max(res["old"], 1), res["yes_lit"], res["yes_old_no"],
             res["bare_old_no"], res["none_lit"], res["blocked"], res["blocked_lit"], res["blocked0_lit"]))
    return res


_SEEN = {}


def class_result(case):
    name, C, r, L, chords, displace = case
    if name not in _SEEN:                                                    # computed once, shared by the tests below
        rng = np.random.default_rng(11)
        C32, r32, L32 = np.asarray(C, f32), np.asarray(r, f32), np.asarray(L, f32)
        P, k = points_on(C32, r32, L32, rng, 3000, chords, displace)
        _SEEN[name] = judge(name, C32, r32, L32, P, k)
    return _SEEN[name]


@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_scene_classes_one_sided(case):
    res = class_result(case)
    assert res["yes_lit"] == 0                       # a yes means the reference returns minIntensity
    assert res["yes_old_no"] == 0                    # ... and is a yes of the literal predicate
    assert res["blocked_lit"] == 0                   # a blocker short of P by the margin: the same
    assert 0 < res["new"] < res["n"]                 # points on both sides
    # What is given up lies within the margins of an edge: 32u l + 8u S / A in t_k, S / A the half chord of the line through
    # k -- some 2e-5 for the spheres of these scenes, a fifth of the 1e-4 steps of CHORDS around 0.005, and 5e-3 on the ground
    # sphere of radius 1e4, whose own literal t_k is no better than 6e-4.  Two per cent of a class bounds both.
    assert res["lost"] <= max(3, res["old"] // 50), res


# ---- points at the edges of the comparisons ---------------------------------------------------------------------------
def ray_through(rng, L, c, rad, frac):
    """a unit direction from L whose line passes c at distance frac * rad, and the parameters of the line's two crossings"""
    to = c - L
    dist = np.linalg.norm(to)
    w = rng.normal(size=3); w -= (w @ to) / dist ** 2 * to; w /= np.linalg.norm(w)
    sin_a = min(frac * rad / dist, 1.0)
    d = to / dist * np.sqrt(1.0 - sin_a * sin_a) + w * sin_a
    tc = d @ to
    half = np.sqrt(max(rad * rad - (frac * rad) ** 2, 0.0))
    return d, tc - half, tc + half


def edge_upper(seed, n=1500, L=(0.3, 5.0, -0.2), off=(0.0, 0.0, 0.0), lo=0.05, hi=1.0, spread=3.0):
    """P = L + l d with l within 64u of the l at which t_k + d_a = l (1 - 16u): the edge of `t_k + d_a <= l_lo`"""
    rng = np.random.default_rng(seed)
    C, r = cloud(rng, 40, lo, hi, spread=spread, off=off)
    L = np.asarray(L, f64) + np.asarray(off)
    l1 = np.abs(L).sum()
    k = rng.integers(0, len(r), n)
    D, T = np.empty((n, 3)), np.empty(n)
    for i in range(n):
        D[i], T[i], _ = ray_through(rng, L, C[k[i]], r[k[i]], rng.uniform(0.0, 0.999))
    edge = lambda t: (t + 0.0050011 + 16 * U * l1) / (1.0 - 32 * U)
    # the edge is where the LITERAL t_k sits, and far from the light that one is off the geometric entry by whole units: the
    # points are placed by geometry first, then again along the same directions by the float32 t_k that placement gave
    C32, r32, L32 = C.astype(f32), r.astype(f32), L.astype(f32)
    s, _ = shadow_ray(L32, (L + D * edge(T)[:, None]).astype(f32))
    with np.errstate(invalid="ignore"):
        t32 = literal(C32, (r32 * r32).astype(f32), L32, s)[1][np.arange(n), k].astype(f64)
    T = np.where(np.isfinite(t32), t32, T)
    P = L + D * (edge(T) * (1.0 + rng.uniform(-64, 64, n) * U))[:, None]
    return C, r, L, P, k


def edge_tmin(seed, n=1500):
    """the light 0.001 (1 +- 2e-6) outside small spheres near the origin, where float32 resolves an ulp of 0.001"""
    rng = np.random.default_rng(seed)
    L = np.zeros(3)
    d = unit(rng, n)
    r = 10.0 ** rng.uniform(np.log10(0.003), np.log10(0.01), n)
    gap = 0.001 * (1.0 + rng.uniform(-2e-6, 2e-6, n))
    gap[::7] = 0.0010001 * (1.0 + rng.uniform(-2e-6, 2e-6, len(gap[::7])))           # and around the comparison's own bound
    C = d * (r + gap)[:, None]
    P = d * (2.0 * r + gap + 0.1)[:, None]                                           # well beyond the sphere
    return C, r, L, P, np.arange(n)


def edge_tmax(seed, n=1200):
    """spheres entered at 9999 (1 +- 4e-6) and at 9998 (1 +- 4e-6) from the light, the shaded point well beyond"""
    rng = np.random.default_rng(seed)
    L = np.zeros(3)
    d = unit(rng, n)
    r = rng.uniform(20.0, 80.0, n)
    t_in = np.where(np.arange(n) % 2 == 0, 9999.0, 9998.0 + 0.0050011 + 32 * U * 12000.0) * (1.0 + rng.uniform(-4e-6, 4e-6, n))
    C = d * (t_in + r)[:, None]
    far = np.where(np.arange(n) % 2 == 0, 12000.0, 0.0)
    # odd points: P so that B = l (1 - 32u) - d_a sits around 9998 while t_k is well below it -- the `B < 9998` edge
    P = d * np.where(np.arange(n) % 2 == 0, far, (9998.0 + 0.0050011) * (1.0 + rng.uniform(-4e-6, 4e-6, n)))[:, None]
    C[1::2] = d[1::2] * (5000.0 + r[1::2])[:, None]
    return C, r, L, P, np.arange(n)


def edge_graze(seed, n=1500):
    """rays whose line passes the sphere at r (1 +- 3e-7): disc around zero, of either sign"""
    rng = np.random.default_rng(seed)
    C, r = cloud(rng, 40, 0.05, 1.0)
    L = np.array([0.0, 5.0, 0.0])
    k = rng.integers(0, len(r), n)
    P = np.empty((n, 3))
    for i in range(n):
        d, t_in, t_out = ray_through(rng, L, C[k[i]], r[k[i]], min(1.0 + rng.uniform(-3e-7, 3e-7), 1.0))
        P[i] = L + d * (t_out + rng.choice([0.004, 0.0052, 0.01, 1.0]))
    return C, r, L, P, k


def edge_nonfinite(seed, n=1200):
    """records with NaN and infinite entries among ordinary ones; every fourth point has such a sphere as its own"""
    rng = np.random.default_rng(seed)
    C, r = cloud(rng, 40, 0.05, 1.0)
    L = np.array([0.0, 5.0, 0.0])
    P, k = points_on(C.astype(f32), r.astype(f32), L.astype(f32), rng, n, [0.0049, 0.0051, 0.01, -0.5, -1.0], [0.0, 1e-5, 1e-3])
    bad = [(np.nan, 0, 0, 1), (np.inf, 0, 0, 1), (0, -np.inf, 0, 1), (0, 0, 0, np.inf), (0, 0, 0, np.nan), (3e19, 0, 0, 1), (0, 0, 0, 2e19),
           (np.inf, np.inf, np.inf, np.inf), (1e38, 1e38, 0, 1e38), (0, 0, 0, 1e-30)]
    C = np.concatenate([C, [b[:3] for b in bad]])
    r = np.concatenate([r, [b[3] for b in bad]])
    k[::4] = 40 + rng.integers(0, len(bad), len(k[::4]))
    return C, r, L, P.astype(f64), k


EDGES = {"t_k + d_a at l_lo": lambda: edge_upper(21), "the same, light far": lambda: edge_upper(22, L=(3000.0, 8000.0, -2000.0)),
         "the same, offset 2^16": lambda: edge_upper(23, off=(65536.0, -32768.0, 16384.0), lo=0.8, hi=32.0, spread=48.0, L=(0.0, 80.0, 0.0)),
         "t_k at 0.001": lambda: edge_tmin(24), "t_k at 9999": lambda: edge_tmax(25), "grazing": lambda: edge_graze(26),
         "NaN / inf records": lambda: edge_nonfinite(27)}
_EDGE_SEEN = {}


def edge_result(name):
    if name not in _EDGE_SEEN:
        C, r, L, P, k = EDGES[name]()
        _EDGE_SEEN[name] = judge(name, C, r, L, P, k)
    return _EDGE_SEEN[name]


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_one_sided(name):
    res = edge_result(name)
    assert res["yes_lit"] == 0
    assert res["yes_old_no"] == 0
    assert res["blocked_lit"] == 0
    if name != "NaN / inf records":
        assert 0 < res["old"] < res["n"], res        # the literal predicate is on both sides at these points ...
    if name not in ("grazing", "NaN / inf records"):
        assert res["lost"] > 0, res                  # ... and the edge is close enough for the one-sided form to give some up


def test_without_the_margins_the_answers_are_wrong():
    """The comparisons bare say yes where the literal t_k, rounded three times, says no; with claim A's margin gone as well,
    where the reference finds the point lit.  The suspended-walk comparison without its margin: the same."""
    bare = {n: edge_result(n)["bare_old_no"] for n in EDGES}
    assert bare["t_k + d_a at l_lo"] > 0 and bare["t_k at 0.001"] > 0, bare
    none = sum(class_result(c)["none_lit"] for c in CLASSES)
    blk0 = sum(class_result(c)["blocked0_lit"] for c in CLASSES)
    assert none > 100 and blk0 > 100, (none, blk0)


def test_given_up_share_is_reported():
    """On the thirteen scene classes (3,000 points each, a third of them at terminators and thin chords) the one-sided form
    keeps all but a sliver of the literal yeses; on the edge sets, built within 64u of a bound, it gives up a large share."""
    old = sum(class_result(c)["old"] for c in CLASSES)
    lost = sum(class_result(c)["lost"] for c in CLASSES)
    e_old = sum(edge_result(n)["old"] for n in EDGES)
    e_lost = sum(edge_result(n)["lost"] for n in EDGES)
    print("scene classes: %d of %d literal yeses given up (%.3f %%); edge sets: %d of %d (%.1f %%)"
          % (lost, old, 100.0 * lost / old, e_lost, e_old, 100.0 * e_lost / e_old))
    assert lost <= old // 200                        # half a per cent over all classes (see test_scene_classes_one_sided)
    assert e_lost > 0


def test_nan_leaves_the_lane_undecided():
    C = np.array([[0.0, 0.0, 0.0]], f32)
    L = np.array([0.0, 5.0, 0.0], f32)
    P = np.array([[0.0, -1.0, 0.0]], f32)
    s, ln = shadow_ray(L, P)
    k = np.array([0])
    one = np.array([1.0], f32)
    yes = lambda *a: bool(compared(*a, **MARGINS)[0])
    assert yes(C, one, k, L, s, ln)                                          # the far pole of a unit sphere: yes
    nan, inf = f32(np.nan), f32(np.inf)
    for bad in (nan, inf, -inf):
        assert not yes(C, np.array([bad], f32), k, L, s, ln)
        assert not yes(np.array([[bad, 0.0, 0.0]], f32), one, k, L, s, ln)
        assert not yes(C, one, k, np.array([bad, 5.0, 0.0], f32), s, ln)
        assert not yes(C, one, k, L, np.array([[bad, -1.0, 0.0]], f32), ln)
        assert not yes(C, one, k, L, s, np.array([bad], f32))
        assert not blocked(L, np.array([[bad, -1.0, 0.0]], f32), np.array([[1.0]], f32))[0, 0]
        assert not blocked(np.array([bad, 5.0, 0.0], f32), P, np.array([[1.0]], f32))[0, 0]
        assert not blocked(L, P, np.array([[nan]], f32))[0, 0]
    s0, ln0 = shadow_ray(L, np.array([[3.0e19, -3.0e19, 0.0]], f32))         # |P - L|^2 overflows: len = inf, s = 0
    assert not yes(C, one, k, L, s0, ln0)
    assert blocked(L, P, np.array([[4.0]], f32))[0, 0] and not blocked(L, P, np.array([[5.996]], f32))[0, 0]
