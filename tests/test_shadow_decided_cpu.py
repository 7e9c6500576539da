"""Claim D of rt_bvh.hip, exercised without a GPU: a shadow ray is settled without a traversal when the reference's own
literal test accepts the sphere k the reflection ray has just hit at a t_k that ends short of the shaded point P by the
margin of claim A (shadow_decided).  The predicate is restated here in fp32, statement for statement, and set against the
reference's full evaluation of RK:147-165 over ALL spheres (HK:308-318 in fp32, the oracle's operation order, nearest hit,
`diff < 0.005`): whenever the predicate fires the reference must return minIntensity -- whatever else is in the scene.

The shaded points are built to sit at the edge: at the terminator of a sphere where the chord of the shadow ray through it
is around 0.005, on spheres with radii from 0.002 to 0.02, displaced off the surface as a grazing hit displaces
fl(ro + t rd), with the light inside, on and far from spheres, on coincident spheres, on a huge ground sphere, in scenes
moved up to 2^20 from the origin, and in scenes with NaN and zero radii.  With the margin set to zero the same points must
produce wrong answers (the margin carries weight; the mutation is caught), and every scene class must have points on both
sides of the predicate."""
import numpy as np
import pytest

f32 = np.float32
DEC_DELTA, DEC_REL = f32(0.0050011), f32(2.0 ** -20)          # rt_bvh.hip: RT_BVH_DEC_DELTA, RT_BVH_DEC_REL


def dot32(a, b):                                               # rt_device.h: dot -- (x x' + y y') + z z', each op rounded
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def shadow_ray(L, P):
    """RK:147 as the kernel forms it: dl = P - L, len = length(dl), s = dl / len"""
    dl = (P - L[None, :]).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ln = np.sqrt(dot32(dl, dl)).astype(f32)
        s = (dl / ln[:, None]).astype(f32)
    return s, ln


def literal(C, r2, L, s):
    """HK:308-318 for every point's ray (L, s) and every sphere: (accepted, t), fp32, the oracle's operation order"""
    oc = (L[None, :] - C).astype(f32)                                              # (S, 3)
    a = dot32(s, s)                                                                # (N,)
    b = (f32(2.0) * dot32(s[:, None, :], oc[None, :, :])).astype(f32)              # (N, S)
    cc = (dot32(oc, oc) - r2).astype(f32)                                          # (S,)
    disc = ((b * b).astype(f32) - ((f32(4.0) * a).astype(f32)[:, None] * cc[None, :]).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ((-b - np.sqrt(disc).astype(f32)).astype(f32) / (f32(2.0) * a).astype(f32)[:, None]).astype(f32)
        hit = (disc > 0) & (t > f32(0.001)) & (t < f32(9999.0))
    return hit, t


def reference_lit(hit, t, L, s, P):
    """RK:155-159: is the nearest accepted hit within 0.005 of P?  (False: RK:165, minIntensity)"""
    tm = np.where(hit, t, f32(np.inf)).min(axis=1)
    any_hit = hit.any(axis=1)
    tm = np.where(any_hit, tm, f32(0.0)).astype(f32)
    hp = (L[None, :] + (tm[:, None] * s).astype(f32)).astype(f32)
    dv = (hp - P).astype(f32)
    with np.errstate(invalid="ignore"):
        diff = np.sqrt(dot32(dv, dv)).astype(f32)
        return any_hit & (diff < f32(0.005))


def decided(C, r2, k, L, s, ln, delta=DEC_DELTA, rel=DEC_REL):
    """shadow_decided (rt_bvh.hip), fp32, for the points' own spheres k"""
    light_l1 = f32(f32(abs(L[0]) + abs(L[1])) + abs(L[2]))
    a2 = dot32(s, s)
    oc = (L[None, :] - C[k]).astype(f32)
    b = (f32(2.0) * dot32(s, oc)).astype(f32)
    cc = (dot32(oc, oc) - r2[k]).astype(f32)
    disc = ((b * b).astype(f32) - ((f32(4.0) * a2).astype(f32) * cc).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tk = ((-b - np.sqrt(disc).astype(f32)).astype(f32) / (f32(2.0) * a2).astype(f32)).astype(f32)
        d_a = ((ln + light_l1).astype(f32).astype(np.float64) * np.float64(rel) + np.float64(delta)).astype(f32)    # fmaf
        l_lo = (ln * f32(f32(1.0) - rel)).astype(f32)
        return (disc > 0) & (b < 0) & (tk > f32(0.001)) & (tk < f32(9999.0)) & ((tk + d_a).astype(f32) <= l_lo)


# ---- the shaded points ------------------------------------------------------------------------------------------------
def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def points_on(C, r, L, rng, n, chords, displace):
    """n points, each on a sphere k of its own: where a ray from the light that cuts a chord h through k leaves it (the side
    facing away from the light; h from `chords`, as a fraction of the diameter when below 0, absolute otherwise) or enters it,
    or anywhere on the surface; then moved off the surface by one of `displace`."""
    C64, r64, L64 = C.astype(np.float64), np.abs(np.nan_to_num(r.astype(np.float64))), L.astype(np.float64)
    k = rng.integers(0, len(r), n)
    P = np.empty((n, 3))
    for i in range(n):
        c, rad = C64[k[i]], r64[k[i]]
        to = c - L64
        dist = np.linalg.norm(to)
        kind = i % 4
        if kind == 3 or dist < 1e-12 or not rad > 0:
            P[i] = c + unit(rng, 1)[0] * rad                              # anywhere (and all there is for a degenerate sphere)
            continue
        h = float(rng.choice(chords))
        h = min(-h * 2.0 * rad if h < 0 else h, 2.0 * rad)
        rho = np.sqrt(max(rad * rad - 0.25 * h * h, 0.0))                 # the line's distance from the centre
        if dist <= rho:                                                   # the light inside: no such line, take the surface
            P[i] = c + unit(rng, 1)[0] * rad
            continue
        w = rng.normal(size=3); w -= (w @ to) / dist ** 2 * to; w /= np.linalg.norm(w)
        # the line from L tangent to the ball of radius rho about c, in the plane (to, w)
        sin_a = rho / dist
        dirn = to / dist * np.sqrt(1.0 - sin_a * sin_a) + w * sin_a
        tc = dirn @ to
        P[i] = L64 + (tc + (0.5 * h if kind != 2 else -0.5 * h)) * dirn   # leaves (kinds 0, 1) or enters (kind 2) the sphere
    P += unit(rng, n) * rng.choice(displace, n)[:, None]
    return P.astype(f32), k


def run_class(name, C, r, L, seed, n, chords, displace):
    """-> (points, fired, wrong with the margin, wrong without it)"""
    rng = np.random.default_rng(seed)
    C, r, L = np.asarray(C, f32), np.asarray(r, f32), np.asarray(L, f32)
    r2 = (r * r).astype(f32)                                              # prep_spheres: geo.w = radius * radius
    P, k = points_on(C, r, L, rng, n, chords, displace)
    s, ln = shadow_ray(L, P)
    hit, t = literal(C, r2, L, s)
    lit = reference_lit(hit, t, L, s, P)
    fired = decided(C, r2, k, L, s, ln)
    bare = decided(C, r2, k, L, s, ln, delta=f32(0.0), rel=f32(0.0))
    wrong, wrong_bare = int((fired & lit).sum()), int((bare & lit).sum())
    print("%-22s %5d points: fired on %5.1f %%, lit %5.1f %%; wrong %d, wrong without the margin %d"
          % (name, n, 100.0 * fired.mean(), 100.0 * lit.mean(), wrong, wrong_bare))
    return n, int(fired.sum()), wrong, wrong_bare


CHORDS = [0.001, 0.003, 0.0045, 0.0049, 0.005, 0.0051, 0.0055, 0.006, 0.01, 0.05, -0.3, -0.9, -1.0]
DISPLACE = [0.0, 0.0, 1e-7, 1e-5, 1e-4, 1e-3, 0.004, 0.006]


def cloud(rng, n, lo, hi, spread=3.0, off=(0.0, 0.0, 0.0)):
    C = rng.normal(size=(n, 3)) * spread + np.asarray(off)
    r = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    return C, r


def scene_classes():
    rng = np.random.default_rng(7)
    out = []
    C, r = cloud(rng, 40, 0.199, 1.0)
    out.append(("terminator", C, r, [0.0, 5.0, 0.0], CHORDS, DISPLACE))
    C, r = cloud(rng, 60, 0.002, 0.02, spread=0.5)
    out.append(("radii 0.002-0.02", C, r, [0.2, 1.5, 0.1], CHORDS, DISPLACE))
    C, r = cloud(rng, 40, 0.05, 1.0)
    out.append(("displaced", C, r, [0.0, 5.0, 0.0], CHORDS, [1e-4, 1e-3, 0.004, 0.005, 0.006, 0.02, 0.1]))
    C, r = cloud(rng, 30, 0.1, 1.0)
    out.append(("light inside", C, r, C[3] + r[3] * np.array([0.2, -0.1, 0.3]), CHORDS, DISPLACE))
    out.append(("light at a centre", C, r, C[5], CHORDS, DISPLACE))
    out.append(("light on a surface", C, r, C[7] + r[7] * np.array([0.0, 1.0, 0.0]), CHORDS, DISPLACE))
    out.append(("light far", C, r, [3000.0, 8000.0, -2000.0], CHORDS + [-0.99], DISPLACE))
    C, r = cloud(rng, 12, 0.01, 1.0)
    C, r = np.concatenate([C, C, C]), np.concatenate([r, r, r * (1.0 + 1e-6)])
    out.append(("coincident", C, r, [0.0, 5.0, 0.0], CHORDS, DISPLACE))
    C, r = cloud(rng, 30, 0.05, 0.5, spread=2.0)
    C[:, 1] = r                                                           # resting on the ground y = 0
    C, r = np.concatenate([C, [[0.0, -1.0e4, 0.0]]]), np.concatenate([r, [1.0e4]])
    out.append(("huge ground", C, r, [1.0, 6.0, 2.0], CHORDS, DISPLACE))
    for e in (10, 16, 20):
        big = 2.0 ** e
        off = np.array([big, -0.5 * big, 0.25 * big])
        C, r = cloud(rng, 30, 0.05 * max(1.0, big / 2 ** 12), 2.0 * max(1.0, big / 2 ** 12), spread=3.0 * max(1.0, big / 2 ** 12), off=off)
        out.append(("offset 2^%d" % e, C, r, off + np.array([0.0, 5.0, 0.0]) * max(1.0, big / 2 ** 12), CHORDS, DISPLACE))
    C, r = cloud(rng, 30, 0.01, 1.0)
    r[::3] = 0.0
    r[1::3] = np.nan
    out.append(("NaN / zero radii", C, r, [0.0, 5.0, 0.0], CHORDS, DISPLACE))
    return out


CLASSES = scene_classes()


@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_fired_means_min_intensity(case):
    name, C, r, L, chords, displace = case
    n, fired, wrong, _ = run_class(name, C, r, L, seed=11, n=3000, chords=chords, displace=displace)
    assert wrong == 0                      # whenever the predicate fires, the reference returns minIntensity
    assert 0 < fired < n                   # and the class has points on both sides of it


def test_without_the_margin_the_answer_is_wrong():
    """delta_A' = 0: the literal t_k may end less than 0.005 short of P, the reference finds that hit `lit`."""
    bad = {}
    for name, C, r, L, chords, displace in CLASSES:
        _, _, wrong, wrong_bare = run_class(name, C, r, L, seed=11, n=3000, chords=chords, displace=displace)
        assert wrong == 0
        bad[name] = wrong_bare
    assert bad["terminator"] > 0 and bad["radii 0.002-0.02"] > 0 and bad["displaced"] > 0, bad
    assert sum(bad.values()) > 100, bad


def test_nan_leaves_the_lane_undecided():
    C = np.array([[0.0, 0.0, 0.0]], f32)
    L = np.array([0.0, 5.0, 0.0], f32)
    P = np.array([[0.0, -1.0, 0.0]], f32)
    s, ln = shadow_ray(L, P)
    k = np.array([0])
    assert decided(C, np.array([1.0], f32), k, L, s, ln)[0]                # the far pole of a unit sphere: fires
    nan = f32(np.nan)
    assert not decided(C, np.array([nan], f32), k, L, s, ln)[0]
    assert not decided(np.array([[nan, 0.0, 0.0]], f32), np.array([1.0], f32), k, L, s, ln)[0]
    assert not decided(C, np.array([1.0], f32), k, np.array([nan, 5.0, 0.0], f32), s, ln)[0]
    assert not decided(C, np.array([1.0], f32), k, L, np.array([[nan, -1.0, 0.0]], f32), ln)[0]
    assert not decided(C, np.array([1.0], f32), k, L, s, np.array([nan], f32))[0]
    s0, ln0 = shadow_ray(L, np.array([[3.0e19, -3.0e19, 0.0]], f32))       # |P - L|^2 overflows: len = inf, s = 0
    assert not decided(C, np.array([1.0], f32), k, L, s0, ln0)[0]
