"""Design tool (CPU, float64): node/leaf tests per ray of the sphere hierarchy the LIBRARY builds (rt_build_hierarchy_ex:
the top-down tree with 0 passes, the optimised one otherwise), on primary, reflection and shadow rays of sampled 8x8 tiles.
Shadow rays are walked the way the kernel walks them (rt_bvh.hip: reversed_shadow_walk) when the scene takes the sign-aware
node test.  Both trees are walked with the same rays, so the difference carries far less sampling error than either figure;
the standard errors printed are over tiles (ratio estimator).  Calibration: on C3 the top-down figure has to reproduce the
counting builds of the parent tree (profiles/r09/C3-fast-v0-n1__counts.json: 39.49 tests, 28.17 inner + 11.32 leaf, 2.244
literal evaluations per ray, 5.56 rays per pixel) to within that error.

usage: python tools/bvh_opt_sim.py [C3|C5|C2|gauss:<seed>[:<n>]] [--tiles 96] [--passes 2] [--seed 1]
       gauss:<seed>: a scene of the kind tests/test_filter_fuzz_gpu.py draws (a normal cloud of n spheres with radii over a
       range of ratios, sometimes a ground sphere), 480x320, 5 bounces."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compute_raytracer_amd as rt                                                    # noqa: E402
from compute_raytracer_amd import abi                                                 # noqa: E402
from compute_raytracer_amd.scene_raytracing import BASELINE_CONFIGS, synthetic_spheres  # noqa: E402

LEAF = 0x80000000
S = 2.0 ** 40
EPS, KAPPA, KAPPA_H = 2.0 ** -17, 2.0 ** -16, 2.0 ** -14
REV_DELTA, REV_DELTA_REL, REV_SLACK, REV_SLACK_ABS = 0.0051, 2.0 ** -17, 2.0 ** -12, 2.0 ** -21


def build(rec, passes):
    """(centres (m+1, 3), k (m+1,), link (m+1,), m, info) of the library's tree; leaves as prep_spheres fills them."""
    n = rec.shape[0]
    cap = 2 * n + 64
    out, link, nodes = np.zeros((cap, 4), np.float32), np.zeros(cap, np.uint32), ctypes.c_uint32(0)
    info = (ctypes.c_double * 4)()
    fp = ctypes.POINTER(ctypes.c_float)
    abi.check(abi.load().rt_build_hierarchy_ex(rec.ctypes.data_as(fp), n, out.ctypes.data_as(fp), link.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                               cap, ctypes.byref(nodes), passes, info))
    m = nodes.value
    link = link[: m + 1].astype(np.int64)
    g = out[: m + 1, 0:3].astype(np.float64) / S
    k = out[: m + 1, 3].astype(np.float64) / (S * S)
    leaf = (link[:m] & LEAF) != 0
    sph = link[:m][leaf] & 0x7FFFFFFF
    c = rec[sph, 0:3].astype(np.float64)
    r2 = (rec[sph, 7] * rec[sph, 7]).astype(np.float64)
    g[:m][leaf] = c
    k[:m][leaf] = (c * c).sum(1) * (1.0 - EPS) - r2 * (1.0 + KAPPA)
    return g, k, link, m, dict(nodes_topdown=int(info[0]), moves=int(info[1]), cost_topdown=info[2], cost=info[3])


def walk(tree, o, d, madd, sgn):
    """trace_bvh's candidate selection for rays (o, d) (N, 3): inner tests, leaf tests, candidates per ray."""
    g, k, link, m, _ = tree
    N = o.shape[0]
    h = d * ((1.0 + KAPPA_H) / np.linalg.norm(d, axis=1))[:, None]
    p = (h * o).sum(1)
    q = (o * o).sum(1) * (1.0 - EPS) - madd
    is_leaf = np.concatenate([(link[:m] & LEAF) != 0, [False]])
    skip = np.where(is_leaf, 0, link // 4)
    j = np.zeros(N, np.int64)
    inner, leaf, cand = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    act = np.arange(N)
    while act.size:
        ja = j[act]
        gj = g[ja]
        b = p[act] - (h[act] * gj).sum(1)
        cp = k[ja] - 2.0 * (o[act] * gj).sum(1)
        bm = np.minimum(b, 0.0) if sgn else b
        ok = bm * bm - q[act] > cp
        lf = is_leaf[ja]
        leaf[act] += lf
        inner[act] += ~lf
        cand[act] += lf & ok
        j[act] = np.where(lf | ok, ja + 1, skip[ja])
        act = act[j[act] != m]
    return inner, leaf, cand


def nearest(C, R, o, d):
    """the literal test in f64: (t, sphere) of the nearest hit with 0.001 < t < 9999, sphere -1 for none"""
    oc = o[:, None, :] - C[None, :, :]
    b = (oc * d[:, None, :]).sum(2)
    cc = (oc * oc).sum(2) - R[None, :] ** 2
    disc = b * b - cc
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    t = np.where((disc > 0) & (t > 0.001) & (t < 9999.0), t, np.inf)
    i = t.argmin(1)
    tt = t[np.arange(o.shape[0]), i]
    return tt, np.where(np.isfinite(tt), i, -1)


def tile_rays(scene, W, H, B, tx, ty, sgn):
    """walk rays (o, d, madd) of one 8x8 tile, in the order a lane's state machine produces them, bounce by bounce"""
    cam, L = scene.camera, np.asarray(scene.light.position, np.float64)
    rec = scene.pack_spheres().astype(np.float64)
    C, R = rec[:, 0:3], np.abs(rec[:, 7])
    fw, rgt, up = (np.asarray(v, np.float64) for v in (cam.forwards, cam.right, cam.up))
    x = tx * 8 + np.tile(np.arange(8), 8)
    y = ty * 8 + np.repeat(np.arange(8), 8)
    keep = (x < W) & (y < H)
    x, y = x[keep], y[keep]
    d = fw[None] + ((x - W / 2) / W * 2)[:, None] * rgt[None] + ((H / 2 - y) / W * 2)[:, None] * up[None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.repeat(np.asarray(cam.position, np.float64)[None], len(x), 0)
    O, D, M = [], [], []
    for _ in range(B):
        if not len(o):
            break
        O.append(o); D.append(d); M.append(np.zeros(len(o)))
        t, i = nearest(C, R, o, d)
        hit = i >= 0
        o, d, t, i = o[hit], d[hit], t[hit], i[hit]
        P = o + t[:, None] * d
        nrm = (P - C[i]) / R[i][:, None]
        dl = P - L
        s = dl / np.linalg.norm(dl, axis=1)[:, None]
        if sgn:                                         # rt_bvh.hip: reversed_shadow_walk
            l1 = np.abs(dl).sum(1)
            la = l1 + np.abs(L).sum()
            delta = la * REV_DELTA_REL + REV_DELTA
            O.append(P + delta[:, None] * s); D.append(-s); M.append((l1 + delta) ** 2 * REV_SLACK + la * la * REV_SLACK_ABS)
        else:
            O.append(np.repeat(L[None], len(P), 0)); D.append(s); M.append(np.zeros(len(P)))
        d = d - 2.0 * (d * nrm).sum(1)[:, None] * nrm
        d /= np.linalg.norm(d, axis=1)[:, None]
        o = P
    return np.concatenate(O), np.concatenate(D), np.concatenate(M)


def gauss_scene(seed, n=200):
    rng = np.random.default_rng(seed)
    scale = float(10 ** rng.uniform(-1, 1))
    ratio = float(10 ** rng.uniform(0, 2.5))
    spheres = [rt.Sphere(rng.normal(size=3) * scale, scale * 0.25 / ratio * float(10 ** rng.uniform(0, np.log10(ratio))), rng.uniform(0.1, 1.0, 3))
               for _ in range(n)]
    if rng.random() < 0.5:
        Rg = scale * float(10 ** rng.uniform(1, 2))
        spheres.append(rt.Sphere(np.array([0, -Rg - scale, 0]), Rg, [0.8, 0.8, 0.8]))
    scene = rt.SceneRaytracing().createScene(spheres)
    scene.camera.position = [0.0, 0.5 * scale, 3.0 * scale]
    scene.camera.eulers = np.array([270.0, 95.0], np.float32)
    scene.camera.update()
    scene.light.position = [0.3 * scale, 2.5 * scale, 0.5 * scale]
    return scene


def ratio_se(num, den):
    """standard error over tiles of sum(num) / sum(den)"""
    k = len(den)
    r = num.sum() / den.sum()
    return float(np.sqrt(((num - r * den) ** 2).sum() / (k * (k - 1))) / den.mean()) if k > 1 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="C3")
    ap.add_argument("--tiles", type=int, default=96)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    if a.scene.startswith("gauss:"):
        f = a.scene.split(":")
        scene = gauss_scene(int(f[1]), int(f[2]) if len(f) > 2 else 200)
        W, H, B = 480, 320, 5
    else:
        cfg = BASELINE_CONFIGS[a.scene]
        scene = rt.SceneRaytracing().createScene(synthetic_spheres(cfg["spheres"], cfg["seed"]))
        W, H, B = cfg["width"], cfg["height"], cfg["bounces"]
    rec = np.ascontiguousarray(scene.pack_spheres(), np.float32).reshape(-1, 8)
    bound = (np.linalg.norm(rec[:, 0:3].astype(np.float64), axis=1) + np.abs(rec[:, 7])).max()
    reach = max(bound, np.linalg.norm(scene.camera.position), np.linalg.norm(scene.light.position))
    sgn = bool(2.0 * reach * 7.3e-7 < 5.0e-4)           # rt_api.hip: the sign-aware node test for compact scenes only
    trees = {"top-down": build(rec, 0), "optimised": build(rec, a.passes)}
    tw, th = (W + 7) // 8, (H + 7) // 8
    rng = np.random.default_rng(a.seed)
    pick = rng.choice(tw * th, size=min(a.tiles, tw * th), replace=False)
    rays, pixels = [], 0
    for t in pick:
        rays.append(tile_rays(scene, W, H, B, int(t % tw), int(t // tw), sgn))
        pixels += min(8, W - 8 * int(t % tw)) * min(8, H - 8 * int(t // tw))
    n_rays = np.array([len(r[0]) for r in rays], np.float64)
    print("%s: %d spheres, %dx%d, %d bounces, %s node test; %d tiles, %d rays (%.2f per pixel)"
          % (a.scene, rec.shape[0], W, H, B, "sign-aware" if sgn else "plain", len(pick), int(n_rays.sum()), n_rays.sum() / pixels))
    per_tile = {}
    for name, tree in trees.items():
        tot = np.zeros((len(rays), 3))
        wave_max = []
        for ti, (o, d, madd) in enumerate(rays):
            inner, leaf, cand = walk(tree, o, d, madd, sgn)
            tot[ti] = inner.sum(), leaf.sum(), cand.sum()
            tests = inner + leaf
            wave_max += [tests[s: s + 64].max() for s in range(0, len(tests) - 63, 64)]
        per_tile[name] = tot
        tests = tot[:, 0] + tot[:, 1]
        info = tree[4]
        print("  %-9s nodes %5d  cost %.6g  moves %4d | tests/ray %6.2f +- %.2f (inner %5.2f, leaf %5.2f)  candidates/ray %.3f +- %.3f  max of 64 rays %5.1f"
              % (name, tree[3], info["cost"] if name == "optimised" else info["cost_topdown"], info["moves"] if name == "optimised" else 0,
                 tests.sum() / n_rays.sum(), ratio_se(tests, n_rays), tot[:, 0].sum() / n_rays.sum(), tot[:, 1].sum() / n_rays.sum(),
                 tot[:, 2].sum() / n_rays.sum(), ratio_se(tot[:, 2], n_rays), float(np.mean(wave_max)) if wave_max else float("nan")))
    a0, a1 = per_tile["top-down"], per_tile["optimised"]
    dt = (a1[:, 0] + a1[:, 1]) - (a0[:, 0] + a0[:, 1])
    dc = a1[:, 2] - a0[:, 2]
    base = (a0[:, 0] + a0[:, 1]).sum() / n_rays.sum()
    print("  optimised - top-down, same rays: tests/ray %+.2f +- %.2f (%+.1f %%)  candidates/ray %+.3f +- %.3f"
          % (dt.sum() / n_rays.sum(), ratio_se(dt, n_rays), 100.0 * dt.sum() / n_rays.sum() / base, dc.sum() / n_rays.sum(), ratio_se(dc, n_rays)))


if __name__ == "__main__":
    main()
