"""Design tool (CPU, float64): the share of shadow rays that the sphere a reflection ray has just hit settles on its own
(rt_bvh.hip, claim D: the reference's shadow ray (L, s) enters that very sphere at a literal t_k <= |P - L| - dA, so its
nearest hit is not at the shaded point P and RK:165 returns minIntensity whatever else is in the scene).  The paths of
sampled 8x8 tiles are traced by brute force, bounce by bounce as the oracle's loop does (RK:113-144), and the predicate
is restated beside it; the standard errors printed are over tiles (ratio estimator).  The kernel's count of the same
quantity is mode 16 of the counting builds (tools/collect_counts.py: "shadow_decided").

usage: python tools/shadow_decided_sim.py [C3|C5|C2|gauss:<seed>[:<n>]] [--tiles 96] [--seed 1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compute_raytracer_amd as rt                                                    # noqa: E402
from compute_raytracer_amd.scene_raytracing import BASELINE_CONFIGS, synthetic_spheres  # noqa: E402
from bvh_opt_sim import gauss_scene, nearest, ratio_se                                # noqa: E402

U = 2.0 ** -24


def decided(C, R, i, L, P):
    """claim D for the points P shaded on spheres i: the literal test of sphere i on the shadow ray, and the margin"""
    dl = P - L
    ell = np.linalg.norm(dl, axis=1)
    s = dl / ell[:, None]
    oc = L[None] - C[i]
    b = (oc * s).sum(1)
    disc = b * b - ((oc * oc).sum(1) - R[i] ** 2)
    with np.errstate(invalid="ignore"):
        tk = -b - np.sqrt(disc)
    d_a = 0.0050011 + 16.0 * U * (ell + np.abs(L).sum())
    return (disc > 0) & (tk > 0.001) & (tk < 9999.0) & (tk + d_a <= ell * (1.0 - 16.0 * U))


def tile_counts(scene, W, H, B, tx, ty):
    """per bounce of one 8x8 tile: reflection rays, shadow rays, shadow rays settled by their own sphere"""
    cam, L = scene.camera, np.asarray(scene.light.position, np.float64)
    rec = scene.pack_spheres().astype(np.float64).reshape(-1, 8)
    C, R = rec[:, 0:3], np.abs(rec[:, 7])
    fw, rgt, up = (np.asarray(v, np.float64) for v in (cam.forwards, cam.right, cam.up))
    x = tx * 8 + np.tile(np.arange(8), 8)
    y = ty * 8 + np.repeat(np.arange(8), 8)
    keep = (x < W) & (y < H)
    x, y = x[keep], y[keep]
    d = fw[None] + ((x - W / 2) / W * 2)[:, None] * rgt[None] + ((H / 2 - y) / W * 2)[:, None] * up[None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.repeat(np.asarray(cam.position, np.float64)[None], len(x), 0)
    out = np.zeros((B, 3))
    for k in range(B):
        if not len(o):
            break
        t, i = nearest(C, R, o, d)
        hit = i >= 0
        out[k, 0] = len(o)
        o, d, t, i = o[hit], d[hit], t[hit], i[hit]
        P = o + t[:, None] * d
        out[k, 1] = len(P)
        out[k, 2] = decided(C, R, i, L, P).sum()
        nrm = (P - C[i]) / R[i][:, None]
        d = d - 2.0 * (d * nrm).sum(1)[:, None] * nrm
        d /= np.linalg.norm(d, axis=1)[:, None]
        o = P
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="C3")
    ap.add_argument("--tiles", type=int, default=96)
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
    tw, th = (W + 7) // 8, (H + 7) // 8
    pick = np.random.default_rng(a.seed).choice(tw * th, size=min(a.tiles, tw * th), replace=False)
    per = np.stack([tile_counts(scene, W, H, B, int(t % tw), int(t // tw)) for t in pick])     # (tiles, B, 3)
    refl, shad, dec = per[:, :, 0], per[:, :, 1], per[:, :, 2]
    rays = (refl + shad).sum(1)
    print("%s: %dx%d, %d bounces; %d tiles, %d rays (%d shadow rays)" % (a.scene, W, H, B, len(pick), int(rays.sum()), int(shad.sum())))
    print("  bounce " + " ".join("%6d" % k for k in range(B)))
    print("  share  " + " ".join("%5.1f%%" % (100.0 * dec[:, k].sum() / max(shad[:, k].sum(), 1.0)) for k in range(B)))
    print("  settled by their own sphere: %d = %.2f +- %.2f %% of shadow rays, %.2f +- %.2f %% of all rays"
          % (int(dec.sum()), 100.0 * dec.sum() / shad.sum(), 100.0 * ratio_se(dec.sum(1), shad.sum(1)),
             100.0 * dec.sum() / rays.sum(), 100.0 * ratio_se(dec.sum(1), rays)))


if __name__ == "__main__":
    main()
