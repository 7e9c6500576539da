"""Dev tool: what an ambient-occlusion frame costs fused and composed ("Ambient-occlusion frames").

    python tools/ao_rate.py

Workload: the reference's scene at 1344 x 846 (tests/golden/ref_scene.npz), k = 16 directions of ao_directions, radius 1.0, tmin
0.001, the `ao` plane.  Two routes on one build, both wholly on the device, on one side stream:
  fused     render_ao(out={"ao": ...}): rt_render_ao, one kernel.
  composed  what a user had before it: render_gbuffer(out={"depth", "normal"}); the rays of include/rt355.h (rt_render_ao) as torch
            operations, one float32 operation each, from those planes and a table of the primary directions made once outside the
            timed loop; occluded() on the (n k, 8) ray tensor; a sum over k and the division.  A pixel whose primary ray missed
            gets rays with radius -1 (no walk gets past the root) and count 0.
Both produce the same counts (asserted, bit for bit on the ao plane).  Timed with events around REPS calls after WARMUP.  The bytes
per pixel are the least each route must move through device memory, from the shapes: planes, rays and answers written and read
once each; torch's temporaries are not counted.  One JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compute_raytracer_amd as rt  # noqa: E402
from compute_raytracer_amd import abi  # noqa: E402

WARMUP, REPS = 5, 40
K, RADIUS, TMIN = 16, 1.0, 0.001


def primary_directions(scene, W, H):
    """RK:76-86 in numpy float32, the oracle's order: (H * W, 3)"""
    F = np.float32
    p = scene.pack_params(2)
    fw, rgt, up = p[4:7], p[8:11], p[12:15]
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    hc = (xs.astype(F) - F(W) / F(2)) / F(W) * F(2)
    vc = (F(H) / F(2) - ys.astype(F)) / F(W) * F(2)
    d = np.stack([(fw[k] + hc * rgt[k]) + vc * up[k] for k in range(3)], axis=1).astype(F)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (d / ln[:, None]).astype(F)


def main():
    import torch
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    scene, W, H = rt.SceneRaytracing.from_packed(d), int(d["W"]), int(d["H"])
    r = rt.RendererRaytracing(W, H, scene, maxBounces=int(d["maxBounces"])).initialize(None, rt.Material.white())
    r.recalculateScene()
    n = W * H
    dev = torch.device("cuda:0")
    dirs = rt.ao_directions(K)
    t_dirs = torch.from_numpy(dirs).to(dev)
    cam = torch.from_numpy(np.asarray(scene.pack_params(2)[0:3], np.float32)).to(dev)
    pd = torch.from_numpy(primary_directions(scene, W, H)).to(dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    rays = torch.empty((n, K, 8), dtype=torch.float32, device=dev)
    occ = torch.empty((n * K,), dtype=torch.uint8, device=dev)
    fused_ao = torch.empty((H, W), dtype=torch.float32, device=dev)
    one, minus = torch.tensor(1.0, device=dev), torch.tensor(-1.0, device=dev)

    def fused():
        r.render_ao(dirs, radius=RADIUS, tmin=TMIN, out={"ao": fused_ao})
        return fused_ao

    def composed():
        r.render_gbuffer(out={"depth": depth, "normal": normal})
        t = depth.reshape(n, 1)
        nrm = normal.reshape(n, 4)[:, 0:3]
        p = cam + t * pd                                               # one multiply, one add per component
        nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        s = torch.where(nz >= 0, one, minus)
        a = minus / (s + nz)
        b = (nx * ny) * a
        T = torch.stack([one + ((s * nx) * nx) * a, s * b, (-s) * nx], dim=1)
        B = torch.stack([b, s + (ny * ny) * a, -ny], dim=1)
        dx, dy, dz = (t_dirs[:, c].reshape(1, K, 1) for c in range(3))
        rays[:, :, 0:3] = p.reshape(n, 1, 3)
        rays[:, :, 3] = TMIN
        rays[:, :, 4:7] = (dx * T.reshape(n, 1, 3) + dy * B.reshape(n, 1, 3)) + dz * nrm.reshape(n, 1, 3)
        rays[:, :, 7] = torch.where(t < 0, minus, RADIUS * one)         # a miss: no ray
        r.occluded(rays.reshape(n * K, 8), out=occ)
        count = occ.reshape(n, K).sum(dim=1, dtype=torch.int32)
        return ((K - count).to(torch.float32) / float(K)).reshape(H, W)

    res = {"build_id": abi.load().rt_build_id().decode(), "frame": [W, H], "k": K, "radius": RADIUS, "warmup": WARMUP, "reps": REPS}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a_fused = fused().clone()
        a_comp = composed().clone()
        side.synchronize()
        same = torch.equal(a_fused.view(torch.int32), a_comp.view(torch.int32))
        res["pixels_that_differ"] = int((a_fused != a_comp).sum())
        assert same, "the two routes differ on %d pixels" % res["pixels_that_differ"]
        for name, run in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
            for _ in range(WARMUP):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run()
            e1.record()
            side.synchronize()
            res[name + "_ms"] = round(e0.elapsed_time(e1) / REPS, 4)
    hit = float((depth > 0).float().mean())
    res["hit_fraction"] = round(hit, 3)
    res["ao_mean"] = round(float(a_fused.mean()), 4)
    # bytes per pixel through device memory, at the least: fused -- the ao plane written; composed -- depth and normal written and
    # read (2 x 20), the direction table read (12), k rays written and read (2 x 32 k), k answers written and read (2 k), ao written
    res["bytes_per_pixel"] = {"fused": 4, "composed": 2 * 20 + 12 + 2 * 32 * K + 2 * K + 4}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
