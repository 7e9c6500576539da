"""Dev tool: what a frame of geometry planes costs by each route ("Geometry frames").

    python tools/gbuffer_rate.py            # rt_render_gbuffer_host (four planes, depth only), the device form, rt_pick
    python tools/gbuffer_rate.py pick       # rt_pick over every pixel alone: runs on a checkout that has no rt_render_gbuffer

Workloads: the reference's scene at 1344 x 846 (tests/golden/ref_scene.npz, bench.py --config REF's scene) and 1024 spheres
(BASELINE config C3's) at 3840 x 2160.  Host routes are synchronous, so they are timed on the host's clock around the call, output
arrays allocated once: WARMUP calls, then REPS calls, the median.  The device form (planes resident in device memory, no copy) is
timed with events around REPS calls on one stream, after WARMUP.  One JSON line."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compute_raytracer_amd as rt  # noqa: E402
from compute_raytracer_amd import abi  # noqa: E402

WARMUP, REPS = 3, 15


def median_ms(run):
    for _ in range(WARMUP):
        run()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        run()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)


def measure(scene, mat, bounces, W, H, pick_only):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=bounces).initialize(None, mat)
    r.recalculateScene()
    lib, ctx = r._lib, r._ctx
    n = W * H
    res = {"pixels": n}
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.ascontiguousarray(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.uint32))
    hits = np.zeros(n, dtype=abi.HIT_DTYPE)
    res["pick_ms"] = median_ms(lambda: abi.check(lib.rt_pick(ctx, xy.ctypes.data, n, hits.ctypes.data), ctx))
    if not pick_only:
        import torch
        host = {k: np.zeros((H, W) + abi.GBUFFER_PLANES[k][0], abi.GBUFFER_PLANES[k][1]) for k in abi.GBUFFER_PLANES}
        dev = {k: torch.from_numpy(a).to("cuda:0") for k, a in host.items()}
        for label, names in (("four", list(host)), ("depth", ["depth"])):
            gb = abi.RtGbuffer(**{k: host[k].ctypes.data for k in names})
            res["host_%s_ms" % label] = median_ms(lambda: abi.check(lib.rt_render_gbuffer_host(ctx, None, ctypes.byref(gb), n), ctx))
            out = {k: dev[k] for k in names}
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(WARMUP):
                    r.render_gbuffer(out=out)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    r.render_gbuffer(out=out)
                e1.record()
            side.synchronize()
            res["device_%s_ms" % label] = round(e0.elapsed_time(e1) / REPS, 4)
        # the routes agree (the planes of the last host call hold depth alone: ask again)
        g = r.render_gbuffer()
        assert np.array_equal(g["depth"].reshape(-1).view(np.uint32), hits["t"].view(np.uint32))
        assert np.array_equal(g["ids"].reshape(-1, 2), np.stack([hits["prim"], hits["instance"]], axis=1))
    res["hit_fraction"] = round(float((hits["prim"] >= 0).mean()), 3)
    r.close()
    return res


def main():
    pick_only = sys.argv[1:] == ["pick"]
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    cfg = rt.BASELINE_CONFIGS["C3"]
    out = {"build_id": abi.load().rt_build_id().decode(), "warmup": WARMUP, "reps": REPS, "ms": "median, min, max"}
    out["ref_1344x846"] = measure(rt.SceneRaytracing.from_packed(d), rt.Material.white(), int(d["maxBounces"]), int(d["W"]), int(d["H"]), pick_only)
    out["c3_3840x2160"] = measure(rt.synthetic_scene(cfg["spheres"], cfg["seed"]), None, cfg["bounces"], 3840, 2160, pick_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
