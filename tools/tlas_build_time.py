"""Dev tool: what the device top-level build costs and what its tree saves a frame.

    python tools/tlas_build_time.py [--sizes 3,16,256,4096] [--frame-models 120] [--width 1344 --height 846]

1. Build time for procedural.triangle_scene(seed=5) with n instances, by each route, the host's clock around synchronous calls:
     rt_build_tlas        the C call alone (the matrices in host memory): prep, one read-back word per level, the result's
                          read-back and its commit;
     build_top_level      RendererRaytracing.build_top_level(): that call plus the read-back into the scene object;
     reference            the route without it -- scene.buildTopLevel() (instances.py: matrices, inverses, placeholder boxes, the
                          median-split tree, in numpy) and the three rt_write_* calls of its result;
     rt_build_tlas_host   the serial host model on the same arrays, no device.
   WARMUP calls, then REPS, alternating the routes; median, min, max in ms.  `levels`: depth + 1, the number of times the device
   build waits for one word.
2. Frame time of the scene with --frame-models models under the built top level against the reference's placeholder one, in one
   process, alternating: awaited frames (enqueue + wait, one at a time) and frames in flight (FLIGHT enqueued, one wait; per
   frame), the kernel time rt_stats reports, and rt_stats.rays of both.  The two frames are compared byte for byte.
One JSON line."""
import argparse
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
from compute_raytracer_amd.procedural import tri_buffers, triangle_scene  # noqa: E402

WARMUP, REPS, FLIGHT = 2, 9, 16
F = np.float32
FP = ctypes.POINTER(ctypes.c_float)
U32 = ctypes.POINTER(ctypes.c_uint32)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats3(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def build_times(n):
    scene, mat = triangle_scene(seed=5, n_models=n - 1)
    r = rt.RendererRaytracing(96, 64, scene, maxBounces=2).initialize(None, mat)
    lib, ctx = r._lib, r._ctx
    r.render()
    models = np.ascontiguousarray(scene.instances.matrices(), F)
    roots = np.ascontiguousarray([scene.meshes[k].root_node for k in scene.instances.mesh_index], np.uint32)
    nodes = np.ascontiguousarray(tri_buffers(scene, mat)["nodes"], F)
    cap = scene.tlasNodesMax
    info = abi.RtTlasInfo()
    out_t, out_b, out_l = np.zeros((cap, 8), F), np.zeros((n, 20), F), np.zeros(n, F)

    def call_only():
        abi.check(lib.rt_build_tlas(ctx, models.ctypes.data_as(FP), roots.ctypes.data_as(U32), n, cap, ctypes.byref(info)), ctx)

    def reference():
        scene.buildTopLevel()
        r.loaded = True
        r.recalculateScene()                                   # params and the three per-frame writes

    def host_model():
        rc = lib.rt_build_tlas_host(models.ctypes.data_as(FP), roots.ctypes.data_as(U32), n, nodes.ctypes.data_as(FP), nodes.shape[0],
                                    out_t.ctypes.data_as(FP), out_b.ctypes.data_as(FP), out_l.ctypes.data_as(FP), cap, None)
        assert rc == abi.RT_OK

    legs = {"rt_build_tlas_ms": call_only, "build_top_level_ms": r.build_top_level, "reference_ms": reference, "rt_build_tlas_host_ms": host_model}
    times = {k: [] for k in legs}
    for i in range(WARMUP + REPS):
        for k, fn in legs.items():
            t = timed(fn)[0]
            if i >= WARMUP:
                times[k].append(t)
    call_only()
    res = {"instances": n, "nodes": int(info.nodes_used), "levels": int(info.depth) + 1, "max_leaf": int(info.max_leaf)}
    res.update({k: stats3(v) for k, v in times.items()})
    assert np.array_equal(r.read_nodes(0, cap).view(np.uint32), out_t.view(np.uint32)), "the device and the host model left different nodes"
    r.close()
    return res


def frame_times(n_models, width, height):
    scene, mat = triangle_scene(seed=5, n_models=n_models)
    r = rt.RendererRaytracing(width, height, scene, maxBounces=4).initialize(None, mat)
    r.render()
    placeholder = dict(scene.frame), scene.tlasNodesUsed

    def use(which):
        if which == "placeholder":
            scene.frame, scene.tlasNodesUsed = dict(placeholder[0]), placeholder[1]
            r.recalculateScene()
        else:
            r.build_top_level()

    def awaited():
        r.enqueue()
        r.wait()

    def in_flight():
        for _ in range(FLIGHT):
            r.enqueue()
        r.wait()

    res, images = {}, {}
    times = {w: {"awaited_ms": [], "in_flight_ms": [], "kernel_ms": []} for w in ("placeholder", "built")}
    for i in range(WARMUP + REPS):
        for which in ("placeholder", "built"):
            use(which)
            awaited()                                          # the first frame after a scene write rebuilds what hangs on it
            a = timed(awaited)[0]
            k = r.stats()["kernel_ms"]
            b = timed(in_flight)[0] / FLIGHT
            if i >= WARMUP:
                times[which]["awaited_ms"].append(a)
                times[which]["kernel_ms"].append(k)
                times[which]["in_flight_ms"].append(b)
            if i == 0:
                awaited()
                images[which] = r.read_pixels().copy()
                res[which] = {"rays": int(r.stats()["rays"]), "tri_form": int(r.stats()["tri_form"]), "top_level_nodes": int(scene.tlasNodesUsed)}
    for which in times:
        res[which].update({k: stats3(v) for k, v in times[which].items()})
    res["frames_equal"] = bool(np.array_equal(images["placeholder"], images["built"]))
    res["instances"], res["width"], res["height"], res["flight"] = n_models + 1, width, height, FLIGHT
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3,16,256,4096")
    ap.add_argument("--frame-models", type=int, default=120)
    ap.add_argument("--width", type=int, default=1344)
    ap.add_argument("--height", type=int, default=846)
    a = ap.parse_args()
    out = {"build_id": abi.load().rt_build_id().decode(), "warmup": WARMUP, "reps": REPS, "ms": "median, min, max"}
    out["build"] = [build_times(int(n)) for n in a.sizes.split(",") if n]
    if a.frame_models > 0:
        out["frame"] = frame_times(a.frame_models, a.width, a.height)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
