"""Dev tool: the rate of closest-point queries (rt_closest_points) beside rt_trace_rays on the same scenes.

    python tools/closest_rate.py [--reps 9] [--grid 64]

Scenes:
  ref    the reference's scene (tests/golden/ref_scene.npz), its own top level (placeholder boxes);
  grid   --grid x --grid instances of procedural.triangle_scene's two sphere meshes on a square lattice 2.5 apart, each turned
         about Y by a seeded angle, and the floor; the top level built by rt_build_tlas (build_top_level()).
Points: the 2^20 points of a 1024 x 1024 lattice over the x and z extent of the scene box (the top-level root's, within 20 of the
camera for `ref`), y at a seeded height within the box, radius +inf.  Rays (the yardstick): 2^20 rays from those points in seeded
directions, through rt_trace_rays.
Each query runs on one stream from device memory: 2 warm-up calls, then --reps timed ones, each between two events; the median,
minimum and maximum are printed with the clock state bench.py reports (amd-smi, in a child process, before anything is timed).
The model's candidate tests per point (rt_closest_points_model) are counted on every 256th point, and its records are compared
with the device's there, bit for bit."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compute_raytracer_amd as rt  # noqa: E402
from compute_raytracer_amd import abi  # noqa: E402
from compute_raytracer_amd.procedural import obj_floor, obj_uv_sphere, tri_buffers  # noqa: E402

F = np.float32


def grid_scene(side, seed=5):
    rng = np.random.default_rng(seed)
    meshes = [rt.load_mesh(obj_uv_sphere(6, 8, 1.0), dict(color=[0.9, 0.5, 0.3, 0.6], alignBottom=True, scale=1.0)),
              rt.load_mesh(obj_uv_sphere(8, 11, 1.0, quads=False), dict(color=[0.3, 0.7, 0.9, 1.0], alignBottom=True, scale=0.7)),
              rt.load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 0.8], alignBottom=False, scale=1.25 * side + 2.0))]
    models = []
    for i in range(side * side - 1):
        x, z = (i % side - 0.5 * (side - 1)) * 2.5, -5.0 - (i // side) * 2.5
        models.append(dict(meshIndex=i % 2, position=[x, 0.0, z], eulers=[0, float(rng.uniform(0, 360)), 0]))
    models.append(dict(meshIndex=2, position=[0.0, 0.0, -5.0 - 1.25 * (side - 1)], eulers=[0, 0, 0]))
    return rt.SceneRaytracing().createScene([]).createTriangleScene(meshes, models), rt.Material.white()


def lattice(lo, hi, seed):
    rng = np.random.default_rng(seed)
    xs, zs = np.meshgrid(np.linspace(lo[0], hi[0], 1024), np.linspace(lo[2], hi[2], 1024))
    pts = np.zeros((1 << 20, 4), F)
    pts[:, 0], pts[:, 2] = xs.reshape(-1), zs.reshape(-1)
    pts[:, 1] = rng.uniform(lo[1], hi[1], 1 << 20)
    pts[:, 3] = np.inf
    d = rng.normal(size=(1 << 20, 3))
    rays = np.zeros((1 << 20, 8), F)
    rays[:, 0:3] = pts[:, 0:3]
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1)[:, None]
    rays[:, 3], rays[:, 7] = 0.001, 9999.0
    return pts, rays


def timed(torch, run, reps):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
            "per_s_median": round((1 << 20) / ms[len(ms) // 2] * 1e3)}


def model_sample(buf, pts):
    L = abi.load()
    sub = np.ascontiguousarray(pts[::256])
    arr = [np.ascontiguousarray(buf[k], F) for k in ("triangles", "tri_lookup", "nodes", "blas", "blas_lookup")]
    per = (40, 1, 8, 20, 1)
    out = np.zeros(sub.shape[0], dtype=abi.CLOSEST_DTYPE)
    tests = ctypes.c_uint64(0)
    args = []
    for a, k in zip(arr, per):
        args += [ctypes.c_void_p(a.ctypes.data), a.size // k]
    abi.check(L.rt_closest_points_model(ctypes.c_void_p(sub.ctypes.data), sub.shape[0], *args, None, 0, 0xFFFFFFFF,
                                        ctypes.c_void_p(out.ctypes.data), ctypes.byref(tests)))
    return out, tests.value / sub.shape[0]


def measure(torch, name, scene, mat, lo, hi, reps, build):
    r = rt.RendererRaytracing(96, 64, scene, maxBounces=2).initialize(None, mat)
    r.recalculateScene()
    info = r.build_top_level() if build else None
    buf = tri_buffers(scene, mat)
    pts, rays = lattice(lo, hi, 17)
    dp, dr = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(rays).to("cuda:0")
    out_p = torch.empty((1 << 20, 8), dtype=torch.float32, device="cuda:0")
    out_r = torch.empty((1 << 20, 8), dtype=torch.float32, device="cuda:0")
    res = {"scene": name, "instances": len(scene.instances), "lookup_slots": int(len(buf["tri_lookup"])), "top_level": info}
    res["closest_points"] = timed(torch, lambda: r.closest_points(dp, out=out_p), reps)
    res["trace_rays"] = timed(torch, lambda: r.trace_rays(dr, out=out_r), reps)
    got = np.ascontiguousarray(out_p.cpu().numpy()).view(abi.CLOSEST_DTYPE).reshape(-1)
    res["ray_hit_fraction"] = round(float((out_r[:, 3].view(torch.int32) >= 0).sum().item()) / (1 << 20), 3)
    want, per_point = model_sample(buf, pts)
    res["model_tests_per_point"] = round(per_point, 2)
    res["device_equals_model_on_sample"] = bool(got[::256].tobytes() == want.tobytes())
    res["mean_dist"] = round(float(np.sqrt(got["dist2"].astype(np.float64)).mean()), 3)
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--grid", type=int, default=64)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import bench
    out = {"build_id": abi.load().rt_build_id().decode(), "clocks": bench.gpu_clocks(), "reps": a.reps}
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    scene = rt.SceneRaytracing.from_packed(d)
    root = np.asarray(scene.pack_tlas_nodes(), np.float64).reshape(-1, 8)[0]
    cam = scene.pack_params(4)[0:3].astype(np.float64)
    out["ref"] = measure(torch, "ref", scene, rt.Material.white(), np.maximum(root[0:3], cam - 20.0), np.minimum(root[4:7], cam + 20.0),
                         a.reps, False)
    scene, mat = grid_scene(a.grid)
    half = 1.25 * a.grid + 2.0
    lo = np.array([-half, 0.0, -5.0 - 1.25 * (a.grid - 1) - half])
    hi = np.array([half, 3.0, -5.0 - 1.25 * (a.grid - 1) + half])
    out["grid"] = measure(torch, "grid %d x %d" % (a.grid, a.grid), scene, mat, lo, hi, a.reps, True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
