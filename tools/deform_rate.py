"""Dev tool: what one deformation step of a mesh costs when its vertices live in a torch tensor on the device ("Device mesh
deformation").

    python tools/deform_rate.py [--big PACKED.npz] [--save-big PACKED.npz]

A step moves every vertex of one mesh (two poses, alternating; the (T, 3, 3) float32 corner tensors are made on the device before
the clock starts) and ends with the bottom-level trees refitted.  No frame is rendered: both routes leave the same bytes.
  (a) the route without rt_deform_triangles: tensor.cpu() -> the corners repacked on the host into the mesh's 40-float records ->
      update_triangles() -> refit();
  (b) deform(tensor), which is rt_deform_triangles on torch's current stream, the read-back of the records into the scene object
      and refit();
  (b, C ABI) rt_deform_triangles + rt_refit_blas alone, for callers that keep no host mirror.
Meshes: the 176-triangle sphere of the tests' scene, the largest mesh of the reference's scene (tests/golden/ref_scene.npz), and a
UV sphere of 114,688 triangles made by the project's loader and SAH builder (about a minute and a half of host time: --save-big
keeps the packed scene, --big loads it again).
All routes run in one process on one build, interleaved (a, b, c, a, b, c, ...); the host's clock around the calls, which are
synchronous; WARMUP steps of each, then REPS, the median with the minimum and maximum.  Both routes are checked to leave the same
triangle records and the same nodes.  One JSON line."""
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

WARMUP, REPS = 3, 15
W, H = 64, 48                                        # no frame is timed: the colour buffers stay small
F = np.float32
COLS = (slice(0, 3), slice(12, 15), slice(24, 27))


def u32f(f):
    f = float(f)
    return 0 if not f > 0.0 else (4294967295 if f >= 4294967040.0 else int(f))


def big_scene():
    """one UV sphere of 224 x 256 quads (114,688 triangles) and the floor, through the loader and the SAH builder"""
    from compute_raytracer_amd.procedural import obj_floor, obj_uv_sphere
    meshes = [rt.load_mesh(obj_uv_sphere(224, 256, 1.0), dict(color=[0.9, 0.5, 0.3, 0.6], alignBottom=True, scale=1.0)),
              rt.load_mesh(obj_floor(1.0), dict(color=[1.0, 1.0, 1.0, 0.8], alignBottom=False, scale=12))]
    models = [dict(meshIndex=0, position=[0.0, 0.0, -5.0], eulers=[0, 30.0, 0]), dict(meshIndex=1, position=[0, 0, -5], eulers=[0, 0, 0])]
    scene = rt.SceneRaytracing().createScene([])
    scene.createTriangleScene(meshes, models)
    return scene


def largest_mesh(scene):
    """(first triangle, count) of the mesh with the most triangles: the longest run of lookup slots under one root"""
    lookup = np.asarray(scene.pack_tri_lookup(), F)
    blas = np.ascontiguousarray(scene.pack_blas_nodes(), F)
    base = scene.tlasNodesMax
    whole = np.zeros((base + blas.shape[0], 8), F)
    whole[base:] = blas
    roots = np.array(sorted(set(u32f(b[16]) for b in np.asarray(scene.pack_blas(), F).reshape(-1, 20))), np.uint32)
    plan = np.zeros((whole.shape[0], 3), np.uint32)
    n_plan = ctypes.c_uint32(0)
    FP, U32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    abi.check(abi.load().rt_refit_plan(whole.ctypes.data_as(FP), whole.shape[0], lookup.shape[0], roots.ctypes.data_as(U32), roots.shape[0],
                                       plan.ctypes.data_as(U32), plan.shape[0], ctypes.byref(n_plan)))
    runs = {int(node): (int(first), int(n)) for node, first, n in plan[:n_plan.value] if node in set(roots.tolist())}
    first, n = max(runs.values(), key=lambda fn: fn[1])
    members = np.sort(lookup[first:first + n].astype(np.int64))
    assert members[-1] - members[0] + 1 == n, "the mesh's triangles are not one run of records"
    return int(members[0]), int(n)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(scene, mat, first=None, count=None):
    import torch
    r = rt.RendererRaytracing(W, H, scene, maxBounces=2).initialize(None, mat)
    lib, ctx = r._lib, r._ctx
    r.render()
    if first is None:
        first, count = largest_mesh(scene)
    rec0 = np.ascontiguousarray(scene.pack_triangles(), F)[first:first + count].copy()
    corners = np.stack([rec0[:, c] for c in COLS], axis=1)                                  # (count, 3, 3)
    dev = "cuda:%d" % r.device
    poses = []
    for sign in (1.0, -1.0):                         # the corners displaced by a sine field of either sign
        p = corners + F(sign * 0.05) * np.sin(F(4.0) * corners[..., [1, 2, 0]]).astype(F)
        poses.append(torch.from_numpy(np.ascontiguousarray(p, F)).to(dev))
    torch.cuda.synchronize()

    def route_a(t):
        v = t.cpu().numpy()
        rec = rec0.copy()
        for k, c in enumerate(COLS):
            rec[:, c] = v[:, k]
        r.update_triangles(first, rec)
        r.refit()

    def route_b(t):
        r.deform(first, t)

    def route_c(t):
        abi.check(lib.rt_deform_triangles(ctx, first, count, ctypes.c_void_p(t.data_ptr()), 3 * count, None, None, 0, None), ctx)
        abi.check(lib.rt_refit_blas(ctx, None, 0), ctx)

    routes = {"a_cpu_repack_update_refit": route_a, "b_deform": route_b, "b_c_abi_only": route_c}
    ms = {k: [] for k in routes}
    state = {}
    for i in range(WARMUP + REPS):
        for name, fn in routes.items():
            took = timed(lambda: fn(poses[i % 2]))
            if i >= WARMUP:
                ms[name].append(took)
            state[name] = (r.read_triangles(first, count).view(np.uint32).copy(), r.read_nodes().view(np.uint32).copy())
    for name in routes:                              # every route ends in the same pose: the same records and the same nodes
        assert np.array_equal(state[name][0], state["a_cpu_repack_update_refit"][0]), name
        assert np.array_equal(state[name][1], state["a_cpu_repack_update_refit"][1]), name
    res = {"triangles": int(scene.triangleCount), "moved": int(count), "blas_nodes": int(scene.blasNodesUsed),
           "bytes_a_records": int(count) * 160, "bytes_b_vertices": int(count) * 36}
    for name, v in ms.items():
        res[name + "_ms"] = [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", help="a packed scene saved by --save-big, instead of building the 114,688-triangle mesh")
    ap.add_argument("--save-big", help="build the 114,688-triangle scene, save it packed (np.savez) and exit: needs no device")
    args = ap.parse_args()
    if args.save_big:
        np.savez(args.save_big, **big_scene().to_packed())
        return
    from compute_raytracer_amd.procedural import triangle_scene
    out = {"build_id": abi.load().rt_build_id().decode(), "warmup": WARMUP, "reps": REPS, "ms": "median, min, max"}
    scene, mat = triangle_scene(seed=40, n_models=3)
    m = scene.meshes[1]
    out["test_mesh_176"] = measure(scene, mat, m.lookup_offset, m.soup.count)
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    out["ref"] = measure(rt.SceneRaytracing.from_packed(d), rt.Material.white())
    big = rt.SceneRaytracing.from_packed(np.load(args.big)) if args.big else big_scene()
    out["big_114688"] = measure(big, rt.Material.white())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
