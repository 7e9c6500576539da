"""Dev tool: what one deformation step of a triangle mesh costs by each route ("Deforming meshes").

    python tools/refit_rate.py

Workloads: the reference's scene (tests/golden/ref_scene.npz, 12,604 triangles) and bench.py --config TRI's scene (12,846 triangles),
both at 1344 x 846.  A step moves every vertex of the scene's largest mesh (two poses, alternating) and renders one awaited frame.
  device:  rt_update_triangles of the mesh's records, rt_refit_blas of every root, rt_render + rt_wait.
  host:    the only route without these calls -- the boxes refitted in numpy on the host (over the runs rt_refit_plan lists, made
           once outside the timed region: a loop over the nodes with one numpy reduction each), rt_write_triangles of every record,
           rt_write_nodes of every BLAS node, then the frame, which rebuilds and uploads the pair records.
Both legs run in one process on one build; the host's clock around the calls (they are synchronous): WARMUP steps, then REPS,
the median, with the host leg's parts listed separately.  One JSON line."""
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

WARMUP, REPS = 2, 9
W, H = 1344, 846
F = np.float32
FP = ctypes.POINTER(ctypes.c_float)
U32 = ctypes.POINTER(ctypes.c_uint32)
COLS = (slice(0, 3), slice(12, 15), slice(24, 27))


def u32f(f):
    f = float(f)
    return 0 if not f > 0.0 else (4294967295 if f >= 4294967040.0 else int(f))


def poses(tris, first, count):
    """two poses of triangles [first, first + count): the corners displaced by a sine field of either sign"""
    out = []
    for sign in (1.0, -1.0):
        t = tris.copy()
        for c in COLS:
            v = t[first:first + count, c]
            t[first:first + count, c] = v + F(sign * 0.05) * np.sin(F(4.0) * v[:, [1, 2, 0]]).astype(F)
        out.append(t)
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(scene, mat, bounces):
    r = rt.RendererRaytracing(W, H, scene, maxBounces=bounces).initialize(None, mat)
    lib, ctx = r._lib, r._ctx
    r.render()
    tris0 = np.ascontiguousarray(scene.pack_triangles(), F)
    lookup = np.asarray(scene.pack_tri_lookup(), F)
    blas = np.ascontiguousarray(scene.pack_blas_nodes(), F)
    base = scene.tlasNodesMax
    whole = np.zeros((base + blas.shape[0], 8), F)
    whole[base:] = blas
    roots = np.array(sorted(set(u32f(b[16]) for b in np.asarray(scene.pack_blas(), F).reshape(-1, 20))), np.uint32)
    plan = np.zeros((whole.shape[0], 3), np.uint32)
    n_plan = ctypes.c_uint32(0)
    abi.check(lib.rt_refit_plan(whole.ctypes.data_as(FP), whole.shape[0], lookup.shape[0], roots.ctypes.data_as(U32), roots.shape[0],
                                plan.ctypes.data_as(U32), plan.shape[0], ctypes.byref(n_plan)))
    plan = plan[:n_plan.value].astype(np.int64)
    slot_tri = np.array([u32f(v) for v in lookup], np.int64)
    # the largest mesh: the longest run of triangle indices under one root
    sizes = {int(node): (int(first), int(n)) for node, first, n in plan if node in set(roots.tolist())}
    root = max(sizes, key=lambda k: sizes[k][1])
    members = np.sort(slot_tri[sizes[root][0]:sizes[root][0] + sizes[root][1]])
    first, count = int(members[0]), int(members[-1] - members[0] + 1)
    two = poses(tris0, first, count)

    def frame():
        abi.check(lib.rt_render(ctx), ctx)
        abi.check(lib.rt_wait(ctx), ctx)

    def device_step(t):
        rec = np.ascontiguousarray(t[first:first + count])
        abi.check(lib.rt_update_triangles(ctx, first, count, rec.ctypes.data_as(FP)), ctx)
        abi.check(lib.rt_refit_blas(ctx, None, 0), ctx)
        frame()

    parts = {"numpy_refit": [], "write_triangles": [], "write_nodes": [], "frame": []}

    def host_step(t, keep):
        nodes = [None]

        def refit():
            c = np.stack([t[slot_tri][:, cc] for cc in COLS], axis=1).reshape(-1, 3)          # (3 slots, 3): slot s at rows 3s .. 3s+2
            out = blas.copy()
            for node, f0, n in plan:
                run = c[3 * f0:3 * (f0 + n)]
                out[node - base, 0:3] = run.min(axis=0)
                out[node - base, 4:7] = run.max(axis=0)
            nodes[0] = out
        a = timed(refit)
        b = timed(lambda: abi.check(lib.rt_write_triangles(ctx, t.ctypes.data_as(FP), t.shape[0]), ctx))
        c_ = timed(lambda: abi.check(lib.rt_write_nodes(ctx, 32 * base, nodes[0].ctypes.data_as(FP), nodes[0].shape[0]), ctx))
        d = timed(frame)
        if keep:
            for k, v in zip(parts, (a, b, c_, d)):
                parts[k].append(v)
        return nodes[0]

    res = {"triangles": int(tris0.shape[0]), "moved": count, "blas_nodes": int(blas.shape[0])}
    dev = []
    for i in range(WARMUP + REPS):
        ms = timed(lambda: device_step(two[i % 2]))
        if i >= WARMUP:
            dev.append(ms)
    st0 = r.stats()["pair_rebuilds"]
    dev_nodes = r.read_nodes(base, blas.shape[0])
    dev_img = r.read_pixels().copy()
    host = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        host_nodes = host_step(two[i % 2], i >= WARMUP)
        if i >= WARMUP:
            host.append((time.perf_counter() - t0) * 1e3)
    last = (WARMUP + REPS - 1) % 2
    # both routes end in the same pose: the same node bytes and the same picture
    assert np.array_equal(host_nodes.view(np.uint32), dev_nodes.view(np.uint32)) and np.array_equal(r.read_pixels(), dev_img), last
    res["device_step_ms"] = [round(float(np.median(dev)), 3), round(float(np.min(dev)), 3), round(float(np.max(dev)), 3)]
    res["host_step_ms"] = [round(float(np.median(host)), 3), round(float(np.min(host)), 3), round(float(np.max(host)), 3)]
    res["host_parts_ms"] = {k: round(float(np.median(v)), 3) for k, v in parts.items()}
    res["pair_rebuilds"] = {"device_leg": int(st0) - 1, "host_leg": int(r.stats()["pair_rebuilds"] - st0)}
    r.close()
    return res


def main():
    from compute_raytracer_amd.procedural import triangle_scene
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    out = {"build_id": abi.load().rt_build_id().decode(), "warmup": WARMUP, "reps": REPS, "frame": [W, H], "ms": "median, min, max"}
    out["ref"] = measure(rt.SceneRaytracing.from_packed(d), rt.Material.white(), int(d["maxBounces"]))
    scene, mat = triangle_scene(seed=21, n_models=2, rings=48, sectors=64)
    out["tri_12846"] = measure(scene, mat, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
