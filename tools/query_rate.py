"""Dev tool: the rate of ray queries -- nearest (rt_trace_rays), limited nearest (rt_trace_rays_ex with RT_QUERY_LIMITS),
occlusion (rt_occluded) and shaded (rt_shade_rays) -- beside the per-ray cost of an awaited frame of the reference's scene.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o q -- python tools/query_rate.py

Workloads: the 1344x846 primary rays of the reference's scene (tests/golden/ref_scene.npz), 2^20 random rays on it (origins in
the scene box, within 20 of the camera, grown by half, directions of random length), 2^20 random rays on C3 (1024 spheres).  Each
runs REPS times through the device path on one stream, once per kind: "nearest" (flags 0), "limited" (words 3 and 7 = 0.001 and
9999, the same answers through the limited kernels) and "occluded" (the same limits); the kernel statistics of rocprofv3
(query_triangles / query_spheres, limited_triangles / limited_spheres / occlude_spheres) give the rays per ms of the query
kernels, and the line printed here gives the same from hipEvents around the batch.  The frame's
figure is rt_stats.rays / kernel_ms of an awaited frame (RK:114 + RK:153 traversals, reflections and shadow rays included).
"shade" is rt_shade_rays on the same rays (whole paths: rays_per_ms counts caller rays, not traversals; hit_fraction: dist > 0).
"multi1" / "multi4" / "multi8" is rt_trace_rays_multi with k = 1, 4, 8 under the same limits (hit_fraction: hit 0 exists).
"shade_vs_frame": the 2^20 primary rays of a 1024 x 1024 frame shaded with RT_SHADE_COMPOSE, beside kernel_ms of that frame
through rt_render -- the same pixels by both routes -- on the reference's scene and on C3's spheres (the query searches the
spheres by brute force, the frame walks the hierarchy).
"samples_ref_s2" ... "samples_c3_s4": rt_render_samples (both outputs) of a 1024 x 1024 frame at s = 2 and 4, beside (a) rt_shade_rays
with RT_SHADE_COMPOSE over the same s*s 2^20 rays resident on the device and (b) kernel_ms of an rt_render frame of
(1024 s) x (1024 s) -- the same samples by the three routes.  `python tools/query_rate.py samples` runs these alone.
`python tools/query_rate.py ref` runs "ref_primary" and "ref_random_2^20" alone, for nearest, limited, occluded, shade and multi4:
the A/B of two builds (RT355_LIB), a run each in turn.  `python tools/query_rate.py ref hide` does so with an instance mask table
that hides every instance of the reference scene's largest mesh (rt_write_instance_masks): what a skipped instance saves."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compute_raytracer_amd as rt  # noqa: E402

REPS = 20


def ray_tensor(torch, o, d):
    rays = np.zeros((o.shape[0], 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = 0.001, 9999.0            # the reference's limits: every kind answers the same rays the same way
    return torch.from_numpy(rays).to("cuda:0")


def camera(scene, W, H, bounces=4):
    p = scene.pack_params(bounces)
    F = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    hc = (xs.reshape(-1).astype(F) - F(W) / F(2)) / F(W) * F(2)
    vc = (F(H) / F(2) - ys.reshape(-1).astype(F)) / F(W) * F(2)
    d = np.stack([(p[4 + k] + hc * p[8 + k]) + vc * p[12 + k] for k in range(3)], axis=1)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    return np.broadcast_to(p[0:3], d.shape).astype(F), d.astype(F)


def random_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    ext = hi - lo
    o = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.05, 20.0, (n, 1))
    return o, d.astype(np.float32)


def timed_one(torch, r, rays, kind):
    if kind == "occluded":
        out = torch.empty((rays.shape[0],), dtype=torch.uint8, device=rays.device)
        run = lambda: r.occluded(rays, out=out)
    elif kind == "shade":
        out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
        run = lambda: r.shade_rays(rays, out=out)
    elif kind.startswith("multi"):
        k = int(kind[5:])
        out = torch.empty((rays.shape[0], k, 8), dtype=torch.float32, device=rays.device)
        run = lambda: r.trace_rays_multi(rays, k=k, limits=True, out=out)
    else:
        out = torch.empty_like(rays)
        run = lambda: r.trace_rays(rays, out=out, limits=kind == "limited")
    run()                                         # warm-up (first-use work: corner array, code objects)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / REPS
    if kind == "occluded":
        hits = int((out > 0).sum().item())
    elif kind == "shade":
        hits = int((out[:, 3] > 0).sum().item())
    elif kind.startswith("multi"):
        hits = int((out[:, 0, 3].view(torch.int32) >= 0).sum().item())
    else:
        hits = int((out[:, 3].view(torch.int32) >= 0).sum().item())
    return {"ms": round(ms, 4), "rays_per_ms": round(rays.shape[0] / ms), "hit_fraction": round(hits / rays.shape[0], 3)}


KINDS = ("nearest", "limited", "occluded", "shade", "multi1", "multi4", "multi8")


def timed(torch, r, rays, kinds=KINDS):
    res = {"rays": int(rays.shape[0])}
    for kind in kinds:
        res[kind] = timed_one(torch, r, rays, kind)
    return res


def shade_vs_frame(torch, scene, bounces, mat):
    """kernel_ms of an awaited 1024 x 1024 frame and the time of rt_shade_rays (RT_SHADE_COMPOSE) over its 2^20 primary rays"""
    W = H = 1024
    r = rt.RendererRaytracing(W, H, scene, maxBounces=bounces).initialize(None, mat)
    for _ in range(5):
        r.render()
    st = r.stats()
    rays = ray_tensor(torch, *camera(scene, W, H, bounces))
    out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
    r.shade_rays(rays, compose=True, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        r.shade_rays(rays, compose=True, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / REPS
    r.close()
    return {"rays": int(rays.shape[0]), "frame_kernel_ms": round(st["kernel_ms"], 4), "frame_kernel": st["kernel_id"],
            "shade_ms": round(ms, 4), "shade_rays_per_s": round(rays.shape[0] / ms * 1e3)}


def samples_vs_routes(torch, scene, bounces, mat, s):
    """rt_render_samples of a 1024 x 1024 frame at factor s; rt_shade_rays over its s*s 2^20 sample rays; kernel_ms of the frame of
    the larger target"""
    W = H = 1024
    r = rt.RendererRaytracing(s * W, s * H, scene, maxBounces=bounces).initialize(None, mat)
    for _ in range(5):
        r.render()
    st = r.stats()
    r.close()
    r = rt.RendererRaytracing(W, H, scene, maxBounces=bounces).initialize(None, mat)
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    flt = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

    def timed_ms(run):
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    samples_ms = timed_ms(lambda: r.render_samples(s, out=(img, flt)))
    rays = ray_tensor(torch, *camera(scene, s * W, s * H, bounces))
    out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
    shade_ms = timed_ms(lambda: r.shade_rays(rays, compose=True, out=out))
    r.close()
    return {"s": s, "samples": int(rays.shape[0]), "render_samples_ms": round(samples_ms, 4), "shade_rays_ms": round(shade_ms, 4),
            "frame_kernel_ms": round(st["kernel_ms"], 4), "frame_kernel": st["kernel_id"],
            "samples_per_s": round(rays.shape[0] / samples_ms * 1e3)}


def samples(torch, out):
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    scene = rt.SceneRaytracing.from_packed(d)
    cfg = rt.BASELINE_CONFIGS["C3"]
    c3 = rt.synthetic_scene(cfg["spheres"], cfg["seed"])
    out["build_id"] = rt.abi.load().rt_build_id().decode()
    for s in (2, 4):
        out["samples_ref_s%d" % s] = samples_vs_routes(torch, scene, int(d["maxBounces"]), rt.Material.white(), s)
        out["samples_c3_s%d" % s] = samples_vs_routes(torch, c3, cfg["bounces"], None, s)


def largest_mesh(scene):
    """The mesh with the most lookup slots under its BLAS root, and that count"""
    nodes = np.asarray(scene.pack_blas_nodes(), np.float32).reshape(-1, 8)

    def slots(root):
        total, todo = 0, [int(root) - scene.tlasNodesMax]
        while todo:
            i = todo.pop()
            left, count = int(nodes[i, 3]) - scene.tlasNodesMax, int(nodes[i, 7])
            if count:
                total += count
            else:
                todo += [left, left + 1]
        return total

    sizes = [slots(m.root_node) for m in scene.meshes]
    return int(np.argmax(sizes)), max(sizes)


def main():
    import torch
    if sys.argv[1:] == ["samples"]:
        out = {}
        samples(torch, out)
        print(json.dumps(out))
        return
    ref_only = sys.argv[1:2] == ["ref"]
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene.npz"))
    scene = rt.SceneRaytracing.from_packed(d)
    W, H = int(d["W"]), int(d["H"])
    r = rt.RendererRaytracing(W, H, scene, maxBounces=int(d["maxBounces"])).initialize(None, rt.Material.white())
    out = {}
    for _ in range(5):
        r.render()
    st = r.stats()
    out["ref_frame"] = {"rays": st["rays"], "kernel_ms": round(st["kernel_ms"], 4), "rays_per_ms": round(st["rays"] / st["kernel_ms"])}
    kinds = ("nearest", "limited", "occluded", "shade", "multi4") if ref_only else KINDS
    if sys.argv[1:] == ["ref", "hide"]:
        mesh, n_slots = largest_mesh(scene)
        hidden = np.asarray(scene.instances.mesh_index) == mesh
        r.set_instance_masks(np.where(hidden, 0, 0xFFFFFFFF))
        out["hidden"] = {"mesh": mesh, "slots": n_slots, "instances": [int(i) for i in np.nonzero(hidden)[0]]}
    out["ref_primary"] = timed(torch, r, ray_tensor(torch, *camera(scene, W, H)), kinds)
    root = np.asarray(scene.pack_tlas_nodes(), np.float64).reshape(-1, 8)[0]
    cam = scene.pack_params(4)[0:3].astype(np.float64)                  # (the floor's box spans millions: within 20 of the camera)
    lo, hi = np.maximum(root[0:3], cam - 20.0), np.minimum(root[4:7], cam + 20.0)
    out["ref_random_2^20"] = timed(torch, r, ray_tensor(torch, *random_rays(lo, hi, 1 << 20, 1)), kinds)
    r.close()
    if ref_only:
        out["build_id"] = rt.abi.load().rt_build_id().decode()
        print(json.dumps(out))
        return
    cfg = rt.BASELINE_CONFIGS["C3"]
    c3 = rt.synthetic_scene(cfg["spheres"], cfg["seed"])
    r = rt.RendererRaytracing(256, 256, c3, maxBounces=cfg["bounces"]).initialize()
    r.recalculateScene()
    sp = np.asarray(c3.pack_spheres(), np.float32).reshape(-1, 8)
    lo, hi = (sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)
    out["c3_random_2^20"] = timed(torch, r, ray_tensor(torch, *random_rays(lo.astype(np.float64), hi.astype(np.float64), 1 << 20, 2)))
    r.close()
    out["shade_vs_frame_ref"] = shade_vs_frame(torch, scene, int(d["maxBounces"]), rt.Material.white())
    out["shade_vs_frame_c3"] = shade_vs_frame(torch, c3, cfg["bounces"], None)
    samples(torch, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
