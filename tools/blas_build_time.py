"""Dev tool: what a fresh bottom-level tree of one mesh costs by each route.

    python tools/blas_build_time.py [--big-rings 78]

Workloads: a random soup of 1,000 triangles, and a tessellated sphere of 2 * rings^2 triangles (78: 12,168, the size of the
reference's largest mesh) -- each its own scene of one instance, laid out with node_capacity="full", written with a one-leaf tree.
  device:  RendererRaytracing.rebuild() -- rt_build_blas and the read-back of nodes and lookup into the scene object.
           Also timed: rt_build_blas alone.
  host:    the route without it -- acceleration/bvh.py: build_tree of the mesh's soup, then rt_write_nodes and rt_write_tri_lookup
           of the result.  Timed once (it takes seconds), its parts listed.
Both legs run in one process on one build, the host's clock around synchronous calls: WARMUP calls, then REPS, the median.  Both
routes must leave the same node bytes.  `levels` is the depth of the tree + 1: the number of times the build waits for one word
from the device.  One JSON line."""
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
from compute_raytracer_amd.acceleration.bvh import MeshTree, build_tree  # noqa: E402
from compute_raytracer_amd.procedural import obj_uv_sphere  # noqa: E402
from compute_raytracer_amd.scene_raytracing import TriMesh  # noqa: E402
from compute_raytracer_amd.soup import TriangleSoup, parse_obj  # noqa: E402

WARMUP, REPS = 2, 7
F = np.float32
FP = ctypes.POINTER(ctypes.c_float)


def f32_soup(soup):
    """the soup with its corners rounded to float32: what the device holds, and what rt_build_blas builds a tree of"""
    return TriangleSoup(soup.position.astype(F).astype(np.float64), soup.normal, soup.uv, soup.color)


def random_soup(T, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-4, 4, (T, 1, 3)) + rng.uniform(-0.6, 0.6, (T, 3, 3))
    n = np.zeros((T, 3, 3))
    n[..., 1] = 1.0
    return f32_soup(TriangleSoup(p, n, np.zeros((T, 3, 2)), [0.8, 0.7, 0.6, 1.0]))


def one_leaf(soup):
    c = soup.position.reshape(-1, 3)
    t = MeshTree()
    t.lo, t.hi = c.min(axis=0)[None, :].copy(), c.max(axis=0)[None, :].copy()
    t.first, t.count = np.zeros(1, np.int64), np.array([soup.count], np.int64)
    t.order, t.used = np.arange(soup.count, dtype=np.int64), 1
    t.box_lo, t.box_hi = np.array([999999.0] * 3), np.array([-999999.0] * 3)
    return t


def depth(nodes, root):
    best, todo = 0, [(root, 1)]
    while todo:
        i, d = todo.pop()
        best = max(best, d)
        if nodes[i, 7] == 0:
            todo += [(int(nodes[i, 3]), d + 1), (int(nodes[i, 3]) + 1, d + 1)]
    return best


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(soup):
    models = [dict(meshIndex=0, position=[0.0, 0.5, -6.0], eulers=[0, 0, 0])]
    scene = rt.SceneRaytracing().createScene([]).createTriangleScene([TriMesh(soup, one_leaf(soup))], models, node_capacity="full")
    r = rt.RendererRaytracing(256, 192, scene, maxBounces=2).initialize(None, rt.Material.white())
    lib, ctx = r._lib, r._ctx
    r.render()
    mesh = scene.meshes[0]
    rng_ = np.zeros(1, dtype=abi.BLAS_RANGE_DTYPE)
    rng_[0] = (mesh.root_node, scene.node_buffer_length() - mesh.root_node, 0, soup.count)
    used = np.zeros(1, np.uint32)

    def call_only():
        abi.check(lib.rt_build_blas(ctx, rng_.ctypes.data_as(ctypes.POINTER(abi.RtBlasRange)), 1, used.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), ctx)
    whole, alone = [], []
    for i in range(WARMUP + REPS):
        a = timed(r.rebuild)[0]
        b = timed(call_only)[0]
        if i >= WARMUP:
            whole.append(a)
            alone.append(b)
    dev_nodes = r.read_nodes()
    r.render()
    dev_img = r.read_pixels().copy()
    # the host route, once
    t_build, tree = timed(lambda: build_tree(soup))
    nodes = np.ascontiguousarray(tree.nodes(mesh.root_node, 0), F)
    lookup = np.ascontiguousarray(tree.order.astype(F))
    t_up = timed(lambda: (abi.check(lib.rt_write_nodes(ctx, 32 * mesh.root_node, nodes.ctypes.data_as(FP), nodes.shape[0]), ctx),
                          abi.check(lib.rt_write_tri_lookup(ctx, lookup.ctypes.data_as(FP), lookup.shape[0]), ctx)))[0]
    host_nodes = r.read_nodes()
    assert np.array_equal(host_nodes.view(np.uint32), dev_nodes.view(np.uint32)), "the two routes left different nodes"
    r.render()
    assert np.array_equal(r.read_pixels(), dev_img)
    res = {"triangles": int(soup.count), "nodes": int(tree.used), "levels": depth(dev_nodes, mesh.root_node),
           "rebuild_ms": [round(float(np.median(whole)), 3), round(float(np.min(whole)), 3), round(float(np.max(whole)), 3)],
           "rt_build_blas_ms": [round(float(np.median(alone)), 3), round(float(np.min(alone)), 3), round(float(np.max(alone)), 3)],
           "host_ms": round(t_build + t_up, 1), "host_parts_ms": {"build_tree": round(t_build, 1), "upload": round(t_up, 3)}}
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-rings", type=int, default=78)
    a = ap.parse_args()
    out = {"build_id": abi.load().rt_build_id().decode(), "warmup": WARMUP, "reps": REPS, "ms": "median, min, max"}
    out["soup_1000"] = measure(random_soup(1000, 1100))
    big = parse_obj(obj_uv_sphere(a.big_rings, a.big_rings, 1.0, quads=False), dict(color=[0.3, 0.7, 0.9, 1.0], alignBottom=True, scale=1.0))
    out["sphere_%d" % big.count] = measure(f32_soup(big))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
