"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

import compute_raytracer_amd as rt
from compute_raytracer_amd.scene_raytracing import CONSTANT_SKY_RGBA, synthetic_spheres


def config_inputs(name, width=None, height=None, spheres=None, bounces=None):
    cfg = dict(rt.BASELINE_CONFIGS[name])
    if width: cfg["width"] = width
    if height: cfg["height"] = height
    if spheres: cfg["spheres"] = spheres
    if bounces is not None: cfg["bounces"] = bounces
    scene = rt.synthetic_scene(cfg["spheres"], cfg["seed"])
    return cfg, scene


def gpu_render(scene, width, height, bounces, strict, skybox=None, variant=0, rank=0, world=1):
    r = rt.RendererRaytracing(width, height, scene, maxBounces=bounces, rank=rank, world=world)
    r.initialize(skybox)
    r.set_mode(strict)
    r.set_variant(variant)
    r.render()
    img = r.read_pixels()
    st = r.stats()
    r.close()
    return img, st


def oracle_render(oracle, scene, width, height, bounces, skybox=None, want_float=False, **kw):
    sky = skybox if skybox is not None else rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)
    return oracle.render(scene.pack_params(bounces), scene.pack_spheres(), sky.faces, width, height,
                         want_float=want_float, **kw)


def diff_stats(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))[..., :3].max(axis=-1)
    n = d.size
    return {
        "pixels": n,
        "exact": float((d == 0).sum()) / n,
        "within1": float((d <= 1).sum()) / n,
        "within2": float((d <= 2).sum()) / n,
        "max": int(d.max()),
        "n_gt1": int((d > 1).sum()),
    }


# ---- procedural triangle scenes: compute_raytracer_amd/procedural.py (bench.py --config TRI uses them too) ----
from compute_raytracer_amd.procedural import obj_floor, obj_uv_sphere, tri_buffers, triangle_scene  # noqa: E402,F401


def gpu_render_tri(scene, material, width, height, bounces, skybox=None, heatmap=False, variant=0):
    """variant 0: the library's choice (pair records where the scene fits them), 6: the reference's node buffer only."""
    import compute_raytracer_amd as rt
    r = rt.RendererRaytracing(width, height, scene, maxBounces=bounces)
    r.initialize(skybox, material)
    r.set_variant(variant)
    if heatmap:
        r.showHeatmap()
    r.render()
    img = r.read_pixels()
    st = r.stats()
    r.close()
    return img, st


# ---- the reference's own scene, as committed fixtures (tests/golden/make_ref_scene.py) ----
def ref_fixture():
    """-> (scene, sky CubemapMaterial, W, H, maxBounces, canvas (H,W,3) uint8, pin dict).  Reads only tests/golden/."""
    import json
    import os
    from PIL import Image
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = np.load(os.path.join(g, "ref_scene.npz"))
    scene = rt.SceneRaytracing.from_packed(d)
    strip = np.array(Image.open(os.path.join(g, "ref_sky.png")).convert("RGBA"), dtype=np.uint8)
    sky = rt.CubemapMaterial()
    n = strip.shape[0]
    sky.faces = [np.ascontiguousarray(strip[:, k * n:(k + 1) * n]) for k in range(6)]
    canvas = np.array(Image.open(os.path.join(g, "ref_canvas.png")).convert("RGB"), dtype=np.uint8)
    pin = json.load(open(os.path.join(g, "ref_pin.json")))
    return scene, sky, int(d["W"]), int(d["H"]), int(d["maxBounces"]), canvas, pin


# ---- triangle scenes made by hand, and the top-level trees and stack forms of the triangle kernel (tests/test_triangles_gpu.py,
# tests/test_work_list_gpu.py) ----
def random_sky(seed, w=8, h=8):
    rng = np.random.default_rng(seed)
    m = rt.CubemapMaterial()
    m.faces = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(6)]
    return m


def spine_scene(depth):
    """A BLAS no builder would make: a spine of `depth` inner nodes, each with a leaf as its FARTHER child, so that the
    walk pushes one entry per level -- beyond the eight slots the persistent kernel keeps in LDS, and beyond the twenty the
    reference's stack has at all (RK:71; RK:303-306 pushes without a guard: the index clamps to the last slot, and the pops
    that follow read that slot again and again).  One triangle per leaf, each covering its own part of the view."""
    base = 1                                                    # tlasNodesMax of one instance
    nodes = np.zeros((1 + 2 * depth, 8), np.float32)            # S_0, then the pairs (A_k, S_{k+1}); the last "S" is a leaf
    tris = np.zeros((depth + 1, 40), np.float32)
    def box(i, lo, hi, left, count):
        nodes[i, 0:3] = lo; nodes[i, 3] = left; nodes[i, 4:7] = hi; nodes[i, 7] = count
    box(0, [-9, -9, -1.0], [9, 9, 5.0], base + 1, 0)
    for k in range(depth):
        a, s = 1 + 2 * k, 2 + 2 * k
        box(a, [-9, -9, -3.0], [9, 9, -2.0], k, 1)                                   # leaf A_k: lookup slot k
        if k + 1 < depth: box(s, [-9, -9, -1.0], [9, 9, 5.0], base + s + 1, 0)       # S_{k+1}
        else: box(s, [-9, -9, -1.0], [9, 9, 5.0], depth, 1)                          # the bottom: a leaf inside the near box
    for k in range(depth + 1):
        z = -2.05 - 0.9 * k / depth if k < depth else -0.5
        x0 = -8.0 + 16.0 * ((k * 7) % (depth + 1)) / (depth + 1)
        w = 3.0 if k < depth else 40.0
        # front face towards +z (RK:359 culls det < 1e-5)
        for c, (x, y) in enumerate([(x0, -8.0), (x0 + w, -8.0), (x0 + w / 2, 9.0)]):
            tris[k, 12 * c:12 * c + 3] = [x, y, z]
            tris[k, 12 * c + 4:12 * c + 7] = [0, 0, 1]
            tris[k, 12 * c + 8:12 * c + 10] = [c / 2.0, c % 2]
        tris[k, 36:40] = [0.2 + 0.8 * ((k * 5) % 7) / 7.0, 0.3 + 0.7 * ((k * 3) % 5) / 5.0, 0.9 - 0.6 * (k % 4) / 4.0, 1.0 if k % 3 else 0.5]
    d = dict(triangles=tris, blas_nodes=nodes, tri_lookup=np.arange(depth + 1, dtype=np.float32),
             mesh_root=np.array([base]), mesh_box_lo=np.array([[-9.0, -9.0, -3.0]]), mesh_box_hi=np.array([[9.0, 9.0, 5.0]]),
             inst_mesh=np.array([0]), inst_position=np.array([[0.0, 0.0, 0.0]]), inst_eulers=np.array([[0.0, 0.0, 0.0]]),
             inst_speed=np.array([[0.0, 0.0, 0.0]]), camera_position=np.array([0.0593, 2.692, 3.293]),
             camera_eulers=np.array([0.0, 106.0, 270.0], np.float32), light=np.array([0.0, 5.0, 6.0, 3.0, 0.3]))
    return rt.SceneRaytracing.from_packed(d)



def deepen_top_level(scene, levels):
    """The frame's top-level tree under `levels` extra inner nodes: each new node has the old tree (one level down) as its first
    child and a leaf far away from everything (instance 0 again: never entered) as its second.  Same picture, a deeper walk."""
    t = np.asarray(scene.frame["tlas_nodes"], np.float32).reshape(-1, 8)
    n_old, extra = t.shape[0], 2 * levels
    assert n_old + extra <= scene.tlasNodesMax
    out = np.zeros((n_old + extra, 8), np.float32)
    for k in range(levels):                                  # node 0 and the chain nodes at 1, 3, 5, ...: children at (2k+1, 2k+2)
        i = 0 if k == 0 else 2 * k - 1
        out[i] = [-1e4, -1e4, -1e4, 2 * k + 1, 1e4, 1e4, 1e4, 0]
        out[2 * k + 2] = [9e3, 9e3, 9e3, 0, 9.1e3, 9.1e3, 9.1e3, 1]      # the far leaf
    base = 2 * levels - 1                                    # where the old root goes; the rest of the old tree behind the chain
    remap = lambda i: base if i == 0 else extra + i
    for i in range(n_old):
        row = t[i].copy()
        if row[7] == 0:
            row[3] = remap(int(row[3]))                      # old children sit side by side at left, left + 1 (left >= 1)
        out[remap(i)] = row
    scene.frame["tlas_nodes"] = out


def expected_form(scene, mat):
    """rt_tlas_fit.h restated: the stack form the library must pick for the frame's top-level tree (tiny 2, small 1, neither 0)."""
    nodes = tri_buffers(scene, mat)["nodes"]
    n = len(nodes)
    def u32f(f):
        f = float(f)
        return 0 if not f > 0.0 else (4294967295 if f >= 4294967040.0 else int(f))
    def fits(max_depth, max_nodes):
        todo = [(0, 0)]
        while todo:
            i, d = todo.pop()
            i = min(i, n - 1)
            if i >= max_nodes: return False
            if u32f(nodes[i, 7]) != 0: continue
            if d >= max_depth: return False
            left = u32f(nodes[i, 3])
            todo += [(left, d + 1), ((left + 1) & 0xFFFFFFFF, d + 1)]
        return True
    if len(scene.instances) > 16: return 0
    if len(scene.instances) > 12: return 4 if fits(8, 32) else 0       # 13-16 instances: the form that stages sixteen records
    if len(scene.instances) <= 4 and fits(3, 8): return 2
    if fits(4, 16): return 1
    if fits(8, 24): return 3
    return 4 if fits(8, 32) else 0


def leafy_scene(per_leaf, wild=False):
    """spine_scene's tree of depth 9 with `per_leaf` triangles in every leaf, side by side; wild: one leaf's first slot lies far
    beyond the lookup table (the oracle clamps it to the last slot; 14 bits would wrap it)."""
    depth = 9                                                    # spine_scene's tree with `per_leaf` triangles in every leaf, side by side
    nodes = np.zeros((1 + 2 * depth, 8), np.float32)
    tris = np.zeros(((depth + 1) * per_leaf, 40), np.float32)
    def box(i, lo, hi, left, count):
        nodes[i, 0:3] = lo; nodes[i, 3] = left; nodes[i, 4:7] = hi; nodes[i, 7] = count
    box(0, [-9, -9, -1.0], [9, 9, 5.0], 2, 0)
    for k in range(depth):
        a, sidx = 1 + 2 * k, 2 + 2 * k
        box(a, [-9, -9, -3.0], [9, 9, -2.0], k * per_leaf, per_leaf)
        if k + 1 < depth: box(sidx, [-9, -9, -1.0], [9, 9, 5.0], 1 + sidx + 1, 0)
        else: box(sidx, [-9, -9, -1.0], [9, 9, 5.0], depth * per_leaf, per_leaf)
    for k in range(depth + 1):
        for j in range(per_leaf):
            z = (-2.05 - 0.9 * k / depth if k < depth else -0.5) - 0.01 * j
            x0 = -8.0 + 16.0 * ((k * 7) % (depth + 1)) / (depth + 1) + 0.7 * j
            w = 2.0 if k < depth else 30.0
            t = k * per_leaf + j
            for c, (x, y) in enumerate([(x0, -8.0), (x0 + w, -8.0), (x0 + w / 2, 9.0)]):
                tris[t, 12 * c:12 * c + 3] = [x, y, z]
                tris[t, 12 * c + 4:12 * c + 7] = [0, 0, 1]
                tris[t, 12 * c + 8:12 * c + 10] = [c / 2.0, c % 2]
            tris[t, 36:40] = [0.2 + 0.8 * ((t * 5) % 7) / 7.0, 0.3 + 0.7 * ((t * 3) % 5) / 5.0, 0.9 - 0.6 * (t % 4) / 4.0, 1.0 if t % 3 else 0.5]
    if wild:
        nodes[5, 3] = 30000.0
    dd = dict(triangles=tris, blas_nodes=nodes, tri_lookup=np.arange(tris.shape[0], dtype=np.float32),
              mesh_root=np.array([1]), mesh_box_lo=np.array([[-9.0, -9.0, -3.0]]), mesh_box_hi=np.array([[9.0, 9.0, 5.0]]),
              inst_mesh=np.array([0]), inst_position=np.array([[0.0, 0.0, 0.0]]), inst_eulers=np.array([[0.0, 0.0, 0.0]]),
              inst_speed=np.array([[0.0, 0.0, 0.0]]), camera_position=np.array([0.0593, 2.692, 3.293]),
              camera_eulers=np.array([0.0, 106.0, 270.0], np.float32), light=np.array([0.0, 5.0, 6.0, 3.0, 0.3]))
    return rt.SceneRaytracing.from_packed(dd)


# ---- the work-list rule (rt_triangles.hip: order_hist), restated: quarter-octave classes, half / twice the throughput time, the caps ----
def cost_class(c):
    c = int(c)
    if c < 4:
        return c
    e = c.bit_length() - 1
    return 4 * e + ((c >> (e - 2)) & 3) - 4


def model(cost, wave_slots, mult4=1, mult16=4, cap16=64):
    n = len(cost)
    cls = np.array([cost_class(c) for c in cost])
    total = int(np.asarray(cost, np.uint64).sum())
    thr = total // (2 * max(wave_slots, 1))
    cls_of = lambda v: cost_class(min(v, 0xFFFFFFFF))
    above = lambda k: int((cls > k).sum())
    split, split16 = above(cls_of(mult4 * thr)), above(cls_of(mult16 * thr))
    if above(cls_of(4 * thr)) == 0:
        split = split16 = 0
    most, most16 = min(n // 16, 1024), min(n // 64, cap16)
    split16 = min(split16, most16)
    split = max(min(split, most), split16)
    return split - split16, split16, cls


# ---- awaited triangle frames with a work list (tests/test_work_list_gpu.py, tests/test_work_list_scenes_cpu.py) ----
# From 4,096 tiles on (rt_ctx.h: kOrderMinTiles) an awaited frame renders from the work list the previous frame on its stream left.
# 517 x 509: 65 x 64 = 4,160 tiles, the last column and the last row ragged.
WL_W, WL_H = 517, 509
WL_BOUNCES = 3
WL_SEED = 21

# Scenes that reach each instantiation of the kernel an awaited frame can take (rt_triangles.hip: rt_launch_triangles):
# name -> (n_models, extra top-level levels, how the buffers are changed, variant, the small forms are possible).
#   form1 / form3: trace_roles<SMALL 1 / 3> where the list splits tiles, trace_triangles where it does not;
#   form4: 13-16 instances;  form0_pairs: a lookup table longer than the instance list keeps the twenty-slot form;
#   pairs_wide: leaves of four triangles (pair records without 16-bit packing);  packed: more than 16 instances, no pair records;
#   node_buffer: variant 6, the reference's node buffer;  unpacked: a triangle lookup table over 65,536 entries;
#   wide_stack: a node buffer of more than 65,536 nodes (the uint32_t stack).
WORK_LIST_CASES = {
    "form1": (3, 0, None, 0, True),
    "form3": (9, 5, None, 0, True),
    "form4": (14, 0, None, 0, True),
    "form0_pairs": (3, 0, "double_lookup", 0, True),
    "pairs_wide": (None, 0, "leafy4", 0, False),
    "packed": (20, 0, None, 0, True),
    "node_buffer": (3, 0, None, 6, False),
    "unpacked": (2, 0, "pad_tri_lookup", 0, False),
    "wide_stack": (2, 0, "pad_nodes", 0, False),
}
ROLES_CASES = ("form1", "form3")


class WorkListCase:
    """A scene of WORK_LIST_CASES and its camera path: advance() turns the models and moves the camera (every frame differs
    from the one four frames earlier: a tile a list skipped cannot pass on an older frame's pixels), then applies the case's
    changes to the frame's buffers.  form(): the stack form the library must report for an awaited frame."""

    def __init__(self, name, seed=WL_SEED):
        n_models, self.deepen, self.change, self.variant, self.small = WORK_LIST_CASES[name]
        self.name = name
        if self.change == "leafy4":
            self.scene = leafy_scene(4)
            self.mat = rt.Material(np.random.default_rng(4).integers(0, 256, (8, 8, 4), dtype=np.uint8))
        else:
            rings, sectors = (7, 9) if self.change in ("pad_tri_lookup", "pad_nodes") else (6, 8)
            self.scene, self.mat = triangle_scene(seed=seed, n_models=n_models, rings=rings, sectors=sectors)
        if self.change == "pad_tri_lookup":
            self.scene.static["tri_lookup"] = np.concatenate([np.asarray(self.scene.static["tri_lookup"], np.float32),
                                                              np.zeros(70000, np.float32)])
        if self.change == "pad_nodes":              # unused nodes behind the trees: the buffer, not the walk, is over 65,536 nodes
            nodes = np.asarray(self.scene.static["blas_nodes"], np.float32)
            self.scene.static["blas_nodes"] = np.concatenate([nodes, np.zeros((70000, 8), np.float32)])
            self.scene.blasNodesUsed = self.scene.static["blas_nodes"].shape[0]

    def advance(self, dt=0.15, forwards=0.03, right=0.02):
        s = self.scene
        s.update(dt)
        s.camera.move(forwards, right)
        levels = min(self.deepen, (s.tlasNodesMax - len(s.frame["tlas_nodes"])) // 2)
        if levels:
            deepen_top_level(s, levels)
        if self.change == "double_lookup":          # every top-level leaf names its instances through a copy of the table
            look = np.asarray(s.frame["blas_lookup"], np.float32)
            s.frame["blas_lookup"] = np.concatenate([look, look])
            t = np.asarray(s.frame["tlas_nodes"], np.float32).copy()
            t[t[:, 7] > 0, 3] += len(look)
            s.frame["tlas_nodes"] = t

    def form(self):
        want = expected_form(self.scene, self.mat) if self.small and self.change != "double_lookup" else 0
        return 1 if want == 2 else want


RAGGED_STEP = (0.1, 0.01, 0.005)                  # advance()'s turn and camera step on the path of ragged_edge_case


def ragged_edge_case():
    """form1's scene with the camera turned left and up: the meshes sit in the ragged last column and the ragged last row."""
    case = WorkListCase("form1")
    case.scene.camera.spin(-30.0, -25.0)
    return case


def tile_work(oracle, scene, mat, sky, W, H, bounces, tile_step=1, tile_first=0):
    """A stand-in for the tiles' times: the oracle's per-pixel work (traversals, BLAS inner nodes, triangle tests) summed per 8 x 8
    tile, the tiles of one rank of a row partition in their local order."""
    w = oracle.tri_work_px(scene.pack_params(bounces), tri_buffers(scene, mat), sky.faces, W, H).astype(np.int64)
    px = 16 * w[..., 0] + w[..., 1] + w[..., 2]
    gx, gy = (W + 7) // 8, (H + 7) // 8
    pad = np.zeros((gy * 8, gx * 8), np.int64)
    pad[:H, :W] = px
    tiles = pad.reshape(gy, 8, gx, 8).sum(axis=(1, 3))
    return tiles[tile_first::tile_step].ravel()


# ---- the sphere dispatcher restated: which kernel form renders a sphere frame (tests/test_sphere_forms_gpu.py) ----
KID_LITERAL, KID_BRUTE_SINGLE, KID_BRUTE_PIPELINE = 1, 2, 3              # include/rt355.h: rt_kernel_id
KID_HIERARCHY_8, KID_HIERARCHY_12, KID_HIERARCHY_16, KID_HIERARCHY_GLOBAL = 4, 5, 6, 7
LDS_CAP = 160 * 1024                                                      # rt_kernels.hip: kLdsCap


def filter_plan(scene, bounces):
    """(filter_ok, signed_filter) of the library's own rt_plan (rt_api.hip), through the rt_filter_plan export."""
    import ctypes
    from compute_raytracer_amd import abi
    fp = ctypes.POINTER(ctypes.c_float)
    rec = np.ascontiguousarray(scene.pack_spheres(), np.float32).reshape(-1, 8)
    p = np.ascontiguousarray(scene.pack_params(bounces), np.float32)
    ok, sgn = ctypes.c_int(-1), ctypes.c_int(-1)
    abi.check(abi.load().rt_filter_plan(rec.ctypes.data_as(fp), rec.shape[0], p.ctypes.data_as(fp), ctypes.byref(ok), ctypes.byref(sgn)))
    return bool(ok.value), int(sgn.value)


def hierarchy_nodes(scene):
    """Inner + leaf node count of the sphere hierarchy the library builds (rt_build_hierarchy: rt_bvh_build, arity 4)."""
    import ctypes
    from compute_raytracer_amd import abi
    rec = np.ascontiguousarray(scene.pack_spheres(), np.float32).reshape(-1, 8)
    n = rec.shape[0]
    cap = 2 * n + 64
    out, link, nodes = np.zeros((cap, 4), np.float32), np.zeros(cap, np.uint32), ctypes.c_uint32(0)
    abi.check(abi.load().rt_build_hierarchy(rec.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                            link.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap, ctypes.byref(nodes)))
    return nodes.value


def sky_is_flat(sky):
    """rt_api.hip rt_enqueue: six 1x1 faces whose first texel has one RGB (face_texel0 leaves alpha out)."""
    faces = [np.asarray(f) for f in sky.faces]
    return all(f.shape[:2] == (1, 1) for f in faces) and all(np.array_equal(f[0, 0, :3], faces[0][0, 0, :3]) for f in faces)


def bvh_room(n_nodes, waves, entries):
    """rt_bvh.hip: bvh_lds_l0, bvh_gap_waves, bvh_lds_lists, bvh_list_bytes and launch_bvh's room(), for LDS at address 0."""
    need = (4 * (n_nodes + 1) + 2) // 3
    l0 = max(1024, need)
    l0 = (l0 + 15) & ~15
    gap = min((l0 - 1024) // 512, waves)
    lists = 4 * l0 + 16 * ((n_nodes + 4) & ~3)
    return lists + waves * 128 * (entries + 1) + (waves - gap) * 512


def lds_fits(k, nbytes):
    """rt_bvh.hip lds_fits: k workgroups of `nbytes` each in one CU's 128 granules of 1280 bytes."""
    return k * ((nbytes + 1279) // 1280) <= 128


class SphereForm:
    """What expected_sphere_form predicts: the rt_kernel_id, the form behind it and its hidden template arguments."""
    def __init__(self, kernel_id, form, sgn=None, flat=None, cap=None, resolve=False):
        self.kernel_id, self.form, self.sgn, self.flat, self.cap, self.resolve = kernel_id, form, sgn, flat, cap, resolve

    def __repr__(self):
        return "SphereForm(%d, %s, sgn=%s, flat=%s, cap=%s, resolve=%s)" % (self.kernel_id, self.form, self.sgn, self.flat, self.cap, self.resolve)


def expected_sphere_form(scene, bounces, strict=False, variant=0, sky=None, in_flight=False, nodes=None):
    """The form rt_enqueue / rt_launch_trace / rt_launch_bvh must give a sphere frame.  in_flight: the library has seen the
    previous batch of frames in flight on its own streams (rt_wait: pipelined_hint).  nodes: the node count of the hierarchy
    on the device (rt_read_hierarchy), which after a refit or a handoff need not be that of a fresh build of the scene;
    None: a fresh build's.  None: the frame is refused."""
    sky = sky if sky is not None else rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)
    flat = sky_is_flat(sky)
    n = len(scene.spheres)
    n16 = (n + 15) & ~15
    filter_ok, sgn = filter_plan(scene, bounces)                          # rt_api.hip rt_plan
    fast = not strict
    # rt_api.hip rt_enqueue: bvh_from, use_bvh, queue_pipeline, cfg.mode / cfg.variant
    use_bvh = fast and filter_ok and n > 0 and (variant == 4 or (variant == 0 and n >= (72 if in_flight else 128)))
    queue = not use_bvh and fast and filter_ok and (variant in (2, 3) or (variant in (0, 4, 5) and n >= 320))
    if use_bvh:                                                            # rt_bvh.hip launch_bvh
        nodes = hierarchy_nodes(scene) if nodes is None else nodes
        resolve = not flat                                                 # rt_launch_sky_resolve behind a textured sky
        for kid, waves, cap, k in ((KID_HIERARCHY_8, 8, 12, 3), (KID_HIERARCHY_12, 12, 12, 2), (KID_HIERARCHY_12, 12, 6, 2)):
            if lds_fits(k, bvh_room(nodes, waves, cap)):
                return SphereForm(kid, "bvh%d" % waves, sgn, flat, cap, resolve)
        for cap in (12, 6):
            if bvh_room(nodes, 16, cap) <= LDS_CAP:
                return SphereForm(KID_HIERARCHY_16, "bvh16", sgn, flat, cap, resolve)
        return SphereForm(KID_HIERARCHY_GLOBAL, "bvh_global", sgn, flat, 8, resolve)
    if not filter_ok or strict:                                            # rt_kernels.hip launch_strict (literal: no SGN)
        if n * 48 <= 56 * 1024: return SphereForm(KID_LITERAL, "literal8", None, flat)
        if n * 48 <= LDS_CAP: return SphereForm(KID_LITERAL, "literal16_w", None, flat)
        if n * 32 <= LDS_CAP: return SphereForm(KID_LITERAL, "literal16", None, flat)
        return SphereForm(KID_LITERAL, "literal_global", None, flat)
    v = 0 if variant in (4, 5) else variant                                # rt_kernels.hip fast_form
    single = n16 * 60 + 8 * 16 * 256 <= LDS_CAP                           # lds_pixels<8, true, false, true, 16>
    pipe16 = n16 * 40 + 8 * 16 * 256 <= LDS_CAP                           # lds_paths<8, true, 16> = lds_first<8, true, 8>
    if 2 * n16 * 16 + 8 * 8 * 256 > LDS_CAP:
        return SphereForm(KID_BRUTE_SINGLE, "brute_global", sgn, flat)
    if v == 0 and queue and n >= 320:
        if pipe16: return SphereForm(KID_BRUTE_PIPELINE, "pipe8", sgn, flat)
        if n16 * 32 + 16 * 8 * 256 <= LDS_CAP: return SphereForm(KID_BRUTE_PIPELINE, "pipe16", sgn, flat)   # lds_paths<16, false, 8>
        return SphereForm(KID_BRUTE_PIPELINE, "pipe8_global", sgn, flat)
    if v in (0, 1):
        return SphereForm(KID_BRUTE_SINGLE, "single", sgn, flat) if single else None
    if v == 2:                                                             # lds_pixels<8, true, true, true, 16> and lds_paths<4, true, 16>
        return SphereForm(KID_BRUTE_PIPELINE, "v2", sgn, flat) if queue and pipe16 and n16 * 40 + 4 * 16 * 256 <= LDS_CAP else None
    if v == 3:
        return SphereForm(KID_BRUTE_PIPELINE, "v3", sgn, flat) if queue and pipe16 else None
    return None


def unsigned_ground_spheres(n, seed):
    """synthetic_spheres with a ground sphere large enough (reach 800 >= 342: 2 reach 7.3e-7 >= 5e-4) that rt_plan takes the
    unsigned filter (SGN=0); its top still lies at y = 0."""
    s = synthetic_spheres(n, seed)
    s[0] = rt.Sphere([0.0, -400.0, 0.0], 400.0, [0.8, 0.8, 0.8])
    return s


def unsigned_tiny_spheres(n, seed):
    """synthetic_spheres with one radius below 2^-30 (rt_plan: min_radius): SGN=0 in a compact scene."""
    s = synthetic_spheres(n, seed)
    s[-1] = rt.Sphere(list(s[-1].center), 2.0 ** -31, list(s[-1].color))
    return s


def beyond_filter_range(spheres, scene_of=None):
    """The same spheres, camera and light offset beyond 2^20 (rt_plan: filter_ok false): every mode renders them literally."""
    off = np.array([3.0e6, -2.0e6, 1.5e6])
    moved = [rt.Sphere(off + np.asarray(s.center, np.float64), s.radius, list(s.color)) for s in spheres]
    scene = rt.SceneRaytracing().createScene(moved)
    scene.camera.position = list(off + np.asarray(scene.camera.position, np.float64))
    scene.camera.update()
    scene.light.position = list(off + np.asarray(scene.light.position, np.float64))
    return scene


def non_cube_sky(seed):
    """Six 6x5 faces: neither flat nor seamless (rt_enqueue: sky_seamless = 0)."""
    return random_sky(seed, w=6, h=5)


class SphereCase:
    """One cell of tests/test_sphere_forms_gpu.py: a scene of `n` spheres (sgn 1: synthetic_spheres; 0: its unsigned twin,
    `unsigned` = "ground" or "tiny"; far: offset beyond the filter's range), a sky ("flat", "cube": 8x8 random faces,
    "noncube": 6x5), the mode and variant, and the form (and list capacity) expected_sphere_form must give it.  `beside`:
    the count on the other side of the nearest LDS boundary and the form it must land in instead (None: refused)."""
    def __init__(self, name, form, n, sgn, sky, beside, strict=False, variant=0, unsigned="ground", far=False, cap=None,
                 W=160, H=96, B=4, seed=7):
        self.name, self.form, self.n, self.sgn, self.sky_kind, self.beside = name, form, n, sgn, sky, beside
        self.strict, self.variant, self.unsigned, self.far, self.cap = strict, variant, unsigned, far, cap
        self.W, self.H, self.B, self.seed = W, H, B, seed

    def scene(self, n=None):
        n = self.n if n is None else n
        build = synthetic_spheres if self.sgn != 0 else (unsigned_ground_spheres if self.unsigned == "ground" else unsigned_tiny_spheres)
        spheres = build(n, self.seed)
        return beyond_filter_range(spheres) if self.far else rt.SceneRaytracing().createScene(spheres)

    def sky(self):
        if self.sky_kind == "flat": return rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA)
        return random_sky(self.seed + self.n) if self.sky_kind == "cube" else non_cube_sky(self.seed + self.n)

    def expected(self, n=None, scene=None):
        return expected_sphere_form(scene if scene is not None else self.scene(n), self.B, self.strict, self.variant, self.sky())


def _sphere_cases():
    cases = []
    # frame size and bounces per (SGN, sky) cell: ragged widths and heights in half of them
    frames = {(1, "flat"): (160, 96, 4), (1, "tex"): (157, 91, 5), (0, "flat"): (157, 91, 3), (0, "tex"): (160, 96, 4)}
    # literal forms (rt_kernels.hip launch_strict; no SGN), strict mode: the last count of each form and the first beyond the 3rd
    for form, n, beside, skies in (("literal8", 1194, (1195, "literal16_w"), ("flat", "cube")),
                                   ("literal16_w", 3413, (3414, "literal16"), ("flat", "cube")),
                                   ("literal16", 5120, (5121, "literal_global"), ("flat", "noncube")),
                                   ("literal_global", 5121, (5120, "literal16"), ("flat", "cube"))):
        for sky in skies:
            W, H, B = frames[(1, "flat" if sky == "flat" else "tex")]
            cases.append(SphereCase("strict-%s-%s" % (form, sky), form, n, None, sky, beside, strict=True, W=W, H=H, B=B))
    # ... and the two 16-wave ones in fast mode, for a scene beyond the filter's range (filter_ok false), at their first counts
    for form, n, beside, sky in (("literal16_w", 1195, (1194, "literal8"), "flat"), ("literal16_w", 1195, (1194, "literal8"), "cube"),
                                 ("literal16", 3414, (3413, "literal16_w"), "flat"), ("literal16", 3414, (3413, "literal16_w"), "noncube")):
        W, H, B = frames[(0, "flat" if sky == "flat" else "tex")]
        cases.append(SphereCase("far-%s-%s" % (form, sky), form, n, None, sky, beside, far=True, W=W, H=H, B=B))
    # brute-force forms (rt_kernels.hip fast_form) at their LDS limits; hierarchy forms (rt_bvh.hip launch_bvh) at the last
    # count of each form, counts from expected_sphere_form (tests/test_sphere_forms_cpu.py)
    brute = (("single", 2176, 1, (2177, None)), ("pipe8", 3264, 5, (3265, "pipe16")), ("pipe16", 4096, 5, (4097, "pipe8_global")),
             ("pipe8_global", 4608, 5, (4609, "brute_global")), ("brute_global", 4609, 5, (4608, "pipe8_global")),
             ("v2", 3264, 2, (3265, None)), ("v3", 3264, 3, (3265, None)))
    bvh = (("bvh8", 12, 1184, (1185, "bvh12", 12)), ("bvh12", 12, 1789, (1790, "bvh12", 6)), ("bvh12", 6, 2106, (2107, "bvh16", 12)),
           ("bvh16", 12, 4338, (4339, "bvh16", 6)), ("bvh16", 6, 4724, (4725, "bvh_global", 8)), ("bvh_global", 8, 4725, (4724, "bvh16", 6)))
    rows = [(f, None, n, v, b) for f, n, v, b in brute] + [(f, c, n, 0, b) for f, c, n, b in bvh]
    for i, (form, cap, n, variant, beside) in enumerate(rows):
        for sgn in (1, 0):
            for tex in (False, True):
                sky = "flat" if not tex else ("cube" if sgn == 1 else "noncube")
                W, H, B = frames[(sgn, "tex" if tex else "flat")]
                uns = "ground" if i % 2 == 0 else "tiny"
                name = "%s%s-sgn%d-%s" % (form, "" if cap is None else "-cap%d" % cap, sgn, sky)
                cases.append(SphereCase(name, form, n, sgn, sky, beside, variant=variant, unsigned=uns, cap=cap, W=W, H=H, B=B))
    return cases


SPHERE_CASES = _sphere_cases()


def crowded_spheres(n, seed, unsigned=False):
    """n - 1 heavily overlapping spheres in a 5-unit box in front of the reference's camera, over a ground sphere (unsigned: the
    large one of unsigned_ground_spheres): every primary ray crosses dozens of them, so the hierarchy's candidate lists fill
    to their last row."""
    rng = np.random.default_rng(seed)
    g = rt.Sphere([0.0, -400.0, 0.0], 400.0, [0.8, 0.8, 0.8]) if unsigned else rt.Sphere([0.0, -100.0, 0.0], 100.0, [0.8, 0.8, 0.8])
    pos = np.stack([rng.uniform(-2.5, 2.5, n - 1), rng.uniform(0.5, 5.5, n - 1), rng.uniform(-12.5, -7.5, n - 1)], axis=1)
    return [g] + [rt.Sphere(p, float(rng.uniform(0.3, 0.9)), rng.uniform(0.2, 1.0, 3)) for p in pos]


# crowded_spheres scenes for the 12- and 16-wave hierarchy forms: (count, form, list capacity, SGN, sky)
CROWDED_CASES = ((1700, "bvh12", 12, 1, "cube"), (1700, "bvh12", 12, 0, "flat"), (2000, "bvh12", 6, 1, "flat"), (2000, "bvh12", 6, 0, "cube"),
                 (3000, "bvh16", 12, 1, "flat"), (3000, "bvh16", 12, 0, "noncube"), (4500, "bvh16", 6, 1, "cube"), (4500, "bvh16", 6, 0, "flat"))


def crowded_case(n, sgn, sky):
    scene = rt.SceneRaytracing().createScene(crowded_spheres(n, 5, unsigned=sgn == 0))
    s = (rt.CubemapMaterial.constant(CONSTANT_SKY_RGBA) if sky == "flat" else random_sky(n) if sky == "cube" else non_cube_sky(n))
    return scene, s


# ---- the sphere hierarchy's records restated (tests/test_hierarchy_cpu.py, test_refit_model_cpu.py, test_moving_spheres_gpu.py) ----
LEAF = 0x80000000
FILTER_SCALE = 2.0 ** 40                                                  # rt_filter.h: RT_FILTER_SCALE (its square: SCALE2)
FILTER_EPS, FILTER_KAPPA = 2.0 ** -17, 2.0 ** -16                         # RT_FILTER_EPS, RT_FILTER_KAPPA
BVH_SIGMA = 1.04                                                          # rt_bvh_build.h: RT_BVH_SIGMA


def build_hierarchy(records):
    """rt_build_hierarchy of (n, 8) float32 records: (rec4 (m+1, 4), link (m+1,), m), sentinel included."""
    import ctypes
    from compute_raytracer_amd import abi
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
    n = rec.shape[0]
    cap = 2 * n + 64
    out, link, nodes = np.zeros((cap, 4), np.float32), np.zeros(cap, np.uint32), ctypes.c_uint32(0)
    fp = ctypes.POINTER(ctypes.c_float)
    abi.check(abi.load().rt_build_hierarchy(rec.ctypes.data_as(fp), n, out.ctypes.data_as(fp),
                                            link.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap, ctypes.byref(nodes)))
    m = nodes.value
    return out[: m + 1].copy(), link[: m + 1].copy(), m


def _members_f64(records):
    """centres and |radius| in f64 with NaN taken as 0 (rt_bvh_build.h cx / rad, rt_bvh.hip bvh_refit: sphere)"""
    rec = np.asarray(records, np.float32).reshape(-1, 8)
    c = rec[:, 0:3].astype(np.float64)
    r = np.abs(rec[:, 7].astype(np.float64))
    c[np.isnan(c)] = 0.0
    r[np.isnan(r)] = 0.0
    return c, r


def leaf_records(records):
    """The filter record of each sphere, as rt_kernels.hip prep_spheres writes geo_f (and bvh_fill_leaves copies it into the
    hierarchy's leaves): centre * 2^40 in f32, k = fl32((|c|^2 (1-eps) - fl32(r*r) (1+kappa)) * 2^80) with |c|^2 in f64."""
    rec = np.asarray(records, np.float32).reshape(-1, 8)
    c = rec[:, 0:3]
    r2 = rec[:, 7] * rec[:, 7]                                            # f32 product (HK:310 radius * radius)
    cd = c.astype(np.float64)
    cd2 = cd[:, 0] * cd[:, 0] + cd[:, 1] * cd[:, 1] + cd[:, 2] * cd[:, 2]
    k = cd2 * (1.0 - FILTER_EPS) - r2.astype(np.float64) * (1.0 + FILTER_KAPPA)
    out = np.empty((rec.shape[0], 4), np.float32)
    out[:, 0:3] = c * np.float32(FILTER_SCALE)
    out[:, 3] = (k * FILTER_SCALE ** 2).astype(np.float32)
    return out


def refit_model(rec4, link, records):
    """rt_bvh.hip bvh_refit, restated operation by operation in f64, for the topology `link` (rt_build_hierarchy's layout)
    over `records`: every inner node's bound from its members (the leaves between it and its skip link) -- the centre of
    their box, then up to 32 greedy steps of 0.05 R towards the farthest member while the radius falls, the centre rounded to
    f32, the radius about that point times 1.04, k = |C|^2 (1-eps) - R^2 (1+kappa) in f64 rounded once to f32.  The
    farthest member is the kernel's: member j sits on lane (j - first) % 64 (first = node + 1), each lane keeps the first
    strict maximum of its stride, the lowest lane holding the wave's maximum speaks.  Leaves are the filter records
    (leaf_records: bvh_fill_leaves), the sentinel is kept from rec4.  All nodes are refitted at once, one segment per node."""
    rec4 = np.asarray(rec4, np.float32)
    link = np.asarray(link, np.uint32)
    m = link.shape[0] - 1
    out = rec4.copy()
    is_leaf = (link[:m] & LEAF) != 0
    sph = (link[:m] & 0x7FFFFFFF).astype(np.int64)
    out[:m][is_leaf] = leaf_records(records)[sph[is_leaf]]
    inner = np.nonzero(~is_leaf)[0]
    if inner.size == 0:
        return out
    c, r = _members_f64(records)
    leaf_at = np.nonzero(is_leaf)[0]
    segs = [leaf_at[np.searchsorted(leaf_at, i + 1): np.searchsorted(leaf_at, int(link[i]) >> 2)] for i in inner]
    counts = np.array([len(g) for g in segs])
    assert (counts >= 1).all(), "an inner node without members"
    j = np.concatenate(segs)                                              # member node indices, node by node
    seg = np.repeat(np.arange(inner.size), counts)                        # segment (inner node) of each member
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    jrel = j - (inner[seg] + 1)
    key = (jrel % 64) * (1 << 32) + jrel                                  # (lane, position in the lane's stride)
    cm, rm = c[sph[j]], r[sph[j]]

    def radius_at(P):
        dx = cm - P[seg]
        d = np.sqrt(dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1] + dx[:, 2] * dx[:, 2]) + rm
        R = np.maximum.reduceat(d, starts)
        kmin = np.minimum.reduceat(np.where(d == R[seg], key, np.iinfo(np.int64).max), starts)
        far = c[sph[inner + 1 + (kmin & 0xFFFFFFFF)]]
        return R, far

    mn = np.minimum.reduceat(cm - rm[:, None], starts, axis=0)
    mx = np.maximum.reduceat(cm + rm[:, None], starts, axis=0)
    P = 0.5 * (mn + mx)
    Rp, far = radius_at(P)
    active = np.ones(inner.size, bool)
    for _ in range(32):
        s = far - P
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        active &= ln > 1e-12
        if not active.any():
            break
        Q = P + s / np.where(active, ln, 1.0)[:, None] * 0.05 * Rp[:, None]
        Rq, farq = radius_at(Q)
        active &= Rq < Rp
        P = np.where(active[:, None], Q, P)
        Rp = np.where(active, Rq, Rp)
        far = np.where(active[:, None], farq, far)
    C = P.astype(np.float32)
    Cd = C.astype(np.float64)
    R = radius_at(Cd)[0] * BVH_SIGMA
    c2 = Cd[:, 0] * Cd[:, 0] + Cd[:, 1] * Cd[:, 1] + Cd[:, 2] * Cd[:, 2]
    k = c2 * (1.0 - FILTER_EPS) - R * R * (1.0 + FILTER_KAPPA)
    out[inner, 0:3] = C * np.float32(FILTER_SCALE)
    out[inner, 3] = (k * FILTER_SCALE ** 2).astype(np.float32)
    return out


def check_tree(rec, out, link, m, tight=True):
    """The invariants the device walk relies on, for n (n, 8) records and a hierarchy (out (m+1, 4), link (m+1,)) in
    rt_build_hierarchy's layout: depth-first layout with forward skip links and a self-linked sentinel, every sphere a leaf
    exactly once, every inner node containing its members with the 4 % slack of the proof (rt_bvh.hip, header).
    tight: the host build's records -- leaves zero (the device fills them), radii within 5 % of the members' bound.  False:
    records refitted on the device (bvh_refit) or by refit_model, whose centre comes from the greedy walk alone and whose
    leaves hold the filter records (compared with leaf_records elsewhere): the slack bound only."""
    rec = np.asarray(rec, np.float32).reshape(-1, 8)
    n = rec.shape[0]
    S = FILTER_SCALE
    assert n <= m <= 2 * n + 64
    assert link[m] == 4 * m and np.isinf(out[m, 3]) and out[m, 3] > 0          # sentinel
    leaves = link[:m][(link[:m] & LEAF) != 0] & 0x7FFFFFFF
    assert sorted(leaves.tolist()) == list(range(n))                            # every sphere exactly once
    c, r = _members_f64(rec)
    for i in range(m):
        if link[i] & LEAF:
            if tight:
                assert not out[i].any()                                         # filled on the device
            continue
        assert link[i] % 4 == 0
        end = link[i] // 4
        assert i + 1 < end <= m                                                 # forward link, non-empty subtree
        inner = [j for j in range(i + 1, end) if not (link[j] & LEAF)]
        assert all(link[j] // 4 <= end for j in inner)                          # nested subtrees
        members = link[i + 1 : end][(link[i + 1 : end] & LEAF) != 0] & 0x7FFFFFFF
        assert len(members) >= 2
        C = out[i, 0:3].astype(np.float64) / S
        k = float(out[i, 3]) / (S * S)
        c2 = float(C @ C)
        need = (np.linalg.norm(c[members] - C, axis=1) + r[members]).max()
        # k = |C|^2 (1-eps) - R^2 (1+kappa) with R >= 1.04 * need, stored in fp32 (the eps term of the
        # node test covers that rounding, 2^-24 |k|, many times over)
        round_k = 2.0 ** -23 * max(c2, need * need)
        k_slack = c2 * (1.0 - FILTER_EPS) - (1.04 * need) ** 2 * (1.0 + FILTER_KAPPA)
        assert k <= k_slack + round_k, (i, k, k_slack)          # the radius carries the 4 % slack of the proof
        if tight:
            k_tight = c2 * (1.0 - FILTER_EPS) - (1.05 * need) ** 2 * (1.0 + FILTER_KAPPA)
            assert k >= k_tight - round_k - 1e-12, (i, k, k_tight)  # and not much more


def drift_spheres(base, step, seed, keep=(0,)):
    """(n, 8) records moved by `step`: every sphere but those in `keep` (a ground sphere, a tiny one: what puts the scene in
    its filter class) drifts and breathes, and n // 50 of them, chosen by `seed`, jump across the scene's box."""
    s = np.array(base, np.float32).reshape(-1, 8).copy()
    n = s.shape[0]
    mv = np.setdiff1d(np.arange(n), np.asarray(keep, np.int64))
    s[mv, 0] += (0.35 * step * np.sin(mv * 0.37)).astype(np.float32)
    s[mv, 1] += (0.20 * step * np.abs(np.cos(mv * 0.11))).astype(np.float32)
    s[mv, 2] += (0.30 * step * np.cos(mv * 0.23)).astype(np.float32)
    s[mv, 7] *= (1.0 + 0.04 * step * np.sin(mv * 0.5)).astype(np.float32)
    rng = np.random.default_rng(seed)
    jump = rng.choice(mv, size=max(1, n // 50), replace=False)
    s[jump, 0] = rng.uniform(-12, 12, len(jump)).astype(np.float32)
    s[jump, 2] = rng.uniform(-26, -3, len(jump)).astype(np.float32)
    return s


def teleport_spheres(base, seed, keep=(0,)):
    """every sphere but those in `keep` somewhere else in the scene's box: a topology built for `base` groups them at random"""
    s = np.array(base, np.float32).reshape(-1, 8).copy()
    mv = np.setdiff1d(np.arange(s.shape[0]), np.asarray(keep, np.int64))
    rng = np.random.default_rng(seed)
    s[mv, 0] = rng.uniform(-12, 12, len(mv)).astype(np.float32)
    s[mv, 1] = rng.uniform(0.05, 3, len(mv)).astype(np.float32)
    s[mv, 2] = rng.uniform(-26, -3, len(mv)).astype(np.float32)
    return s


# Motions (drift_spheres seed, step) of two SPHERE_CASES cells whose fresh build lands on the other side of the cell's LDS edge,
# and the form (and list capacity) it lands in (tests/test_refit_model_cpu.py checks them, test_moving_spheres_gpu.py hands
# such a topology over)
MOVING_BOUNDARY_MOTIONS = {"bvh8-cap12-sgn1-flat": (0, 2, ("bvh12", 12)), "bvh16-cap6-sgn1-flat": (0, 3, ("bvh_global", 8))}
