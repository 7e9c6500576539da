"""RendererRaytracing -- host-side mirror of src/rendering-raycast/renderer-raytracing.ts.

Same surface as the reference class (RR:53-76, RR:434): construct with (width, height, scene)
-- the canvas argument is dropped, there is no canvas in a headless renderer --, `initialize()`,
`render()`, `showRaytracer()`, `showHeatmap()`.  Every WebGPU call of the reference is replaced
by the C-ABI call include/rt355.h lists next to it.  The frame is the rgba8unorm colour buffer
itself (RR:102-109); the blit to the canvas (RR:449-463) has no counterpart.

No CPU fallback: without librt355.so and a gfx950 device, `initialize()` raises.
"""
import contextlib
import ctypes

import numpy as np

from . import abi
from .cubemap_material import CubemapMaterial
from .scene_raytracing import CONSTANT_SKY_RGBA


def ao_directions(k):
    """k directions over the hemisphere z > 0 with density proportional to z (cosine-weighted), as (k, 3) float32 of unit length to
    float32 rounding: point i of the Hammersley set ((i + 0.5) / k, the base-2 radical inverse of i) mapped through the disc
    (Malley's method).  The same bits on every call; render_ao's default rays."""
    k = int(k)
    if k < 1:
        raise ValueError("ao_directions: k must be at least 1")
    i = np.arange(k, dtype=np.uint64)
    u = (i.astype(np.float64) + 0.5) / k                                 # in (0, 1): z = sqrt(1 - u) > 0
    v = np.zeros(k, np.float64)
    bit, scale = i.copy(), 0.5
    while bit.any():                                                     # the radical inverse: the bits of i mirrored about the point
        v += scale * (bit & np.uint64(1)).astype(np.float64)
        bit >>= np.uint64(1)
        scale *= 0.5
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    d = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], axis=1)
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return d.astype(np.float32)


class RendererRaytracing:
    def __init__(self, width, height, scene, device=0, maxBounces=4, rank=0, world=1):
        self.scene = scene                     # RR:54
        self.width = int(width)                # RR:56-57
        self.height = int(height)
        self.device = int(device)
        # RR:157 hard-codes maxBounces = 4; it already travels in the uniform (RK:10), so the
        # BASELINE configs simply set it.
        self.maxBounces = maxBounces
        self.rank, self.world = int(rank), int(world)
        self.skyboxMaterial = None             # RR:33
        self.meshMaterial = None               # RR:32 mouseyMaterial (the mesh texture, binding 8)
        self.loaded = False                    # RR:51
        self.render_time_ms = None             # the 'render-time' label of RR:468-469
        self._ctx = None
        self._lib = None
        self._pinned = []

    # ---- RR:62-68 -------------------------------------------------------------------------
    def initialize(self, skybox=None, meshMaterial=None):
        self._lib = abi.load()
        ctx = ctypes.c_void_p()
        abi.check(self._lib.rt_create(self.device, ctypes.byref(ctx)))           # RR:78-97 setupDevice
        self._ctx = ctx
        self.meshMaterial = meshMaterial
        self._create_assets(skybox)                                              # RR:99-153
        self.showRaytracer()                                                     # RR:356-365
        return self

    def _create_assets(self, skybox):
        L, c = self._lib, self._ctx
        self.skyboxMaterial = skybox if skybox is not None else CubemapMaterial.constant(CONSTANT_SKY_RGBA)
        for i, face in enumerate(self.skyboxMaterial.faces):                     # CM:73-77
            f = np.ascontiguousarray(face, dtype=np.uint8)
            abi.check(L.rt_write_cubemap_face(c, i, f.shape[1], f.shape[0], f.ctypes.data), c)
        abi.check(L.rt_set_partition(c, self.rank, self.world), c)
        abi.check(L.rt_resize(c, self.width, self.height), c)                    # RR:102-109 colorBuffer

    def showRaytracer(self):                                                     # RR:70-72
        abi.check(self._lib.rt_select_kernel(self._ctx, abi.RT_KERNEL_RAYTRACER), self._ctx)

    def showHeatmap(self):                                                       # RR:74-76
        abi.check(self._lib.rt_select_kernel(self._ctx, abi.RT_KERNEL_HEATMAP), self._ctx)

    def set_mode(self, strict):
        abi.check(self._lib.rt_set_mode(self._ctx, abi.RT_MODE_STRICT if strict else abi.RT_MODE_FAST), self._ctx)

    def set_variant(self, variant):
        abi.check(self._lib.rt_set_variant(self._ctx, int(variant)), self._ctx)

    # ---- RR:155-230 -----------------------------------------------------------------------
    def recalculateScene(self):
        L, c = self._lib, self._ctx
        p = self.scene.pack_params(self.maxBounces)                              # RR:157-165
        abi.check(L.rt_write_params(c, p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), c)
        fp = ctypes.POINTER(ctypes.c_float)
        if self.scene.hasTriangles:                                                 # the reference's live scene type
            b = np.ascontiguousarray(self.scene.pack_blas(), dtype=np.float32)           # RR:169-174
            abi.check(L.rt_write_blas(c, b.ctypes.data_as(fp), b.shape[0]), c)
            bl = np.ascontiguousarray(self.scene.pack_blas_lookup(), dtype=np.float32)   # RR:177-181
            abi.check(L.rt_write_blas_lookup(c, bl.ctypes.data_as(fp), bl.shape[0]), c)
            na = np.ascontiguousarray(self.scene.pack_tlas_nodes(), dtype=np.float32)    # RR:184-192
            abi.check(L.rt_write_nodes(c, 0, na.ctypes.data_as(fp), na.shape[0]), c)
        if self.loaded:                                                          # RR:194-195
            return
        self.loaded = True
        if self.scene.hasTriangles:
            t = np.ascontiguousarray(self.scene.pack_triangles(), dtype=np.float32)      # RR:198-209
            abi.check(L.rt_write_triangles(c, t.ctypes.data_as(fp), t.shape[0]), c)
            nb = np.ascontiguousarray(self.scene.pack_blas_nodes(), dtype=np.float32)    # RR:212-223
            abi.check(L.rt_write_nodes(c, 32 * self.scene.tlasNodesMax, nb.ctypes.data_as(fp), nb.shape[0]), c)
            tl = np.ascontiguousarray(self.scene.pack_tri_lookup(), dtype=np.float32)    # RR:225-229
            abi.check(L.rt_write_tri_lookup(c, tl.ctypes.data_as(fp), tl.shape[0]), c)
            if self.meshMaterial is not None:                                            # RR:113-114 mouseyMaterial
                img = np.ascontiguousarray(self.meshMaterial.image, dtype=np.uint8)
                abi.check(L.rt_write_mesh_texture(c, img.shape[1], img.shape[0], img.ctypes.data), c)
            return
        s = np.ascontiguousarray(self.scene.pack_spheres(), dtype=np.float32)    # in place of RR:198-229
        abi.check(L.rt_write_spheres(c, s.ctypes.data_as(fp), s.shape[0]), c)

    # ---- deforming meshes: partial triangle writes and the device refit (rt_update_triangles / rt_refit_blas / rt_read_nodes) ----
    def update_triangles(self, first, records):
        """Replaces triangle records [first, first + n) -- (n, 40) float32 in pack_triangles' layout -- on the device and in the
        scene's packed `triangles` (the scene is uploaded first if it has not been: recalculateScene()).  A contiguous float32
        (n, 40) torch tensor on this renderer's device is copied there, on torch's current stream (rt_update_triangles_device).  No
        node changes: follow it with refit().  Drains the frames in flight."""
        first = int(first)
        if self._is_tensor(records):                                               # (n, 40) on this renderer's device: read there
            self._check_deform_tensor("update_triangles", "records", records, ((None, 40),))
            self.recalculateScene()
            with self._current_stream(records.device) as stream:
                abi.check(self._lib.rt_update_triangles_device(self._ctx, first, records.shape[0], ctypes.c_void_p(records.data_ptr()), stream), self._ctx)
            self._mirror_triangles(first, self.read_triangles(first, records.shape[0]))
            return
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 40)
        self.recalculateScene()
        abi.check(self._lib.rt_update_triangles(self._ctx, first, rec.shape[0], rec.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        self._mirror_triangles(first, rec)

    def _mirror_triangles(self, first, rec):
        tris = np.array(self.scene.static["triangles"], dtype=np.float32)          # a copy: packed arrays may be shared between scenes
        tris[first:first + rec.shape[0]] = rec
        self.scene.static["triangles"] = tris

    @staticmethod
    def _is_tensor(x):
        return x is not None and type(x).__module__.split(".")[0] == "torch"

    def _check_deform_tensor(self, who, name, t, shapes, dtype="float32"):
        """A contiguous tensor of `dtype` on this renderer's device with one of `shapes` (None: any extent), as build_top_level
        asks of its matrices."""
        import torch
        fits = any(len(s) == t.dim() and all(w is None or w == g for w, g in zip(s, t.shape)) for s in shapes)
        if t.dtype != getattr(torch, dtype) or not fits or not t.is_contiguous():
            want = " or ".join("(%s)" % ", ".join("n" if w is None else str(w) for w in s) for s in shapes)
            raise ValueError("%s: %s must be a contiguous %s %s tensor" % (who, name, dtype, want))
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError("%s: %s must live on cuda:%d, this renderer's device" % (who, name, self.device))

    def deform(self, first, vertices, faces=None, normals=None, flat_normals=False, refit=True):
        """New corner positions for triangles [first, first + T) from vertex arrays, with no 40-float records on the caller's
        side.  vertices: float32 (V, 3), or (T, 3, 3) -- three corners per triangle; faces: int32 (T, 3) indices into
        `vertices` (an index at or beyond V reads vertex V - 1; negative ones too), None: triangle i takes vertices 3 i .. 3 i + 2;
        normals: float32, per vertex like `vertices`, written to the corners' normals; flat_normals: the three corners get the
        unit normal of the new triangle instead (not together with normals); with neither the normals stay.  uv, colour and
        every other triangle keep their bytes.  torch tensors on this renderer's device are read there, on torch's current
        stream (rt_deform_triangles), and nothing crosses to the host but the read-back below; numpy arrays are staged
        (rt_deform_triangles_host).  All arrays of one call are of one kind.  Afterwards the scene's packed `triangles` are
        the device's bytes for the range, so scene.to_packed() describes exactly what frames read.  refit: refit() follows --
        new boxes for every bottom-level tree.  The top-level tree made by scene.update(dt) has placeholder boxes and needs
        nothing; a tight one (build_top_level()) must be built again after a deformation that grows a root box: call
        build_top_level() afterwards.  Drains the frames in flight."""
        who = "deform"
        first = int(first)
        if flat_normals and normals is not None:
            raise ValueError("deform: flat_normals and normals exclude each other")
        flags = abi.RT_DEFORM_FLAT_NORMALS if flat_normals else 0
        arrays = [a for a in (vertices, faces, normals) if a is not None]
        on_device = self._is_tensor(vertices)
        if any(self._is_tensor(a) != on_device for a in arrays):
            raise ValueError("deform: vertices, faces and normals must be all torch tensors or all numpy arrays")
        if on_device:
            per_vertex = ((None, 3), (None, 3, 3))
            self._check_deform_tensor(who, "vertices", vertices, per_vertex)
            if faces is not None:
                self._check_deform_tensor(who, "faces", faces, ((None, 3),), "int32")
            if normals is not None:
                self._check_deform_tensor(who, "normals", normals, per_vertex)
                if normals.numel() != vertices.numel():
                    raise ValueError("deform: normals must have one row per vertex")
            V = vertices.numel() // 3
            n = faces.shape[0] if faces is not None else V // 3
            ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        else:
            vertices = np.ascontiguousarray(vertices, dtype=np.float32)
            if vertices.ndim not in (2, 3) or vertices.shape[1:] not in ((3,), (3, 3)):
                raise ValueError("deform: vertices must be (V, 3) or (T, 3, 3)")
            V = vertices.size // 3
            if faces is not None:
                faces = np.ascontiguousarray(np.asarray(faces).astype(np.int64).astype(np.uint32))
                if faces.ndim != 2 or faces.shape[1] != 3:
                    raise ValueError("deform: faces must be (T, 3)")
            if normals is not None:
                normals = np.ascontiguousarray(normals, dtype=np.float32)
                if normals.size != vertices.size:
                    raise ValueError("deform: normals must have one row per vertex")
            n = faces.shape[0] if faces is not None else V // 3
            ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        if faces is None and V != 3 * n:
            raise ValueError("deform: without faces the vertex count must be a multiple of 3")
        self.recalculateScene()
        head = (self._ctx, first, n, ptr(vertices), V, ptr(faces), ptr(normals), flags)
        if on_device:
            with self._current_stream(vertices.device) as stream:
                abi.check(self._lib.rt_deform_triangles(*head, stream), self._ctx)
        else:
            abi.check(self._lib.rt_deform_triangles_host(*head), self._ctx)
        self._mirror_triangles(first, self.read_triangles(first, n))
        if refit:
            self.refit()

    def read_triangles(self, first=0, n=None):
        """(n, 40) float32: triangle records [first, first + n) on the device, as the next frame would read them (n None: up to the
        scene's last triangle).  A diagnostic: it waits for the frames in flight."""
        first = int(first)
        n = self.scene.triangleCount - first if n is None else int(n)
        out = np.zeros((max(n, 0), 40), dtype=np.float32)
        abi.check(self._lib.rt_read_triangles(self._ctx, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        return out

    def refit(self, roots=None):
        """New boxes for the bottom-level trees under `roots` (node indices: a mesh's root_node; None: every root the instances
        name), computed on the device from the triangles it holds.  Afterwards the scene's packed `blas_nodes` are the device's
        bytes, so scene.to_packed() describes exactly what frames and queries read.  The top-level tree is built from the meshes'
        placeholder boxes (scene-raytracing.ts) and does not change.  Drains the frames in flight."""
        self.recalculateScene()
        if roots is None:
            abi.check(self._lib.rt_refit_blas(self._ctx, None, 0), self._ctx)
        else:
            r = np.ascontiguousarray(np.asarray(roots, dtype=np.int64).reshape(-1).astype(np.uint32))
            abi.check(self._lib.rt_refit_blas(self._ctx, r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), r.shape[0]), self._ctx)
        self.scene.static["blas_nodes"] = self.read_nodes(self.scene.tlasNodesMax, self.scene.blasNodesUsed)

    def read_nodes(self, first=0, n=None):
        """(n, 8) float32: nodes [first, first + n) of the node buffer as the next frame would read them (n None: up to the end of
        the scene's buffer).  A diagnostic: it waits for the frames in flight."""
        first = int(first)
        n = self.scene.node_buffer_length() - first if n is None else int(n)
        out = np.zeros((max(n, 0), 8), dtype=np.float32)
        abi.check(self._lib.rt_read_nodes(self._ctx, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        return out

    # ---- device BLAS builds (rt_build_blas / rt_read_tri_lookup) ----
    def rebuild(self, meshes=None):
        """The bottom-level trees of `meshes` (indices into scene.meshes; None: all of them) built anew on the device from the
        triangles it holds: the host builder's SAH tree of the mesh as it is now, where refit() only moves the boxes of the tree
        it was given.  Each tree may use the nodes from its mesh's root up to the next mesh's root (the end of the buffer for the
        last one): a tree that needs more raises RtError(RT_ERR_CAPACITY) with the counts, and nothing has changed -- lay such a
        scene out with createTriangleScene(..., node_capacity="full").  Afterwards the scene's packed `blas_nodes` and
        `tri_lookup` are the device's bytes.  Returns the node count of each tree built.  Drains the frames in flight."""
        self.recalculateScene()
        sc = self.scene
        which = list(range(len(sc.meshes))) if meshes is None else [int(m) for m in meshes]
        roots = sorted(m.root_node for m in sc.meshes) + [sc.node_buffer_length()]
        ranges = np.zeros(len(which), dtype=abi.BLAS_RANGE_DTYPE)
        for k, m in enumerate(which):
            mesh = sc.meshes[m]
            nxt = min(r for r in roots if r > mesh.root_node)
            ranges[k] = (mesh.root_node, nxt - mesh.root_node, mesh.lookup_offset, mesh.soup.count)
        used = np.zeros(max(len(which), 1), dtype=np.uint32)
        rc = self._lib.rt_build_blas(self._ctx, ranges.ctypes.data_as(ctypes.POINTER(abi.RtBlasRange)), len(which),
                                     used.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        if rc == abi.RT_ERR_CAPACITY:
            short = ["mesh %d needs %d nodes, has %d" % (m, u, r["node_cap"]) for m, u, r in zip(which, used, ranges) if u > r["node_cap"]]
            raise abi.RtError(rc, "rebuild: " + "; ".join(short) + ' (createTriangleScene(..., node_capacity="full") reserves 2 T - 1 per mesh)')
        abi.check(rc, self._ctx)
        sc.static["blas_nodes"] = self.read_nodes(sc.tlasNodesMax, sc.blasNodesUsed)
        sc.static["tri_lookup"] = self.read_tri_lookup()
        return [int(u) for u in used[:len(which)]]

    def read_tri_lookup(self, first=0, n=None):
        """(n,) float32: slots [first, first + n) of the triangle lookup table on the device (n None: up to the end of the scene's
        table).  A diagnostic: it waits for the frames in flight."""
        first = int(first)
        n = self.scene.triangleCount - first if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=np.float32)
        abi.check(self._lib.rt_read_tri_lookup(self._ctx, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        return out

    # ---- device top-level builds (rt_build_tlas / rt_build_tlas_device / rt_read_blas / rt_read_blas_lookup) ----
    def build_top_level(self, matrices=None):
        """The per-frame instance state -- BLAS records, BLAS lookup and the top-level tree -- made on the device: a SAH tree over
        the instances' tight world boxes, taken from the root boxes the device holds now (after any refit() or rebuild()), where
        scene.update(dt) builds the reference's tree over placeholder boxes that every ray enters.  `matrices`: (M, 16) float32
        forward instance matrices, column-major, in scene.instances order; None: scene.instances.matrices(); a torch tensor on this
        renderer's device is read there, on torch's current stream.  Afterwards scene.frame and scene.tlasNodesUsed are the
        device's bytes, so recalculateScene() rewrites the same state.  scene.update(dt) still builds the reference's tree: call
        build_top_level() after it, and again after anything that grows a root box (update_triangles() + refit(), rebuild()) --
        the boxes are tight, a stale top level can lose hits.  On exact-t ties between instances the winning (instance, prim) may
        differ from the reference tree's; t never does.  For a handful of instances the host recipe is the faster one.  Returns
        {nodes_used, depth, leaves, max_leaf}.  Drains the frames in flight."""
        self.recalculateScene()
        sc = self.scene
        roots = np.ascontiguousarray([sc.meshes[k].root_node for k in sc.instances.mesh_index], dtype=np.uint32)
        info = abi.RtTlasInfo()
        tail = (roots.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), roots.shape[0], sc.tlasNodesMax, ctypes.byref(info))
        if matrices is not None and type(matrices).__module__.split(".")[0] == "torch":
            import torch
            m = matrices
            if m.dtype != torch.float32 or tuple(m.shape) != (roots.shape[0], 16) or not m.is_contiguous():
                raise ValueError("build_top_level: matrices must be a contiguous float32 (%d, 16) tensor" % roots.shape[0])
            if m.device.type != "cuda" or m.device.index != self.device:
                raise ValueError("build_top_level: matrices must live on cuda:%d, this renderer's device" % self.device)
            with self._current_stream(m.device) as stream:
                abi.check(self._lib.rt_build_tlas_device(self._ctx, ctypes.c_void_p(m.data_ptr()), *tail, stream), self._ctx)
        else:
            m = np.ascontiguousarray(sc.instances.matrices() if matrices is None else matrices, dtype=np.float32)
            if m.shape != (roots.shape[0], 16):
                raise ValueError("build_top_level: matrices must be (%d, 16), one per instance" % roots.shape[0])
            abi.check(self._lib.rt_build_tlas(self._ctx, m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), *tail), self._ctx)
        n = roots.shape[0]
        sc.frame = dict(blas=self.read_blas(0, n), blas_lookup=self.read_blas_lookup(0, n), tlas_nodes=self.read_nodes(0, sc.tlasNodesMax))
        sc.tlasNodesUsed = int(info.nodes_used)
        return dict(nodes_used=int(info.nodes_used), depth=int(info.depth), leaves=int(info.leaves), max_leaf=int(info.max_leaf))

    def read_blas(self, first=0, n=None):
        """(n, 20) float32: BLAS records [first, first + n) as the next frame would read them (n None: up to the last instance).  A
        diagnostic: it waits for the frames in flight."""
        first = int(first)
        n = len(self.scene.instances) - first if n is None else int(n)
        out = np.zeros((max(n, 0), 20), dtype=np.float32)
        abi.check(self._lib.rt_read_blas(self._ctx, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        return out

    def read_blas_lookup(self, first=0, n=None):
        """(n,) float32: BLAS lookup words [first, first + n) as the next frame would read them (n None: up to the last instance).
        A diagnostic: it waits for the frames in flight."""
        first = int(first)
        n = len(self.scene.instances) - first if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=np.float32)
        abi.check(self._lib.rt_read_blas_lookup(self._ctx, first, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._ctx)
        return out

    # ---- RR:434-470 -----------------------------------------------------------------------
    def render(self):
        import time
        t0 = time.perf_counter()                                                 # RR:435
        self.recalculateScene()                                                  # RR:437
        abi.check(self._lib.rt_render(self._ctx), self._ctx)                     # RR:442-446, 465
        abi.check(self._lib.rt_wait(self._ctx), self._ctx)                       # RR:467
        self.render_time_ms = (time.perf_counter() - t0) * 1e3                   # RR:468-469

    def enqueue(self):
        """render() without the wait (the reference never does this; bench.py uses it to time
        K frames back to back)."""
        abi.check(self._lib.rt_render(self._ctx), self._ctx)

    def wait(self):
        abi.check(self._lib.rt_wait(self._ctx), self._ctx)

    # ---- results ----------------------------------------------------------------------------
    def local_rows(self):
        rows = 0
        for j in range(abi.load().rt_tiles_of_rank(self.height, self.rank, self.world)):
            y0 = (self.rank + j * self.world) * 8
            rows += min(8, self.height - y0)
        return rows

    def read_pixels(self):
        """The rows this rank rendered, (rows, W, 4) uint8; world == 1: the whole frame."""
        rows = self.local_rows()
        out = np.empty((rows, self.width, 4), dtype=np.uint8)
        abi.check(self._lib.rt_read_pixels(self._ctx, out.ctypes.data, out.nbytes), self._ctx)
        return out

    # ---- streaming read-back: frames in flight AND copied out (rt_read_pixels_async) -----------
    def host_frames(self, n):
        """n pinned (H, W, 4) uint8 frames for read_pixels_async (freed by close())."""
        import weakref
        nbytes = self.height * self.width * 4
        out = []
        for _ in range(n):
            p = ctypes.c_void_p()
            abi.check(self._lib.rt_host_alloc(nbytes, ctypes.byref(p)))
            buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
            # the pinned memory lives as long as anything refers to it -- the arrays handed out (numpy keeps `buf` as their
            # base) or this renderer -- and is freed when the last reference goes, not at close(): a view that outlives the
            # renderer stays valid
            weakref.finalize(buf, self._lib.rt_host_free, ctypes.c_void_p(p.value))
            self._pinned.append(buf)
            out.append(np.frombuffer(buf, dtype=np.uint8).reshape(self.height, self.width, 4))
        return out

    def read_pixels_async(self, frames_back, dst):
        abi.check(self._lib.rt_read_pixels_async(self._ctx, int(frames_back), dst.ctypes.data, dst.nbytes), self._ctx)

    def read_pixels_wait(self):
        abi.check(self._lib.rt_read_pixels_wait(self._ctx), self._ctx)

    # ---- ray queries: the nearest hit of the host's rays (rt_trace_rays / rt_trace_rays_host / rt_pick) ----------------------
    def trace_rays(self, origins, directions=None, out=None, tmin=None, tmax=None, limits=False):
        """Nearest hit of each ray against the scene the next frame would render (recalculateScene() first, as render() does).

        numpy: origins and directions (n, 3) -> dict of numpy arrays t, u, v, prim, instance (n,) and normal (n, 3), through
        rt_trace_rays_host.  torch: `origins` is a float32 (n, 8) tensor {origin, -, dir, -} on this renderer's device and
        `directions` is None -> an (n, 8) float32 tensor of rt_hit records (prim / instance as int32 bits: .view(torch.int32)),
        or `out`, enqueued through rt_trace_rays on torch.cuda.current_stream().

        Limits (RT_QUERY_LIMITS, rt_trace_rays_ex): numpy -- `tmin` / `tmax`, each a scalar or an (n,) array; one of them given,
        the other is the reference's (0.001 or 9999).  torch -- `limits=True` reads words 3 and 7 of the (n, 8) tensor."""
        if type(origins).__module__.split(".")[0] == "torch":
            if tmin is not None or tmax is not None:
                raise ValueError("trace_rays: with a tensor the limits are words 3 and 7 of the rays (limits=True)")
            return self._trace_rays_torch(origins, directions, out, abi.RT_QUERY_LIMITS if limits else 0, False)
        if limits:
            raise ValueError("trace_rays: limits=True is for (n, 8) tensors; numpy rays take tmin / tmax")
        flags = abi.RT_QUERY_LIMITS if (tmin is not None or tmax is not None) else 0
        rays = self._pack_rays(origins, directions, 0.001 if tmin is None else tmin, 9999.0 if tmax is None else tmax)
        self.recalculateScene()
        hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
        if flags:
            abi.check(self._lib.rt_trace_rays_host_ex(self._ctx, rays.ctypes.data, rays.shape[0], flags, hits.ctypes.data), self._ctx)
        else:
            abi.check(self._lib.rt_trace_rays_host(self._ctx, rays.ctypes.data, rays.shape[0], hits.ctypes.data), self._ctx)
        return self._hit_dict(hits)

    def occluded(self, origins, directions=None, tmin=0.001, tmax=9999.0, out=None):
        """Whether anything blocks each ray within (tmin, tmax) (rt_occluded): exactly where trace_rays with the same limits
        reports a hit.  numpy: origins and directions (n, 3), tmin / tmax scalars or (n,) arrays -> an (n,) bool array, through
        rt_occluded_host.  torch: a float32 (n, 8) tensor {origin, tmin, dir, tmax} (tmin / tmax are then words 3 and 7; the
        keywords must stay at their defaults) -> an (n,) uint8 tensor, or `out`, on torch.cuda.current_stream()."""
        if type(origins).__module__.split(".")[0] == "torch":
            if tmin != 0.001 or tmax != 9999.0:
                raise ValueError("occluded: with a tensor the limits are words 3 and 7 of the rays")
            return self._trace_rays_torch(origins, directions, out, abi.RT_QUERY_LIMITS, True)
        rays = self._pack_rays(origins, directions, tmin, tmax)
        self.recalculateScene()
        occ = np.zeros(rays.shape[0], dtype=np.uint8)
        abi.check(self._lib.rt_occluded_host(self._ctx, rays.ctypes.data, rays.shape[0], abi.RT_QUERY_LIMITS, occ.ctypes.data),
                  self._ctx)
        return occ.astype(bool)

    # ---- instance visibility masks (rt_write_instance_masks / rt_set_query_masks): ray queries alone, frames ignore them -----
    def set_instance_masks(self, masks):
        """One 32-bit visibility mask per instance, in scene.instances order (the BLAS record order, rt_hit.instance): a sequence
        or array of integers in [0, 2**32).  Instances beyond the sequence keep 0xFFFFFFFF; None clears the table.  An instance
        is visible to a ray iff (its mask & the ray's mask) != 0 (set_query_masks).  The table belongs to no scene buffer: it
        survives every scene write.  Waits for the queries enqueued before it; frames in flight go on."""
        m = self._pack_masks(masks)
        abi.check(self._lib.rt_write_instance_masks(self._ctx, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if m.size else None,
                                                    m.size), self._ctx)

    def set_query_masks(self, nearest=0xFFFFFFFF, occlusion=0xFFFFFFFF):
        """The masks the rays of later queries carry, copied at each query call.  `nearest`: trace_rays, trace_rays_multi, pick,
        render_gbuffer, the primary ray of render_ao and every ray of shade_rays and render_samples.  `occlusion`: occluded and
        the k rays of render_ao."""
        masks = []
        for name, value in (("nearest", nearest), ("occlusion", occlusion)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) < 2 ** 32:
                raise ValueError("set_query_masks: %s must be an integer in [0, 2**32)" % name)
            masks.append(int(value))
        abi.check(self._lib.rt_set_query_masks(self._ctx, masks[0], masks[1]), self._ctx)

    @staticmethod
    def _pack_masks(masks):
        """(n,) uint32, C-contiguous: the table rt_write_instance_masks takes.  None: the empty table.  Anything that is not a
        one-dimensional sequence of integers in [0, 2**32) raises ValueError."""
        if masks is None:
            return np.zeros(0, dtype=np.uint32)
        if isinstance(masks, (str, bytes)):
            raise ValueError("set_instance_masks: masks must be a sequence of integers")
        try:
            a = np.asarray(masks)
        except Exception:
            raise ValueError("set_instance_masks: masks must be a sequence of integers")
        if a.ndim != 1:
            raise ValueError("set_instance_masks: masks must be one-dimensional, one integer per instance")
        if a.size == 0:
            return np.zeros(0, dtype=np.uint32)
        if a.dtype == object:                   # Python integers too large for any fixed dtype, or a mixed sequence
            if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in a):
                raise ValueError("set_instance_masks: masks must be integers")
        elif a.dtype.kind not in "iu":
            raise ValueError("set_instance_masks: masks must be integers, not %s" % a.dtype)
        if any(int(v) < 0 or int(v) >= 2 ** 32 for v in a):
            raise ValueError("set_instance_masks: every mask must be in [0, 2**32)")
        return np.ascontiguousarray(np.array([int(v) for v in a], dtype=np.uint64).astype(np.uint32))

    @staticmethod
    def _pack_rays(origins, directions, tmin, tmax):
        """(n, 8) float32 rays {origin, tmin, dir, tmax}"""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("trace_rays: origins and directions must both be (n, 3)")
        rays = np.zeros((o.shape[0], 8), dtype=np.float32)
        rays[:, 0:3] = o
        rays[:, 4:7] = d
        for word, lim in ((3, tmin), (7, tmax)):
            lim = np.asarray(lim, dtype=np.float32)
            if lim.ndim > 1 or (lim.ndim == 1 and lim.shape[0] != o.shape[0]):
                raise ValueError("trace_rays: a limit is a scalar or an (n,) array")
            rays[:, word] = lim
        return rays

    @contextlib.contextmanager
    def _current_stream(self, device):
        """The stream handle with which a query runs on torch.cuda.current_stream(device).  torch's default stream has the handle
        0, which the C ABI reads as "the context's stream": the query then goes through a stream of our own, ordered after and
        before the default stream."""
        import torch
        cur = torch.cuda.current_stream(device)
        run = cur
        if cur.cuda_stream == 0:
            if getattr(self, "_query_stream", None) is None:
                self._query_stream = torch.cuda.Stream(device)
            run = self._query_stream
            run.wait_stream(cur)
        yield ctypes.c_void_p(run.cuda_stream)
        if run is not cur:
            cur.wait_stream(run)

    def _check_ray_tensor(self, name, rays, directions):
        import torch
        if directions is not None:
            raise ValueError("%s: a tensor argument is the (n, 8) ray buffer itself" % name)
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("%s: rays must be a contiguous float32 (n, 8) tensor" % name)
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise ValueError("%s: rays must live on cuda:%d, this renderer's device" % (name, self.device))

    def _parse_rect(self, name, rect):
        """rect = (x0, y0, w, h) or None, the whole frame -> (what the C ABI takes, w, h)"""
        if rect is None:
            return None, self.width, self.height
        x0, y0, w, h = (int(v) for v in rect)
        if min(x0, y0, w, h) < 0 or max(x0, y0, w, h) > 0xFFFFFFFF:
            raise ValueError("%s: rect is (x0, y0, w, h), four unsigned 32-bit numbers" % name)
        return (ctypes.c_uint32 * 4)(x0, y0, w, h), w, h

    def _check_plane_tensors(self, name, table, w, h, out):
        """out: a dict of (h, w) + tail tensors named and typed as `table` (abi.GBUFFER_PLANES, abi.AO_PLANES) says -> their device"""
        import torch
        if not isinstance(out, dict) or not out or any(n not in table for n in out):
            raise ValueError("%s: out is a dict of tensors named %s" % (name, ", ".join(table)))
        for n, t in out.items():
            tail, dtype, _ = table[n]
            want = {"<i4": torch.int32, "u1": torch.uint8, "<f4": torch.float32}[dtype]
            if type(t).__module__.split(".")[0] != "torch" or t.dtype != want or tuple(t.shape) != (h, w) + tail or not t.is_contiguous():
                raise ValueError("%s: out[%r] must be a contiguous %s tensor of shape %r" % (name, n, want, (h, w) + tail))
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s: out must live on cuda:%d, this renderer's device" % (name, self.device))
        return next(iter(out.values())).device

    def _trace_rays_torch(self, rays, directions, out, flags, occlusion):
        import torch
        name = "occluded" if occlusion else "trace_rays"
        self._check_ray_tensor(name, rays, directions)
        if occlusion:
            if out is None:
                out = torch.empty((rays.shape[0],), dtype=torch.uint8, device=rays.device)
            elif out.dtype != torch.uint8 or tuple(out.shape) != (rays.shape[0],) or not out.is_contiguous() or out.device != rays.device:
                raise ValueError("occluded: out must be a contiguous uint8 (n,) tensor on the rays' device")
        elif out is None:
            out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
        elif out.element_size() != 4 or tuple(out.shape) != (rays.shape[0], 8) or not out.is_contiguous() or out.device != rays.device:
            raise ValueError("trace_rays: out must be a contiguous 32-bit (n, 8) tensor on the rays' device")
        self.recalculateScene()
        args = (self._ctx, ctypes.c_void_p(rays.data_ptr()), rays.shape[0])
        with self._current_stream(rays.device) as stream:
            tail = (ctypes.c_void_p(out.data_ptr()), stream)
            if occlusion:
                abi.check(self._lib.rt_occluded(*args, flags, *tail), self._ctx)
            elif flags:
                abi.check(self._lib.rt_trace_rays_ex(*args, flags, *tail), self._ctx)
            else:
                abi.check(self._lib.rt_trace_rays(*args, *tail), self._ctx)
        return out

    # ---- closest-point queries: the nearest surface point to the host's points (rt_closest_points / rt_closest_points_host) -----
    def closest_points(self, points, radius=float("inf"), out=None):
        """The nearest point of the scene's surface to each point, within `radius`, against the scene the next frame would render
        (recalculateScene() first, as render() does).  Triangle scenes only; instances hidden from the nearest-hit ray mask
        (set_query_masks) are left out.

        numpy: points (n, 3), radius a scalar or an (n,) array -> dict of arrays dist2, dist (the square root of dist2, taken here
        on the host; -1 on a miss), u, v, prim, instance (n,), point (n, 3) and mesh (the instance's mesh index, -1 on a miss),
        through rt_closest_points_host.  A miss has dist2 = -1 and prim = instance = -1.
        torch: `points` is a float32 (n, 4) tensor {x, y, z, radius} on this renderer's device (`radius` must stay at its default)
        -> an (n, 8) float32 tensor of rt_closest records (prim / instance as int32 bits: .view(torch.int32)), or `out`, enqueued
        through rt_closest_points on torch.cuda.current_stream()."""
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            if not (isinstance(radius, float) and radius == float("inf")):
                raise ValueError("closest_points: with a tensor the radius is word 3 of each point")
            if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4 or not points.is_contiguous():
                raise ValueError("closest_points: points must be a contiguous float32 (n, 4) tensor")
            if points.device.type != "cuda" or points.device.index != self.device:
                raise ValueError("closest_points: points must live on cuda:%d, this renderer's device" % self.device)
            if out is None:
                out = torch.empty((points.shape[0], 8), dtype=torch.float32, device=points.device)
            elif out.element_size() != 4 or tuple(out.shape) != (points.shape[0], 8) or not out.is_contiguous() or out.device != points.device:
                raise ValueError("closest_points: out must be a contiguous 32-bit (n, 8) tensor on the points' device")
            self.recalculateScene()
            with self._current_stream(points.device) as stream:
                abi.check(self._lib.rt_closest_points(self._ctx, ctypes.c_void_p(points.data_ptr()), points.shape[0],
                                                      ctypes.c_void_p(out.data_ptr()), stream), self._ctx)
            return out
        if out is not None:
            raise ValueError("closest_points: out= is for (n, 4) tensors")
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        rad = np.asarray(radius, dtype=np.float32)
        if rad.ndim > 1 or (rad.ndim == 1 and rad.shape[0] != p.shape[0]):
            raise ValueError("closest_points: radius is a scalar or an (n,) array")
        pts = np.zeros((p.shape[0], 4), dtype=np.float32)
        pts[:, 0:3] = p
        pts[:, 3] = rad
        self.recalculateScene()
        rec = np.zeros(pts.shape[0], dtype=abi.CLOSEST_DTYPE)
        abi.check(self._lib.rt_closest_points_host(self._ctx, pts.ctypes.data, pts.shape[0], rec.ctypes.data), self._ctx)
        res = {"dist2": rec["dist2"].copy(), "u": rec["u"].copy(), "v": rec["v"].copy(), "prim": rec["prim"].copy(),
               "instance": rec["instance"].copy(), "point": np.ascontiguousarray(rec["point"])}
        with np.errstate(invalid="ignore"):
            root = np.sqrt(res["dist2"])
        res["dist"] = np.where(np.isnan(root), np.float32(-1.0), root).astype(np.float32)
        if self.scene.hasTriangles:
            mesh_index = np.asarray(self.scene.instances.mesh_index, dtype=np.int64)
            inst = res["instance"]
            res["mesh"] = np.where(inst >= 0, mesh_index[np.clip(inst, 0, len(mesh_index) - 1)], -1)
        return res

    # ---- multi-hit queries: the k nearest hits of the host's rays (rt_trace_rays_multi / rt_trace_rays_multi_host) -------------
    def trace_rays_multi(self, origins, directions=None, k=4, tmin=None, tmax=None, limits=False, out=None):
        """The first k surfaces each ray crosses (1 <= k <= abi.RT355_MAX_HITS), sorted by (t, instance, prim); the conventions
        are trace_rays'.

        numpy: origins and directions (n, 3), `tmin` / `tmax` scalars or (n,) arrays -> dict of arrays t, u, v, prim, instance
        (n, k) and normal (n, k, 3), unused places holding the miss record, plus `count` (n,), the number of hits of each ray.
        torch: a float32 (n, 8) tensor {origin, tmin, dir, tmax} on this renderer's device (`limits=True` reads words 3 and 7)
        -> an (n, k, 8) float32 tensor of rt_hit records, or `out`, enqueued on torch.cuda.current_stream()."""
        k = int(k)
        if type(origins).__module__.split(".")[0] == "torch":
            if tmin is not None or tmax is not None:
                raise ValueError("trace_rays_multi: with a tensor the limits are words 3 and 7 of the rays (limits=True)")
            return self._trace_rays_multi_torch(origins, directions, k, abi.RT_QUERY_LIMITS if limits else 0, out)
        if limits:
            raise ValueError("trace_rays_multi: limits=True is for (n, 8) tensors; numpy rays take tmin / tmax")
        if out is not None:
            raise ValueError("trace_rays_multi: out= is for (n, 8) tensors")
        flags = abi.RT_QUERY_LIMITS if (tmin is not None or tmax is not None) else 0
        rays = self._pack_rays(origins, directions, 0.001 if tmin is None else tmin, 9999.0 if tmax is None else tmax)
        self.recalculateScene()
        hits = np.zeros((rays.shape[0], max(k, 0)), dtype=abi.HIT_DTYPE)
        abi.check(self._lib.rt_trace_rays_multi_host(self._ctx, rays.ctypes.data, rays.shape[0], flags, k, hits.ctypes.data), self._ctx)
        res = self._hit_dict(hits)
        res["count"] = (hits["prim"] >= 0).sum(axis=1)
        return res

    def _trace_rays_multi_torch(self, rays, directions, k, flags, out):
        import torch
        self._check_ray_tensor("trace_rays_multi", rays, directions)
        if out is None:
            out = torch.empty((rays.shape[0], max(k, 0), 8), dtype=torch.float32, device=rays.device)
        elif out.element_size() != 4 or tuple(out.shape) != (rays.shape[0], k, 8) or not out.is_contiguous() or out.device != rays.device:
            raise ValueError("trace_rays_multi: out must be a contiguous 32-bit (n, k, 8) tensor on the rays' device")
        self.recalculateScene()
        with self._current_stream(rays.device) as stream:
            abi.check(self._lib.rt_trace_rays_multi(self._ctx, ctypes.c_void_p(rays.data_ptr()), rays.shape[0], flags, k,
                                                    ctypes.c_void_p(out.data_ptr()), stream), self._ctx)
        return out

    # ---- shaded ray queries: the renderer's colour along the host's rays (rt_shade_rays / rt_shade_rays_host) -----------------
    def shade_rays(self, origins, directions=None, compose=False, out=None):
        """What the renderer would show along each ray, against the scene, light, sky and maxBounces the next frame would use
        (recalculateScene() first, as render() does): {r, g, b, dist} = rayColor (RK:101-144), float32, not quantised; directions are
        used as given and dist is in units of their length.  compose=True (RT_SHADE_COMPOSE): r, g, b is pixelColor (RK:91-96), the
        fog towards the sky along the ray included -- a pixel's primary ray then gives that pixel of the next frame before its
        rgba8 store.

        numpy: origins and directions (n, 3) -> an (n, 4) float32 array, through rt_shade_rays_host.  torch: `origins` is a float32
        (n, 8) tensor {origin, -, dir, -} on this renderer's device and `directions` is None -> an (n, 4) float32 tensor, or `out`,
        enqueued through rt_shade_rays on torch.cuda.current_stream()."""
        flags = abi.RT_SHADE_COMPOSE if compose else 0
        if type(origins).__module__.split(".")[0] == "torch":
            return self._shade_rays_torch(origins, directions, out, flags)
        if out is not None:
            raise ValueError("shade_rays: out= is for (n, 8) tensors")
        rays = self._pack_rays(origins, directions, 0.0, 0.0)
        self.recalculateScene()
        res = np.zeros(rays.shape[0], dtype=abi.SHADE_DTYPE)
        abi.check(self._lib.rt_shade_rays_host(self._ctx, rays.ctypes.data, rays.shape[0], flags, res.ctypes.data), self._ctx)
        return res.view(np.float32).reshape(-1, 4)

    def _shade_rays_torch(self, rays, directions, out, flags):
        import torch
        self._check_ray_tensor("shade_rays", rays, directions)
        if out is None:
            out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (rays.shape[0], 4) or not out.is_contiguous() or out.device != rays.device:
            raise ValueError("shade_rays: out must be a contiguous float32 (n, 4) tensor on the rays' device")
        self.recalculateScene()
        with self._current_stream(rays.device) as stream:
            abi.check(self._lib.rt_shade_rays(self._ctx, ctypes.c_void_p(rays.data_ptr()), rays.shape[0], flags,
                                              ctypes.c_void_p(out.data_ptr()), stream), self._ctx)
        return out

    # ---- supersampled frames: s x s camera rays per pixel, resolved on the device (rt_render_samples / rt_render_samples_host) ----
    def render_samples(self, s=2, float_out=False, out=None):
        """The whole width x height frame the next render() would show (recalculateScene() first, as shade_rays does), anti-aliased:
        each pixel the float32 mean of pixelColor (RK:91-96) over s x s primary rays, 1 <= s <= abi.RT355_MAX_SUPERSAMPLE, added in
        the order sy outer, sx inner on the device; no sample reaches memory.  s = 1 is render()'s frame byte for byte.

        numpy (out=None): an (H, W, 4) uint8 frame, row 0 at the top, and with float_out a pair of it and the (H, W, 4) float32
        frame {r, g, b, 1} before the rgba8 store, through rt_render_samples_host.  torch: `out` is a contiguous uint8 (H, W, 4)
        tensor, a float32 (H, W, 4) tensor, or a pair of both on this renderer's device -> `out`, enqueued through
        rt_render_samples on torch.cuda.current_stream()."""
        s = int(s)
        if out is not None:
            return self._render_samples_torch(s, out)
        self.recalculateScene()
        img = np.zeros((self.height, self.width, 4), np.uint8)
        flt = np.zeros((self.height, self.width, 4), np.float32) if float_out else None
        abi.check(self._lib.rt_render_samples_host(self._ctx, s, img.ctypes.data, img.nbytes, flt.ctypes.data if float_out else None,
                                                   flt.nbytes if float_out else 0), self._ctx)
        return (img, flt) if float_out else img

    def _render_samples_torch(self, s, out):
        import torch
        tensors = list(out) if isinstance(out, (tuple, list)) else [out]
        img = flt = None
        for t in tensors:
            if type(t).__module__.split(".")[0] != "torch" or tuple(t.shape) != (self.height, self.width, 4) or not t.is_contiguous():
                raise ValueError("render_samples: out must be contiguous (H, W, 4) tensors")
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("render_samples: out must live on cuda:%d, this renderer's device" % self.device)
            if t.dtype == torch.uint8 and img is None:
                img = t
            elif t.dtype == torch.float32 and flt is None:
                flt = t
            else:
                raise ValueError("render_samples: out is one uint8 and / or one float32 tensor")
        if img is None and flt is None:
            raise ValueError("render_samples: out holds no tensor")
        self.recalculateScene()
        with self._current_stream((img if img is not None else flt).device) as stream:
            abi.check(self._lib.rt_render_samples(self._ctx, s, ctypes.c_void_p(img.data_ptr()) if img is not None else None,
                                                  img.numel() if img is not None else 0,
                                                  ctypes.c_void_p(flt.data_ptr()) if flt is not None else None,
                                                  4 * flt.numel() if flt is not None else 0, stream), self._ctx)
        return out

    # ---- geometry frames: depth, normal, ids and uv of what the camera sees, as planes (rt_render_gbuffer / rt_render_gbuffer_host) ----
    def render_gbuffer(self, rect=None, planes=("depth", "normal", "ids", "uv"), out=None):
        """pick() over a rectangle of the frame the next render() would show (recalculateScene() first), each field as a dense plane:
        `depth` (h, w) float32 = t (-1 on a miss), `normal` (h, w, 4) float32 {normal, 0}, `ids` (h, w, 2) int32 {prim, instance}
        (-1, -1 on a miss), `uv` (h, w, 2) float32.  rect = (x0, y0, w, h) in full-frame pixels, None: the whole frame.  The rays are
        made on the device and only the planes asked for are stored.

        numpy (out=None): a dict of the arrays named in `planes`, through rt_render_gbuffer_host.  torch: `out` is a dict of
        contiguous tensors of those shapes and dtypes on this renderer's device, any non-empty subset of the four names (`planes` is
        then not read) -> `out`, enqueued through rt_render_gbuffer on torch.cuda.current_stream()."""
        c_rect, w, h = self._parse_rect("render_gbuffer", rect)
        if out is not None:
            return self._render_gbuffer_torch(c_rect, w, h, out)
        names = [planes] if isinstance(planes, str) else list(planes)
        if not names or len(set(names)) != len(names) or any(n not in abi.GBUFFER_PLANES for n in names):
            raise ValueError("render_gbuffer: planes is a non-empty selection of %s" % ", ".join(abi.GBUFFER_PLANES))
        self.recalculateScene()
        res = {n: np.zeros((h, w) + abi.GBUFFER_PLANES[n][0], abi.GBUFFER_PLANES[n][1]) for n in names}
        gb = abi.RtGbuffer(**{n: (a.ctypes.data if a.size else None) for n, a in res.items()})
        abi.check(self._lib.rt_render_gbuffer_host(self._ctx, c_rect, ctypes.byref(gb), w * h), self._ctx)
        return res

    def _render_gbuffer_torch(self, c_rect, w, h, out):
        dev = self._check_plane_tensors("render_gbuffer", abi.GBUFFER_PLANES, w, h, out)
        self.recalculateScene()
        gb = abi.RtGbuffer(**{n: t.data_ptr() for n, t in out.items()})
        with self._current_stream(dev) as stream:
            abi.check(self._lib.rt_render_gbuffer(self._ctx, c_rect, ctypes.byref(gb), w * h, stream), self._ctx)
        return out

    # ---- ambient-occlusion frames: k occlusion rays per pixel over the hemisphere of what the camera sees (rt_render_ao / rt_render_ao_host) ----
    def render_ao(self, directions=None, k=16, radius=1.0, tmin=0.001, rect=None, planes=("ao",), out=None):
        """Per pixel of the frame the next render() would show (recalculateScene() first), or of rect = (x0, y0, w, h) of it: how many
        of k rays from the point pick() sees there are occluded() within (tmin, radius).  `directions` is (k, 3), 1 <= k <=
        abi.RT355_MAX_AO_RAYS, in the tangent space of the shading normal (z along it), used as given; None: ao_directions(k).
        `count` (h, w) uint8 is the number of occluded rays (0 on a miss), `ao` (h, w) float32 is (k - count) / k (1 on a miss).  The
        rays are made on the device: no plane, ray or per-ray answer passes through memory.

        numpy (out=None): a dict of the arrays named in `planes`, through rt_render_ao_host.  torch: `out` is a dict of contiguous
        tensors of those shapes and dtypes on this renderer's device, `count` (torch.uint8), `ao` (torch.float32) or both (`planes`
        is then not read) -> `out`, enqueued through rt_render_ao on torch.cuda.current_stream()."""
        dirs = ao_directions(k) if directions is None else np.ascontiguousarray(directions, dtype=np.float32)
        if dirs.ndim != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= abi.RT355_MAX_AO_RAYS:
            raise ValueError("render_ao: directions is (k, 3) with 1 <= k <= %d" % abi.RT355_MAX_AO_RAYS)
        c_rect, w, h = self._parse_rect("render_ao", rect)
        args = (self._ctx, c_rect, dirs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), dirs.shape[0], float(tmin), float(radius))
        if out is not None:
            return self._render_ao_torch(args, w, h, out)
        names = [planes] if isinstance(planes, str) else list(planes)
        if not names or len(set(names)) != len(names) or any(n not in abi.AO_PLANES for n in names):
            raise ValueError("render_ao: planes is a non-empty selection of %s" % ", ".join(abi.AO_PLANES))
        self.recalculateScene()
        res = {n: np.zeros((h, w), abi.AO_PLANES[n][1]) for n in names}
        ao = abi.RtAo(**{n: (a.ctypes.data if a.size else None) for n, a in res.items()})
        abi.check(self._lib.rt_render_ao_host(*args, ctypes.byref(ao), w * h), self._ctx)
        return res

    def _render_ao_torch(self, args, w, h, out):
        dev = self._check_plane_tensors("render_ao", abi.AO_PLANES, w, h, out)
        self.recalculateScene()
        ao = abi.RtAo(**{n: t.data_ptr() for n, t in out.items()})
        with self._current_stream(dev) as stream:
            abi.check(self._lib.rt_render_ao(*args, ctypes.byref(ao), w * h, stream), self._ctx)
        return out

    def pick(self, x, y):
        """What pixel (x, y) of the next frame sees first: its primary ray's nearest hit (full-frame coordinates, scalars or arrays
        that broadcast).  Triangle scenes add `mesh`, the instance's mesh index (-1 on a miss)."""
        xs, ys = np.broadcast_arrays(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64))
        shape = xs.shape
        xy = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
        xy = np.ascontiguousarray(np.where(xy < 0, 0xFFFFFFFF, xy).astype(np.uint32))   # negatives: outside the frame
        self.recalculateScene()
        hits = np.zeros(xy.shape[0], dtype=abi.HIT_DTYPE)
        abi.check(self._lib.rt_pick(self._ctx, xy.ctypes.data, xy.shape[0], hits.ctypes.data), self._ctx)
        res = self._hit_dict(hits)
        if self.scene.hasTriangles:
            mesh_index = np.asarray(self.scene.instances.mesh_index, dtype=np.int64)
            inst = res["instance"]
            res["mesh"] = np.where(inst >= 0, mesh_index[np.clip(inst, 0, len(mesh_index) - 1)], -1)
        return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}

    @staticmethod
    def _hit_dict(hits):
        return {"t": hits["t"].copy(), "u": hits["u"].copy(), "v": hits["v"].copy(), "prim": hits["prim"].copy(),
                "instance": hits["instance"].copy(), "normal": np.ascontiguousarray(hits["normal"])}

    def stats(self):
        st = abi.RtStats()
        abi.check(self._lib.rt_get_stats(self._ctx, ctypes.byref(st)), self._ctx)
        return {k: getattr(st, k) for k, _ in abi.RtStats._fields_}

    # ---- device-pointer interop for the process-per-GPU path --------------------------------
    def render_to(self, device_ptr, nbytes, stream_ptr=None):
        self.recalculateScene()
        abi.check(self._lib.rt_render_to(self._ctx, ctypes.c_void_p(device_ptr), nbytes,
                                         ctypes.c_void_p(stream_ptr) if stream_ptr else None), self._ctx)

    def assemble_frame(self, gathered_ptr, frame_ptr, world, stream_ptr=None):
        abi.check(self._lib.rt_assemble_frame(self._ctx, ctypes.c_void_p(gathered_ptr), ctypes.c_void_p(frame_ptr),
                                              world, ctypes.c_void_p(stream_ptr) if stream_ptr else None), self._ctx)

    # ---- multi-GPU behind the C ABI: render + RCCL gather + de-interleave in one call ---------------
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128 bytes every rank passes to comm_init (hand them over by any side channel)."""
        buf = ctypes.create_string_buffer(abi.RT355_COMM_ID_BYTES)
        abi.check(abi.load().rt_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """Collective over the group (ncclCommInitRank on this context's device); fixes the partition."""
        if len(unique_id) != abi.RT355_COMM_ID_BYTES:
            raise ValueError("comm_init: the unique id is %d bytes" % abi.RT355_COMM_ID_BYTES)
        buf = ctypes.create_string_buffer(bytes(unique_id), abi.RT355_COMM_ID_BYTES)
        abi.check(self._lib.rt_comm_init(self._ctx, buf, rank, world), self._ctx)
        self.rank, self.world = int(rank), int(world)

    def render_gather(self, root=0, wait=False):
        """RR:434-470 across the group: this rank's tiles, the RCCL exchange and the de-interleave are
        enqueued by ONE library call.  root = -1: every rank receives the frame."""
        self.recalculateScene()
        abi.check(self._lib.rt_render_gather(self._ctx, int(root)), self._ctx)
        if wait:
            abi.check(self._lib.rt_wait(self._ctx), self._ctx)

    def enqueue_gather(self, root=0):
        """render_gather() without recalculateScene and without the wait -- the counterpart of enqueue() for a group (bench.py
        times K frames of a scene that is resident before the timed region, with one rank or with many)."""
        abi.check(self._lib.rt_render_gather(self._ctx, int(root)), self._ctx)

    def read_frame(self):
        """The whole W x H frame of the latest render_gather (on a rank that received it)."""
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        abi.check(self._lib.rt_read_frame(self._ctx, out.ctypes.data, out.nbytes), self._ctx)
        return out

    def close(self):
        """Destroys the context.  The pinned frames of host_frames() stay valid for as long as an array refers to them."""
        if self._ctx is not None:
            self._lib.rt_destroy(self._ctx)      # waits for every copy that was begun
            self._ctx = None
            self._pinned = []                    # the renderer's own references; the memory goes with the last view

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
