"""Shared by the triangle edge-case tests (test infrastructure; tests/test_tri_edges_cpu.py, tests/test_tri_edges_gpu.py): small
hand-packed triangle scenes and constructed rays that drive the triangle path's float32 arithmetic to its edges -- box tests
that multiply 0 by inf, triangle tests exactly on their thresholds, magnitudes at which products go subnormal or overflow,
instance records that are not rigid (or not finite), geometry and node words that are not finite, texture coordinates at the
ends of the float-to-int conversion -- the comparison rule, and numpy counters that prove the inputs produce those cases.

THE COMPARISON RULE (stated here and nowhere else): float words are compared as bits, the sign of zero included, except that a
NaN matches any NaN whatever its sign and payload -- WGSL defines neither, and x86 and the GPU generate different default NaNs.
NaN positions must match exactly.  Nothing else is relaxed, and no ray or pixel is left out of a comparison."""
import functools
from types import SimpleNamespace

import numpy as np

import compute_raytracer_amd as rt
import query_common as qc
from helpers import tri_buffers
from query_common import F, bits, triangle_terms, u32f, walk_leaves

THRESH = F(0.00001)                                     # RK:359
T_MIN, T_MAX = F(0.001), F(9999.0)                      # RK:315, RK:172
TINY = F(2.0 ** -126)                                   # the smallest normal float32


class Comparator:
    """differ(a, b): the rule above, elementwise; nan_matches counts the NaN-against-NaN words it let pass."""
    def __init__(self):
        self.nan_matches = 0

    def differ(self, a, b):
        a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
        both = np.isnan(a) & np.isnan(b)
        self.nan_matches += int(both.sum())
        return (bits(a) != bits(b)) & ~both

    def same(self, a, b):
        return np.shape(a) == np.shape(b) and not self.differ(a, b).any()


def ulps(x, k):
    """float32 x moved k representable values up (k < 0: down)"""
    x = np.asarray(x, F)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def tri(a, b, c, colour, normal=None, uv=None):
    """One 40-float record (RR:198-209): corners a, b, c with their normals (the face's unless given) and uvs, and the colour."""
    a, b, c = (np.asarray(p, np.float64) for p in (a, b, c))
    n = np.cross(b - a, c - a) if normal is None else None
    t = np.zeros(40, F)
    for k, p in enumerate((a, b, c)):
        t[12 * k:12 * k + 3] = p
        nk = n / (np.linalg.norm(n) or 1.0) if normal is None else np.asarray(normal[k], np.float64)
        t[12 * k + 4:12 * k + 7] = nk
        t[12 * k + 8:12 * k + 10] = (((p[0] + 3.0) / 3.0 - 0.5, (p[1] + 3.0) / 3.0 - 0.5) if uv is None else uv[k])
    t[36:40] = colour
    return t


def colour_of(i):
    return [0.2 + 0.8 * ((i * 5) % 7) / 7.0, 0.3 + 0.7 * ((i * 3) % 5) / 5.0, 0.9 - 0.6 * (i % 4) / 4.0, (1.0, 0.5, 1.0, 0.0)[i % 4]]


def quad(p0, p1, p2, p3, i, **kw):
    return [tri(p0, p1, p2, colour_of(i), **kw), tri(p0, p2, p3, colour_of(i + 1), **kw)]


def base_mesh(zero_normals=False, uv_values=None):
    """-> (triangles (T, 40), leaves: lists of triangle indices).  All coordinates are dyadic.
    A 6 x 6 grid of unit cells in the plane z = 0 facing +z (two triangles per cell and leaf; vertex normals lean outwards); a floor
    quad (flat in y) and a wall quad (flat in x); a triangle twice in one leaf and another twice in two leaves (exact t ties);
    one triangle three times one ulp apart in z; a quad facing -z (a back face from the front); a quad of size 2^-6.
    zero_normals: some cells get vertex normals that cancel (along a line, or everywhere).  uv_values: cell k's corners all
    carry uv = (uv_values[k % n], uv_values[(k // n) % n]) instead of the position's."""
    tris, leaves = [], []
    def leaf(ts):
        leaves.append(list(range(len(tris), len(tris) + len(ts))))
        tris.extend(ts)
    cell = 0
    for y in range(-3, 3):
        for x in range(-3, 3):
            p = [(x, y, 0), (x + 1, y, 0), (x + 1, y + 1, 0), (x, y + 1, 0)]
            nrm = [np.array([0.125 * q[0], 0.125 * q[1], 1.0]) for q in p]
            if zero_normals and cell % 5 == 1:
                nrm = [np.array([0, 0, 1.0]), np.array([0, 0, -1.0]), np.zeros(3), np.array([0, 0, 1.0])]
            if zero_normals and cell % 5 == 3:
                nrm = [np.zeros(3)] * 4
            uv = None
            if uv_values is not None:
                n = len(uv_values)
                uv = [(uv_values[cell % n], uv_values[(cell // n + cell) % n])] * 4
            pick = lambda idx, src: None if src is None else [src[i] for i in idx]
            leaf([tri(p[0], p[1], p[2], colour_of(cell), pick((0, 1, 2), nrm), pick((0, 1, 2), uv)),
                  tri(p[0], p[2], p[3], colour_of(cell + 1), pick((0, 2, 3), nrm), pick((0, 2, 3), uv))])
            cell += 1
    leaf(quad((-4, -3, 6), (4, -3, 6), (4, -3, -2), (-4, -3, -2), 2))                    # floor, facing +y
    leaf(quad((-4, -3, 6), (-4, -3, -2), (-4, 3, -2), (-4, 3, 6), 5))                    # wall, facing +x
    d1 = [(1.5, 1.5, 1), (2.5, 1.5, 1), (2.5, 2.5, 1)]
    leaf([tri(*d1, colour_of(8)), tri(*d1, colour_of(9))])                               # a tie inside one leaf
    d2 = [(-2.5, 1.5, 1), (-1.5, 1.5, 1), (-1.5, 2.5, 1)]
    leaf([tri(*d2, colour_of(10))]); leaf([tri(*d2, colour_of(11))])                     # a tie across two leaves
    for k, dz in enumerate((0.0, 2.0 ** -23, -2.0 ** -24)):                              # one ulp behind, one ulp in front
        leaf([tri((-0.5, 1.5, 1 + dz), (0.5, 1.5, 1 + dz), (0.5, 2.5, 1 + dz), colour_of(12 + k))])
    leaf(quad((-2.5, -2.5, 2), (-2.5, -1.5, 2), (-1.5, -1.5, 2), (-1.5, -2.5, 2), 16))   # facing -z
    s = 2.0 ** -6
    leaf(quad((2, -2, 0.5), (2 + s, -2, 0.5), (2 + s, -2 + s, 0.5), (2, -2 + s, 0.5), 19))
    return np.array(tris, F), leaves


def build_tree(tris, leaves):
    """A binary tree over `leaves` (median split of the leaves' centres along their widest axis), children side by side, every
    box the exact float32 min / max of the corners below it (np.fmin / np.fmax: a NaN corner is skipped).
    -> (nodes (N, 8) with indices relative to this tree and this mesh's lookup run, lookup order)."""
    corners = np.stack([tris[:, 0:3], tris[:, 12:15], tris[:, 24:27]], axis=1)
    nodes, order = [None], []
    def centre(g):
        with np.errstate(all="ignore"):
            c = np.nan_to_num(corners[g].reshape(-1, 3).astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        return c.mean(axis=0)
    def fill(i, gs):
        pts = corners[[t for g in gs for t in g]].reshape(-1, 3)
        pts = np.where(np.isfinite(pts), pts, np.nan)
        lo, hi = np.fmin.reduce(pts, axis=0), np.fmax.reduce(pts, axis=0)
        lo, hi = np.nan_to_num(lo, nan=0.0), np.nan_to_num(hi, nan=0.0)
        if len(gs) == 1:
            nodes[i] = np.array([*lo, len(order), *hi, len(gs[0])], F)
            order.extend(gs[0])
            return
        cs = np.array([centre(g) for g in gs])
        axis = int(np.argmax(cs.max(axis=0) - cs.min(axis=0)))
        srt = np.argsort(cs[:, axis], kind="stable")
        left = len(nodes)
        nodes.extend([None, None])
        nodes[i] = np.array([*lo, left, *hi, 0], F)
        fill(left, [gs[k] for k in srt[:len(gs) // 2]])
        fill(left + 1, [gs[k] for k in srt[len(gs) // 2:]])
    fill(0, leaves)
    return np.array(nodes, F), np.array(order, np.int64)


WIDE = 1.0e4                                            # helpers.deepen_top_level's boxes: where geometry is not finite


def assemble(tris, leaves, inverse, world=None, camera=(0.5, 1.0, 6.0), eulers=(270.0, 100.0), light=(0.0, 5.0, 4.0), pad=0.0, full=False):
    """A scene of one mesh and len(inverse) instances of it.  inverse: (M, 16) the records' inverse model matrices (column-major),
    written as given.  world: per instance the forward matrix (4, 4) float64 whose image of the mesh bounds its top-level box
    (grown by `pad` times its size), or None for the wide box.  The top-level tree is a chain: node 0 = {leaf of instance 0,
    the rest}, and so on -- 2 M - 1 nodes, every inner box the union of what is below it.  full: zero nodes behind the tree up to the 2 T - 1 any tree
    of the mesh can need, and the mesh described as RendererRaytracing.rebuild() reads it."""
    inverse = np.asarray(inverse, F).reshape(-1, 16)
    m = inverse.shape[0]
    base = 2 * m - 1
    nodes, order = build_tree(tris, leaves)
    inner = nodes[:, 7] == 0
    nodes[inner, 3] += base
    if full:
        nodes = np.concatenate([nodes, np.zeros((max(2 * tris.shape[0] - 1 - nodes.shape[0], 0), 8), F)])
    corners = np.stack([tris[:, 0:3], tris[:, 12:15], tris[:, 24:27]], axis=1).reshape(-1, 3).astype(np.float64)
    corners = corners[np.isfinite(corners).all(axis=1)]
    lo_w, hi_w = np.zeros((m, 3)), np.zeros((m, 3))
    for k in range(m):
        if world is None or world[k] is None:
            lo_w[k], hi_w[k] = -WIDE, WIDE
            continue
        p = corners @ np.asarray(world[k], np.float64)[:3, :3].T + np.asarray(world[k], np.float64)[:3, 3]
        lo, hi = p.min(axis=0), p.max(axis=0)
        grow = pad * (hi - lo).max()
        lo_w[k] = np.nextafter((lo - grow).astype(F), F(-np.inf)) if pad else lo
        hi_w[k] = np.nextafter((hi + grow).astype(F), F(np.inf)) if pad else hi
    d = dict(triangles=tris, blas_nodes=nodes, tri_lookup=order.astype(F), mesh_root=np.array([base]),
             mesh_box_lo=nodes[0:1, 0:3].astype(np.float64), mesh_box_hi=nodes[0:1, 4:7].astype(np.float64),
             inst_mesh=np.zeros(m, np.int64), inst_position=np.zeros((m, 3)), inst_eulers=np.zeros((m, 3)), inst_speed=np.zeros((m, 3)),
             camera_position=np.asarray(camera, np.float64), camera_eulers=np.asarray(eulers, F),
             light=np.array(list(light) + [3.0, 0.3]))
    with np.errstate(all="ignore"):                    # (the placeholder top-level tree of from_packed is replaced below)
        scene = rt.SceneRaytracing.from_packed(d)
    scene.meshes[0].lookup_offset = 0
    scene.meshes[0].soup = SimpleNamespace(count=tris.shape[0])
    scene.frame["blas"][:, 0:16] = inverse
    scene.frame["blas_lookup"] = np.arange(m, dtype=F)
    t = np.zeros((base, 8), F)
    for k in range(m):                                   # leaf of instance k at 2k + 1 (the last one at 2k), the chain at 2k
        leaf = 2 * k + 1 if k < m - 1 else 2 * k
        t[leaf] = [*lo_w[k], k, *hi_w[k], 1]
        if k < m - 1:
            t[2 * k] = [*lo_w[k:].min(axis=0), 2 * k + 1, *hi_w[k:].max(axis=0), 0]
    scene.frame["tlas_nodes"] = t
    scene.tlasNodesUsed = base
    return scene


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def record(inv44):
    """(4, 4) float64 inverse model matrix -> the 16 column-major words"""
    return np.asarray(inv44, np.float64).T.reshape(16).astype(F)


def material(width):
    return rt.Material(np.random.default_rng(24 + width).integers(0, 256, (16, width, 4), dtype=np.uint8))


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def lattice(x0, x1, y0, y1, step, z, dz):
    xs, ys = np.meshgrid(np.arange(x0, x1 + step / 2, step), np.arange(y0, y1 + step / 2, step))
    o = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, z)], axis=1).astype(F)
    d = np.tile(np.array([0.0, 0.0, dz], F), (o.shape[0], 1))
    return o, d


def threshold_rays():
    """The rays of the threshold class, in the base mesh's space (see the module's test for what each group reaches)."""
    sets = [lattice(-3, 3, -3, 3, 0.25, 4.0, -1.0), lattice(-3, 3, -3, 3, 0.25, 4.0, -2.0), lattice(-3, 3, -3, 3, 0.25, -4.0, 1.0),
            lattice(1.5, 2.5, 1.5, 2.5, 0.125, 4.0, -1.0), lattice(-2.5, -1.5, 1.5, 2.5, 0.125, 4.0, -1.0),       # the ties
            lattice(-0.5, 0.5, 1.5, 2.5, 0.125, 1.5, -1.0)]                                                       # one ulp apart
    cells = [(x + 0.25, y + 0.5) for y in range(-3, 3) for x in range(-3, 3)][:30]
    for k in range(-4, 5):
        L = float(ulps(THRESH, k))                      # det = L on the unit cells
        o = np.array([(x, y, 2.0 ** -7) for x, y in cells], F)
        sets.append((o, np.tile(np.array([0, 0, -L], F), (len(cells), 1))))
        g = float(ulps(THRESH, k))                      # grazing: d = (1, 0, -g), det = g, the hit at t = 1
        o = np.array([(x - 1.0, y, g) for x, y in cells], F)
        sets.append((o, np.tile(np.array([1, 0, -g], F), (len(cells), 1))))
        Lm = float(ulps(THRESH, k)) * 2.0 ** 12         # the small quad: det = Lm * 2^-12
        s = 2.0 ** -6
        o = np.array([(2 + s * a, -2 + s * b, 0.5 + 2.0 ** -7) for a in (0.25, 0.5, 0.75) for b in (0.125, 0.25, 0.5, 0.75)], F)
        sets.append((o, np.tile(np.array([0, 0, -Lm], F), (o.shape[0], 1))))
        z0 = float(ulps(T_MIN, k))                      # t = z0 exactly
        o = np.array([(x, y, z0) for x, y in cells], F)
        sets.append((o, np.tile(np.array([0, 0, -1], F), (len(cells), 1))))
    o, d = lattice(-3, 3, -3, 3, 0.25, 4.0, -1.0)       # tilted: through the same lattice points at t = 4, in no box's face plane
    sets.append((o - F([1.0, 2.0, 0.0]), np.tile(np.array([0.25, 0.5, -1.0], F), (o.shape[0], 1))))
    # subnormal offsets from the vertex at the origin: u = o.x - o.y and v = o.y are subnormal where the hit is accepted; tilted,
    # the slab products of the boxes with a face at 0 are
    near = np.array([(a * 2.0 ** -140, b * 2.0 ** -141, z) for a in range(1, 9) for b in range(8) for z in (4.0, 2.0)], F)
    sets.append((near, np.tile(np.array([0, 0, -1.0], F), (near.shape[0], 1))))
    sets.append((near, np.tile(np.array([0.25, 0.5, -1.0], F), (near.shape[0], 1))))
    sets.append(lattice(-0.5, 0.5, 1.5, 2.5, 0.125, 3.0, -1.0))       # the three one ulp apart again: t = 2 and the value below it
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


def box_rays(buf, seed=3):
    """For every box of the node buffer: origins exactly on each of its six face planes with a zero direction component (+0 and
    -0) on that axis, rays in the plane of a face along an axis, rays from the eight corners, rays from inside."""
    rng = np.random.default_rng(seed)
    nodes = np.asarray(buf["nodes"], F).reshape(-1, 8)
    o, d = [], []
    for i in range(nodes.shape[0]):
        lo, hi = nodes[i, 0:3].astype(np.float64), nodes[i, 4:7].astype(np.float64)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo == 0).all() and (hi == 0).all():
            continue
        ext = np.maximum(hi - lo, 1.0)
        for axis in range(3):
            for face in (lo, hi):
                for zero in (0.0, -0.0):
                    p = lo + np.round(rng.uniform(0, 1, 3) * 8) / 8 * (hi - lo)
                    p[axis] = face[axis]
                    v = np.round(rng.uniform(-2, 2, 3) * 4) / 4
                    v[v == 0] = 0.5
                    if (i + axis) % 3 == 0:             # along one axis only: two infinite inverse components
                        v[(axis + 1) % 3] = 0.0
                    v[axis] = zero
                    back = 0.5 if (i % 2) else 0.0      # half of them start on the box, half before it
                    o.append(p - back * v * np.array([1.0 if a != axis else 0.0 for a in range(3)])); d.append(v)
        if i % 4 == 0:
            for c in range(8):
                p = np.array([hi[a] if (c >> a) & 1 else lo[a] for a in range(3)])
                o.append(p); d.append((lo + hi) / 2 - p + 0.0)
                o.append(p); d.append(np.array([0.0, 0.0, -1.0]) * ext[2])
            for _ in range(3):
                o.append(lo + rng.uniform(0, 1, 3) * (hi - lo)); d.append(rng.normal(size=3))
    return np.array(o, F), np.array(d, F)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """name; scene and mat; buf = tri_buffers(scene, mat); o, d: the constructed rays; honest: every box bounds what is below it
    and the geometry is finite (the brute force is then a reference); mirrored: the instance records with negative determinant."""
    def __init__(self, name, scene, mat, rays, honest=True, mirrored=()):
        self.name, self.scene, self.mat, self.honest, self.mirrored = name, scene, mat, honest, tuple(mirrored)
        self.buf = tri_buffers(scene, mat)
        self.o, self.d = (np.ascontiguousarray(a, F) for a in rays)
        assert self.o.shape[0] <= 4000 and scene.static["triangles"].shape[0] <= 200

    def state(self, bounces, sky):
        return {"tri": self.buf, "params": self.scene.pack_params(bounces), "faces": sky.faces}


def _two_instances(tris, leaves, shift=8.0, **kw):
    """the identity and an exact shift along x"""
    inv = [record(np.eye(4)), record(translation(-shift, 0, 0))]
    return assemble(tris, leaves, inv, world=[np.eye(4), translation(shift, 0, 0)], **kw)


def case_boxes():
    tris, leaves = base_mesh()
    scene = _two_instances(tris, leaves)
    buf = tri_buffers(scene, material(24))
    o, d = box_rays(buf)
    o2 = o[::5] + F([8, 0, 0])                           # the same rays at the second instance (an exact shift)
    return Case("boxes", scene, material(24), (np.concatenate([o, o2]), np.concatenate([d, d[::5]])))


def case_thresholds():
    tris, leaves = base_mesh()
    return Case("thresholds", _two_instances(tris, leaves), material(24), threshold_rays())


LENGTHS = (-40, -12, -8, -4, 0, 4, 8, 12, 40)           # direction lengths 2^j on top of the scene's own scale


def case_scaled(k, full=False):
    """The threshold scene times 2^k, camera, light and rays included; ray i's direction is longer by 2^LENGTHS[i % 9] again."""
    s = 2.0 ** k
    tris, leaves = base_mesh()
    for c in (slice(0, 3), slice(12, 15), slice(24, 27)):
        tris[:, c] *= F(s)
    inv = [record(np.eye(4)), record(translation(-8 * s, 0, 0))]
    scene = assemble(tris, leaves, inv, world=[np.eye(4), translation(8 * s, 0, 0)], camera=(0.5 * s, 1.0 * s, 6.0 * s),
                     light=(0.0, 5.0 * s, 4.0 * s), full=full)
    o, d = threshold_rays()
    o, d = o[::2], d[::2]
    j = np.array(LENGTHS)[np.arange(o.shape[0]) % len(LENGTHS)]
    with np.errstate(all="ignore"):
        return Case("scale%+d" % k, scene, material(24), ((o * F(s)).astype(F), (d * F(s) * (2.0 ** j)[:, None].astype(F)).astype(F)))


def case_far(k, full=False):
    """The threshold scene 2^k away from the origin along (1, -1, 1): integer coordinates stay exact, finer ones round."""
    off = np.array([2.0 ** k, -(2.0 ** k), 2.0 ** k])
    tris, leaves = base_mesh()
    for c in (slice(0, 3), slice(12, 15), slice(24, 27)):
        tris[:, c] = (tris[:, c].astype(np.float64) + off).astype(F)
    scene = _two_instances(tris, leaves, camera=tuple(np.array([0.5, 1.0, 6.0]) + off), light=tuple(np.array([0.0, 5.0, 4.0]) + off), full=full)
    o, d = threshold_rays()
    return Case("far%d" % k, scene, material(24), ((o[::2].astype(np.float64) + off).astype(F), d[::2]))


def case_matrices():
    """Ten instances of the base mesh (with cancelling vertex normals), spread along x -- more than the four the other cases keep
    to, because every kind of record is one instance and the kinds must meet in one scene (one top-level walk, one frame).  Forward
    matrices: identity (the record's row 3 non-zero), scale (2^12, 1, 2^-12), scale (2^-12, 2^12, 1), shear, mirror in x; records
    with no forward matrix: rank 2 (object z constant), rank 0 (object point constant), a NaN entry among the normal's terms, an
    inf entry in row 3, a NaN entry among the geometry's terms."""
    tris, leaves = base_mesh(zero_normals=True)
    fwd = [np.eye(4), np.diag([2.0 ** 12, 1.0, 2.0 ** -12, 1.0]), np.diag([2.0 ** -12, 2.0 ** 12, 1.0, 1.0]),
           np.array([[1, 0.5, 0, 0], [0, 1, 0.25, 0], [0.125, 0, 1, 0], [0, 0, 0, 1.0]]), np.diag([-1.0, 1.0, 1.0, 1.0])]
    fwd = [translation(12.0 * k, 0, 0) @ m for k, m in enumerate(fwd)]
    inv = [record(np.linalg.inv(m)) for m in fwd]
    inv[0][[3, 7, 11]] = (0.5, -2.0, 3.0)
    r2 = np.eye(4); r2[2, :] = (0, 0, 0, 0.5); r2[0, 3] = 2.0
    r0 = np.zeros((4, 4)); r0[:, 3] = (0.25, 0.25, 0.5, 1.0)
    nan_rec = record(translation(-60.0, 0, 0)); nan_rec[7] = np.nan
    inf_rec = record(translation(-72.0, 0, 0)); inf_rec[3] = np.inf; inf_rec[15] = 2.0
    nan_geo = record(translation(-84.0, 0, 0)); nan_geo[0] = np.nan
    inv += [record(r2), record(r0), nan_rec, inf_rec, nan_geo]
    world = fwd + [None, None, translation(60.0, 0, 0), translation(72.0, 0, 0), None]
    scene = assemble(tris, leaves, inv, world=world, pad=2.0 ** -10)
    o, d = threshold_rays()
    o, d = o[:1875:6].astype(np.float64), d[:1875:6].astype(np.float64)          # the three lattices, thinned
    os_, ds_ = [], []
    for k, m in enumerate(world):
        m = np.eye(4) if m is None else m
        os_.append(o @ m[:3, :3].T + m[:3, 3]); ds_.append(d @ m[:3, :3].T)
    rng = np.random.default_rng(11)                      # and rays across all of them
    os_.append(rng.uniform([-6, -3, -2], [100, 4, 7], (400, 3))); ds_.append(rng.normal(size=(400, 3)))
    return Case("matrices", scene, material(24), (np.concatenate(os_), np.concatenate(ds_)), mirrored=(4,))


def case_mixed():
    """For the split-tile forms: the base mesh (flat boxes, threshold geometry, cancelling normals) under seven records with honest
    top-level boxes -- identity with row 3 in use, scales (8, 1, 1/8) and (1/8, 8, 1), shear, mirror, a NaN among the normal's
    terms, an inf in row 3 -- seen from far enough that most tiles are sky and a few are expensive."""
    tris, leaves = base_mesh(zero_normals=True)
    fwd = [np.eye(4), np.diag([8.0, 1.0, 0.125, 1.0]), np.diag([0.125, 8.0, 1.0, 1.0]),
           np.array([[1, 0.5, 0, 0], [0, 1, 0.25, 0], [0.125, 0, 1, 0], [0, 0, 0, 1.0]]), np.diag([-1.0, 1.0, 1.0, 1.0]), np.eye(4), np.eye(4)]
    place = [(0, 0, 0), (0, 9, -6), (14, 4, 0), (-12, 0, 0), (12, -8, 0), (-12, 9, 2), (0, -9, 3)]
    fwd = [translation(*p) @ m for p, m in zip(place, fwd)]
    inv = [record(np.linalg.inv(m)) for m in fwd]
    inv[0][[3, 7, 11]] = (0.5, -2.0, 3.0)
    inv[5][7] = np.nan
    inv[6][3] = np.inf
    scene = assemble(tris, leaves, inv, world=fwd, pad=2.0 ** -10, camera=(0.5, 1.0, 40.0), eulers=(270.0, 92.0), light=(0.0, 5.0, 8.0))
    o, d = threshold_rays()
    return Case("mixed", scene, material(24), (o[:1875:3], d[:1875:3]), mirrored=(4,))


def case_degenerate():
    """The base mesh with a bad triangle added to leaves of the grid -- three equal corners, collinear corners, a NaN, +inf, -inf
    or +-3e38 corner -- then boxes with a NaN, inverted boxes, and count / left words that are NaN, negative, fractional or
    beyond 2^32.  Inner nodes keep their child index, so the buffer stays a tree (the walk ends).  Wide top-level boxes."""
    tris, leaves = base_mesh()
    tris = list(tris)
    bad = [[(0.5, 0.5, 0.25)] * 3, [(0, 0, 0.25), (1, 1, 0.25), (2, 2, 0.25)], [(np.nan, 0, 0), (1, 0, 0), (1, 1, 0)],
           [(0, 0, 0), (np.inf, 0, 0), (1, 1, 0)], [(0, 0, 0), (1, 0, 0), (1, -np.inf, 0)], [(3e38, 0, 0), (-3e38, 1, 0), (0, 3e38, 0)],
           [(0, 0, 0.5), (1, 0, 0.5), (1, 1, np.nan)], [(-3e38, -3e38, 1), (3e38, -3e38, 1), (0, 3e38, 1)]]
    with np.errstate(all="ignore"):
        for k, c in enumerate(bad):
            leaves[3 * k + 1].append(len(tris))
            tris.append(tri(*c, colour_of(k), normal=[(0, 0, 1.0)] * 3))
    tris = np.array(tris, F)
    inv = [record(np.eye(4)), record(translation(-8.0, 0, 0))]
    scene = assemble(tris, leaves, inv, world=[None, None])
    nodes = scene.static["blas_nodes"]
    leaf = np.nonzero(nodes[:, 7] > 0)[0]
    inner = np.nonzero(nodes[:, 7] == 0)[0][1:]
    nodes[leaf[2], 0] = np.nan                                                    # boxes
    nodes[leaf[5], [0, 1, 2, 4, 5, 6]] = nodes[leaf[5], [4, 5, 6, 0, 1, 2]] + F([0.5, 0.5, 0.5, -0.5, -0.5, -0.5])
    nodes[inner[3], 0:3] = np.nan; nodes[inner[3], 4:7] = np.nan
    nodes[inner[6], 4] = nodes[inner[6], 0] - F(1.0)
    nodes[inner[1], 7] = np.nan; nodes[inner[4], 7] = -3.0; nodes[inner[7], 7] = -0.0   # counts that u32() takes to 0
    nodes[leaf[8], 7] += F(0.75); nodes[leaf[11], 7] += F(0.5)                     # ... and that it truncates
    nodes[leaf[14], 3] += F(0.5)                                                   # slots: truncated, NaN and negative (0), beyond
    nodes[leaf[17], 3] = np.nan; nodes[leaf[20], 3] = -5.0                         # 2^32 (the last slot)
    nodes[leaf[23], 3] = 2.0 ** 32; nodes[leaf[26], 3] = 2.0 ** 33
    o, d = threshold_rays()
    rng = np.random.default_rng(13)
    o2, d2 = rng.uniform([-5, -4, -3], [13, 4, 7], (600, 3)), rng.normal(size=(600, 3))
    clean = tri_buffers(_two_instances(*base_mesh()), material(24))
    o3, d3 = box_rays(clean)
    return Case("degenerate", scene, material(24), (np.concatenate([o[:1875:2], o2, o3[::3]]), np.concatenate([d[:1875:2], d2, d3[::3]])),
                honest=False)


UV_VALUES = [0.0, 1.0, -1.0, float(ulps(1.0, -1)), float(ulps(1.0, 1)), float(ulps(2.0, -1)), 2.0 ** -24, -(2.0 ** -24), -0.75, 1.5,
             3.25, -2.5, 1e30, -1e30, 3e9, -3e9, np.inf, -np.inf, np.nan]


def case_uv(width):
    tris, leaves = base_mesh(uv_values=UV_VALUES)
    o, d = threshold_rays()
    return Case("uv%d" % width, _two_instances(tris, leaves), material(width), (o[:1875], d[:1875]))


CASES = {"boxes": case_boxes, "thresholds": case_thresholds, "matrices": case_matrices, "degenerate": case_degenerate,
         "uv24": lambda: case_uv(24), "uv16": lambda: case_uv(16)}
CASES.update({"scale%+d" % k: (lambda k=k: case_scaled(k)) for k in (-60, -40, -20, 20, 40, 60)})
CASES.update({"far%d" % k: (lambda k=k: case_far(k)) for k in (20, 23)})
HAZARD_CLASS = {"boxes": 1, "thresholds": 2, "matrices": 4, "degenerate": 5, "uv24": 6, "uv16": 6}
HAZARD_CLASS.update({n: 3 for n in CASES if n.startswith(("scale", "far"))})


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once per process; nothing changes it (a test that refits or rebuilds builds its own: CASES[name]())."""
    return (CASES.get(name) or {"mixed": case_mixed}[name])()


# ---- the counters: what the inputs reach, in numpy float32 ------------------------------------------------------------------------
def subnormal(x):
    with np.errstate(all="ignore"):
        return (x != 0) & (np.abs(x) < TINY)


def nearest_hits(c, o=None, d=None):
    """pick-style nearest hits of rays (the case's constructed ones unless given) by the box-aware brute force: t, instance,
    prim (-1: none)"""
    o, d = (c.o, c.d) if o is None else (o, d)
    with np.errstate(all="ignore"):
        T, I, P, _ = qc.k_smallest(o.shape[0], 1, qc.all_triangle_hits(c.buf, o, d, boxes=True), T_MIN, T_MAX)
    return T[:, 0], I[:, 0], P[:, 0]


def limits_about(t):
    """The limits the device tests put about a nearest t (-1: a miss): ray i gets the value one below (i % 3 == 0), at (1) or one
    above (2) its t; -> (step (n,) in {-1, 0, 1}, that value (n,))"""
    t = np.asarray(t, F)
    step = np.arange(t.shape[0]) % 3 - 1
    with np.errstate(all="ignore"):
        about = np.where(step < 0, np.nextafter(t, F(0.0)), np.where(step > 0, np.nextafter(t, F(np.inf)), t)).astype(F)
    return step, about


def nearest_by_walk(buf, o, d):
    """One ray through the reference's two-level walk (RK:168-332), restated step by step in float32 with the oracle's clamps:
    -> (t or -1, instance, prim).  The order of the box and triangle tests decides which of two hits at one t is kept."""
    nodes = np.asarray(buf["nodes"], F).reshape(-1, 8)
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    look, blook = np.asarray(buf["tri_lookup"], F), np.asarray(buf["blas_lookup"], F)
    last = nodes.shape[0] - 1
    o, d = np.asarray(o, F).reshape(1, 3), np.asarray(d, F).reshape(1, 3)
    best = [T_MAX, -1, -1]

    def walk(root, oo, od, leaf, test_root=False):
        with np.errstate(all="ignore"):
            inv = F(1.0) / od
        node, stack = min(root, last), []
        while True:
            left, count = u32f(nodes[node, 3]), u32f(nodes[node, 7])
            if count == 0:
                c1, c2 = min(left, last), min((left + 1) & 0xFFFFFFFF, last)
                with np.errstate(all="ignore"):
                    d1 = qc.hit_aabb(nodes[c1, 0:3], nodes[c1, 4:7], oo, inv)[0]
                    d2 = qc.hit_aabb(nodes[c2, 0:3], nodes[c2, 4:7], oo, inv)[0]
                if d1 > d2:
                    d1, d2, c1, c2 = d2, d1, c2, c1
                if d1 > best[0]:
                    if not stack:
                        return
                    node = stack.pop()
                else:
                    node = c1
                    if d2 < best[0] and len(stack) < 20:
                        stack.append(c2)
            else:
                for i in range(count):
                    leaf(left + i)
                if not stack:
                    return
                node = stack.pop()

    def instance(slot):
        bi = min(u32f(blook[min(slot, len(blook) - 1)]), blas.shape[0] - 1)
        m = blas[bi][None]
        with np.errstate(all="ignore"):
            oo, od = qc.mat_apply(m, o, 1.0), qc.mat_apply(m, d, 0.0)
        def triangle(s):
            prim = min(u32f(look[min(s, len(look) - 1)]), tris.shape[0] - 1)
            with np.errstate(all="ignore"):
                q = triangle_terms(blas[bi], tris[prim:prim + 1], o, d)
            t = q["t"][0, 0]
            if q["ok"][0, 0] and t > T_MIN and t < best[0]:
                best[:] = [t, bi, prim]
        walk(u32f(blas[bi, 16]), oo, od, triangle)

    walk(0, o, d, instance)
    return (best[0], best[1], best[2]) if best[2] >= 0 else (F(-1.0), -1, -1)


def shaded_hazards(c, w, h):
    """What the rays that the device SHADES reach -- the camera rays of a w x h frame of the case, at their primary hits:
    tex2d_sample's float-to-int step (rt_tri_device.h: hit_albedo, tex2d_sample; fetches in the upper clamp, in the lower clamp,
    with a NaN coordinate) and shading normals that are NaN when the bounce reflects about them."""
    import shade_common
    o, d = shade_common.camera_rays(c.scene.pack_params(2), w, h)
    t, inst, prim = nearest_hits(c, o, d)
    hit = prim >= 0
    out = dict(tex_clamp_hi=0, tex_clamp_lo=0, tex_nan=0, nan_normal_hits=0, hits=int(hit.sum()))
    if not hit.any():
        return out
    with np.errstate(all="ignore"):
        _, u, v, nrm = qc.restate_triangle_hits(c.buf, o[hit], d[hit], prim[hit], inst[hit])
        tr = np.asarray(c.buf["triangles"], F).reshape(-1, 40)[prim[hit]]
        wgt = (F(1.0) - u) - v
        su = (tr[:, 8] * wgt + tr[:, 20] * u) + tr[:, 32] * v
        sv = F(1.0) - ((tr[:, 9] * wgt + tr[:, 21] * u) + tr[:, 33] * v)
        th, tw = c.buf["mesh_tex"].shape[0:2]
        fx, fy = np.floor(su * F(tw) - F(0.5)), np.floor(sv * F(th) - F(0.5))
    for f in (fx, fy):
        out["tex_clamp_hi"] += int((f >= F(2147483520.0)).sum())
        out["tex_clamp_lo"] += int((f <= F(-2147483520.0)).sum())
        out["tex_nan"] += int(np.isnan(f).sum())
    out["nan_normal_hits"] = int(np.isnan(nrm).any(axis=1).sum())
    return out


def count_hazards(c):
    """What the case's constructed rays reach, counted over every box test and triangle test the walk can make (query_common.reach
    with the reference's 9999): see tests/test_tri_edges_cpu.py for the floors.  (What the shaded rays reach: shaded_hazards.)"""
    buf, o, d = c.buf, c.o, c.d
    n = o.shape[0]
    blas = np.asarray(buf["blas"], F).reshape(-1, 20)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    lookup = np.asarray(buf["tri_lookup"], F)
    k = dict(slab_nan=0, slab_subnormal=0, inv_pos_inf=0, inv_neg_inf=0, u_zero=0, u_det=0, uv_det=0, det_below=0, det_above=0,
             t_min_below=0, t_min_above=0, subnormal_accepted=0, subnormal_terms=0, overflowed=0, mirror_culled=0, nan_compare=0)
    seen = set()
    def visit(bi, dirs, dist, t1, t2, mask):
        with np.errstate(all="ignore"):
            inv = F(1.0) / dirs
        if bi not in seen:                               # the inverse direction is formed once per ray and instance
            seen.add(bi)
            k["inv_pos_inf"] += int(((inv == np.inf) & mask[:, None]).sum()) if bi is not None else int((inv == np.inf).sum())
            k["inv_neg_inf"] += int(((inv == -np.inf) & mask[:, None]).sum()) if bi is not None else int((inv == -np.inf).sum())
        k["slab_nan"] += int(((np.isnan(t1) | np.isnan(t2)).any(axis=1) & mask).sum())
        k["slab_subnormal"] += int(((subnormal(t1) | subnormal(t2)).any(axis=1) & mask).sum())
        k["overflowed"] += int(((np.isinf(t1) | np.isinf(t2)).any(axis=1) & mask & np.isfinite(inv).all(axis=1)).sum())
    accepted = []                                        # (ray, t) of every accepted (triangle, instance) pair
    with np.errstate(all="ignore"):
        for bi, (slots, rm) in sorted(qc.reach(buf, o, d, T_MAX, visit).items()):
            if not slots.size:
                continue
            prims = np.array([min(u32f(lookup[s]), tris.shape[0] - 1) for s in slots], np.int64)
            q = triangle_terms(blas[bi], tris[prims], o, d)
            det, u, v, t = q["det"], q["u"], q["v"], q["t"]
            acc = q["ok"] & rm & (t > T_MIN) & (t < T_MAX)
            k["u_zero"] += int((acc & (u == 0)).sum()); k["u_det"] += int((acc & (u == det)).sum())
            k["uv_det"] += int((acc & (u + v == det)).sum())
            k["det_below"] += int((rm & (det >= ulps(THRESH, -4)) & (det < THRESH)).sum())
            k["det_above"] += int((rm & (det >= THRESH) & (det <= ulps(THRESH, 4))).sum())
            k["t_min_below"] += int((q["ok"] & rm & (t >= ulps(T_MIN, -4)) & (t <= T_MIN)).sum())
            k["t_min_above"] += int((q["ok"] & rm & (t > T_MIN) & (t <= ulps(T_MIN, 4))).sum())
            k["subnormal_accepted"] += int((acc & (subnormal(det) | subnormal(u) | subnormal(v) | subnormal(q["tnum"]))).sum())
            k["subnormal_terms"] += int((rm & (subnormal(det) | subnormal(u) | subnormal(v) | subnormal(q["tnum"]))).sum())
            k["overflowed"] += int((rm & (np.isinf(det) | np.isinf(u) | np.isinf(v) | np.isinf(q["tnum"]) | np.isinf(t))).sum())
            k["nan_compare"] += int((rm & (np.isnan(det) | np.isnan(u) | np.isnan(v) | np.isnan(t))).sum())
            if bi in c.mirrored:                         # a back face only because the record mirrors: the same point test on -det
                inside = (det <= -THRESH) & (u <= 0) & (u >= det) & (v <= 0) & (u + v >= det) & (t > T_MIN) & (t < T_MAX)
                k["mirror_culled"] += int((rm & inside).sum())
            ray, col = np.nonzero(acc)
            accepted.append((ray, t[ray, col]))
    ray = np.concatenate([a[0] for a in accepted]) if accepted else np.zeros(0, np.int64)
    t = np.concatenate([a[1] for a in accepted]) if accepted else np.zeros(0, F)
    best = np.full(n, np.inf, F)
    np.minimum.at(best, ray, t)
    k["t_ties"] = int((np.bincount(ray[t == best[ray]], minlength=n) >= 2).sum())
    # the running nearest hit: another accepted hit within 4 representable values of the nearest, on either side of it in the order
    # of the walk (positive floats order as their bit patterns)
    gap = bits(t).astype(np.int64) - bits(best[ray]).astype(np.int64)
    k["t_near_nearest"] = int((np.bincount(ray[(gap > 0) & (gap <= 4)], minlength=n) >= 1).sum())
    k["hits"] = int(np.isfinite(best).sum())
    step, _ = limits_about(np.where(np.isfinite(best), best, F(-1.0)))       # what limits_about gives the rays that hit
    for name, s in (("limit_below", -1), ("limit_at", 0), ("limit_above", 1)):
        k[name] = int((np.isfinite(best) & (step == s)).sum())
    return k
