"""Shared by the device-BLAS-build tests (test infrastructure; tests/test_build_blas_cpu.py, tests/test_build_blas_gpu.py):
rt_build_blas_host through the C ABI, soups made of the float32 corners of triangle records, the canonical form of a lookup table
(the builder's two-pointer sweep and the library's stable partition order the slots INSIDE a leaf differently), the
well-formedness walk, and the meshes."""
import ctypes

import numpy as np

from compute_raytracer_amd import abi
from compute_raytracer_amd.acceleration.bvh import MeshTree, build_tree
from compute_raytracer_amd.soup import TriangleSoup
from refit_common import CORNER_COLS, F, FP, U32, u32f


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- records and soups ----
def records_of(corners, color=(0.8, 0.7, 0.6, 1.0)):
    """(T, 40) float32 triangle records with the given (T, 3, 3) corners, a constant normal and zero uv"""
    corners = np.asarray(corners, F).reshape(-1, 3, 3)
    n = np.zeros_like(corners, dtype=np.float64)
    n[..., 1] = 1.0
    return TriangleSoup(corners.astype(np.float64), n, np.zeros((corners.shape[0], 3, 2)), color).pack()


def corners_of(records):
    t = np.asarray(records, F).reshape(-1, 40)
    return np.stack([t[:, c] for c in CORNER_COLS], axis=1)


def soup_of(records, color=(0.8, 0.7, 0.6, 1.0)):
    """the soup whose positions are the float32 corners of `records` -- what rt_build_blas builds a tree of"""
    t = np.asarray(records, F).reshape(-1, 40)
    c = corners_of(t).astype(np.float64)
    nrm = np.stack([t[:, 4:7], t[:, 16:19], t[:, 28:31]], axis=1).astype(np.float64)
    uv = np.stack([t[:, 8:10], t[:, 20:22], t[:, 32:34]], axis=1).astype(np.float64)
    return TriangleSoup(c, nrm, uv, color)


def one_leaf_tree(soup):
    """a dummy tree: the root is a leaf of every triangle (what a scene is written with before rebuild())"""
    c = soup.position.reshape(-1, 3)
    t = MeshTree()
    t.lo, t.hi = c.min(axis=0)[None, :].copy(), c.max(axis=0)[None, :].copy()
    t.first, t.count = np.zeros(1, np.int64), np.array([soup.count], np.int64)
    t.order, t.used = np.arange(soup.count, dtype=np.int64), 1
    t.box_lo, t.box_hi = np.array([999999.0] * 3), np.array([-999999.0] * 3)
    return t


# ---- the meshes ----
def random_records(T, seed, spread=4.0, size=0.6):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-spread, spread, (T, 1, 3))
    return records_of((centre + rng.uniform(-size, size, (T, 3, 3))).astype(F))


def grid_vertices(n=12):
    g = np.arange(n + 1, dtype=np.float64) - n / 2.0
    v = np.zeros((n + 1, n + 1, 3))
    v[..., 0], v[..., 2] = g[:, None], g[None, :]
    return v


def grid_records(vertices=None, n=12):
    """the flat n x n grid in y = 0, two triangles a cell: every cost on the y axis is a tie, the leaves hold two triangles"""
    v = grid_vertices(n) if vertices is None else vertices
    tri = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = v[i, j], v[i + 1, j], v[i + 1, j + 1], v[i, j + 1]
            tri += [(a, c, b), (a, d, c)]
    return records_of(np.array(tri))


def duplicate_records(copies=40):
    one = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, 0.5]])
    return records_of(np.repeat(one[None], copies, axis=0))


PERTURB_SEED = 3


def perturbed_grid_records(seed=PERTURB_SEED, n=12):
    """the grid with its vertices moved at random (shared vertices move together): build_tree then needs more than the flat
    grid's 287 nodes (tests/test_build_blas_cpu.py asserts it for this seed)"""
    rng = np.random.default_rng(seed)
    return grid_records(grid_vertices(n) + rng.uniform(-0.45, 0.45, (n + 1, n + 1, 3)), n)


def helper_mesh_records():
    """the three meshes of helpers.triangle_scene (96, 176 and 2 triangles) as records"""
    from refit_common import view_scene
    scene, _ = view_scene()
    return [m.soup.pack() for m in scene.meshes]


def skew_records(n=48, seed=7):
    """n small triangles whose centroids fall geometrically along x (x_k = 10^(-k/2), extents of about 1 % of x_k): every split
    peels the farthest few off, so build_tree makes a long chain of levels two or four nodes wide"""
    rng = np.random.default_rng(seed)
    x = 10.0 ** (-np.arange(n) / 2.0)
    centre = np.stack([x, np.zeros(n), np.zeros(n)], axis=1)[:, None, :]
    return records_of((centre + 0.01 * x[:, None, None] * rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(F))


# runs of exactly a wave (64), two (128), the longest short run (256: kBuildShort), two whole chunks of the block partition (512)
# and one past them
MESHES = {"T1": lambda: random_records(1, 101), "T2": lambda: random_records(2, 102), "T3": lambda: random_records(3, 103),
          "T64": lambda: random_records(64, 164), "T65": lambda: random_records(65, 165), "T128": lambda: random_records(128, 228),
          "T256": lambda: random_records(256, 356), "T257": lambda: random_records(257, 357), "T512": lambda: random_records(512, 612),
          "T513": lambda: random_records(513, 613), "T1000": lambda: random_records(1000, 1100),
          "grid": grid_records, "duplicates": duplicate_records, "skew": skew_records,
          "helper0": lambda: helper_mesh_records()[0], "helper1": lambda: helper_mesh_records()[1], "helper2": lambda: helper_mesh_records()[2]}
_cache = {}

# ---- the mixed scene: long, short and one-triangle runs side by side in the blocks of four nodes of a level ----
# ranges in mesh order make level 0 two blocks: {long, short, single, long} and {short, long, short-that-stays-a-leaf}
MIXED_COUNTS = (300, 65, 1, 600, 2, 257, 40)
MIXED_PLACES = ([-5.0, 0.5, -9.0], [0.0, 0.5, -7.0], [1.5, 2.0, -3.0], [5.0, 0.5, -9.0], [-1.5, 2.0, -3.0], [0.0, 0.5, -16.0], [0.0, 3.0, -4.0])


def mixed_records():
    """the seven meshes' records: random ones with distinct seeds, the last forty copies of one triangle"""
    if "mixed" not in _cache:
        _cache["mixed"] = [random_records(T, 900 + k) for k, T in enumerate(MIXED_COUNTS[:-1])] + [duplicate_records(MIXED_COUNTS[-1])]
    return _cache["mixed"]


def mixed_scene():
    """the seven meshes, each written with the one-leaf tree and laid out "full", one instance of each in view of the camera"""
    import compute_raytracer_amd as rt
    from compute_raytracer_amd.scene_raytracing import TriMesh
    soups = [soup_of(rec) for rec in mixed_records()]
    meshes = [TriMesh(s, one_leaf_tree(s)) for s in soups]
    models = [dict(meshIndex=k, position=list(p), eulers=[20, 30 + 40 * k, 0]) for k, p in enumerate(MIXED_PLACES)]
    return rt.SceneRaytracing().createScene([]).createTriangleScene(meshes, models, node_capacity="full")


def mixed_trees():
    """build_tree of each of the seven meshes: computed once, shared by the tests, never changed"""
    if "mixed_trees" not in _cache:
        _cache["mixed_trees"] = [build_tree(soup_of(rec)) for rec in mixed_records()]
    return _cache["mixed_trees"]


def mesh_rows(scene):
    """the ranges rebuild() passes: (root_node, node_cap, first_slot, n_slots) per mesh"""
    ends = [m.root_node for m in scene.meshes[1:]] + [scene.node_buffer_length()]
    return [(m.root_node, e - m.root_node, m.lookup_offset, m.soup.count) for m, e in zip(scene.meshes, ends)]


def mesh_and_tree(name):
    """(records, build_tree of their soup) of MESHES[name]: computed once, shared by the tests, never changed"""
    if name not in _cache:
        rec = MESHES[name]()
        _cache[name] = (rec, build_tree(soup_of(rec)))
    return _cache[name]


# ---- rt_build_blas_host ----
def ranges_array(rows):
    r = np.zeros(len(rows), dtype=abi.BLAS_RANGE_DTYPE)
    for k, row in enumerate(rows):
        r[k] = tuple(int(x) for x in row)
    return r


def build_host(triangles, tri_lookup, nodes, rows):
    """rt_build_blas_host on copies -> (status, nodes, lookup, used)"""
    L = abi.load()
    t = np.ascontiguousarray(triangles, F).reshape(-1, 40)
    lk = np.array(tri_lookup, F).reshape(-1).copy()
    nd = np.array(nodes, F).reshape(-1, 8).copy()
    r = ranges_array(rows)
    used = np.full(max(len(rows), 1), 0xFFFFFFFF, np.uint32)
    rc = L.rt_build_blas_host(t.ctypes.data_as(FP), t.shape[0], lk.ctypes.data_as(FP), lk.shape[0], nd.ctypes.data_as(FP), nd.shape[0],
                              r.ctypes.data_as(ctypes.POINTER(abi.RtBlasRange)), len(rows), used.ctypes.data_as(U32))
    return rc, nd, lk, used[:len(rows)]


def builder_arrays(records, root_node, first_slot, tri_base=0):
    """build_tree of the records' soup, laid out at root_node / first_slot -> ((used, 8) nodes, (T,) lookup words, the tree)"""
    tree = build_tree(soup_of(records))
    lookup = (tree.order + tri_base).astype(np.float64).astype(F)
    return tree.nodes(root_node, first_slot), lookup, tree


# ---- canonical form and well-formedness ----
def leaves_of(nodes, root):
    """[(first_slot, count)] of the leaves under `root`, by a walk that checks every node is reached once"""
    nodes = np.asarray(nodes, F).reshape(-1, 8)
    seen, out, todo = set(), [], [root]
    while todo:
        i = todo.pop()
        assert 0 <= i < nodes.shape[0] and i not in seen, "node %d reached twice or beyond the buffer" % i
        seen.add(i)
        left, count = u32f(nodes[i, 3]), u32f(nodes[i, 7])
        if count:
            out.append((left, count))
        else:
            todo += [left + 1, left]
    return out, seen


def level_widths(nodes, root):
    """[node count per depth] under `root`, from a breadth-first walk: the widths of the levels a level-by-level build goes through"""
    nodes = np.asarray(nodes, F).reshape(-1, 8)
    widths, level = [], [root]
    while level:
        widths.append(len(level))
        assert sum(widths) <= nodes.shape[0], "a cycle"
        nxt = []
        for i in level:
            if u32f(nodes[i, 7]) == 0:
                left = u32f(nodes[i, 3])
                nxt += [left, left + 1]
        level = nxt
    return widths


def canonical(lookup, nodes, root):
    """the lookup table with the run of every leaf under `root` sorted"""
    out = np.array(lookup, F).copy()
    for first, count in leaves_of(nodes, root)[0]:
        out[first:first + count] = np.sort(out[first:first + count])
    return out


def check_rows_are_build_tree(nodes, lookup, before_nodes, before_lookup, rows, trees, built=None):
    """ranges `built` (indices into rows; None: all) hold build_tree's nodes bit for bit and its order up to the order inside a
    leaf (slot s of a mesh held triangle first_slot + s before); every other node and slot is what it was"""
    built = range(len(rows)) if built is None else built
    node_same, slot_same = np.ones(len(nodes), bool), np.ones(len(lookup), bool)
    for k in built:
        root, cap, first, n = rows[k]
        tree = trees[k]
        assert tree.used <= cap
        assert np.array_equal(bits(nodes[root:root + tree.used]), bits(tree.nodes(root, first))), "mesh %d" % k
        want = np.array(before_lookup, F).copy()
        want[first:first + n] = (tree.order + first).astype(F)
        assert np.array_equal(canonical(lookup, nodes, root)[first:first + n], canonical(want, nodes, root)[first:first + n]), "mesh %d" % k
        node_same[root:root + tree.used] = False
        slot_same[first:first + n] = False
    assert np.array_equal(bits(nodes[node_same]), bits(np.asarray(before_nodes, F)[node_same]))      # gaps, unused capacity, the others
    assert np.array_equal(bits(lookup[slot_same]), bits(np.asarray(before_lookup, F)[slot_same]))


def check_well_formed(nodes, lookup, row, used, before_lookup):
    """the tree of range `row` = (root_node, node_cap, first_slot, n_slots): its nodes are exactly [root, root + used), every
    slot of the range lies in exactly one leaf, and the range's lookup words are a permutation of what they were"""
    root, cap, first, n = [int(x) for x in row]
    assert 1 <= used <= cap
    leaves, seen = leaves_of(nodes, root)
    assert seen == set(range(root, root + used))
    cover = np.zeros(n, np.int64)
    for lf, cnt in leaves:
        assert first <= lf and lf + cnt <= first + n
        cover[lf - first:lf - first + cnt] += 1
    assert (cover == 1).all()
    assert np.array_equal(np.sort(bits(lookup[first:first + n])), np.sort(bits(before_lookup[first:first + n])))
