"""Shared by the instance-mask tests (test infrastructure; tests/test_instance_masks_cpu.py, test_instance_masks_gpu.py): the masks
and the ray-mask trials they use, and the reference of a masked query -- the twin scene.

For buffers whose indices are all in range, the masked query on `buf` equals the unmasked reference on twin(buf, visible), bit for
bit: the twin is `buf` with one all-zero triangle record appended (three equal corners), one lookup slot naming it, one node
{left = that slot, count = 1} appended to the node buffer, and word 16 of every invisible BLAS record pointing at that node.
hitTriangle rejects that triangle (det = 0 < 0.00001, RK:359), so an invisible instance contributes nothing; the top-level walk
and every visible instance's walk are untouched.  Every existing reference (oracle.trace_tri_rays, check_triangle_hits,
brute_triangles, all_triangle_hits + k_smallest, oracle.render_tri, ao_common) then serves unchanged, given the twin.  Buffers
with wild indices are not for this: they clamp to the last entry, and the twin moves the last entry."""
import numpy as np

from query_common import F, all_triangle_hits, bits, k_smallest

ALL = 0xFFFFFFFF
TRIALS = (0, 0xFFFFFFFF, 0x1, 0x2, 0x80000004, 0x7FFFFFF8)      # the ray masks every test tries; 0 and 0x7FFFFFF8 hide everything


def instance_masks(n):
    """m_i = (1 << (i % 3)) | (0x80000000 if i is odd), and m_1 = 0 in a scene of at least four records"""
    m = np.array([(1 << (i % 3)) | (0x80000000 if i % 2 else 0) for i in range(n)], np.uint32)
    if n >= 4:
        m[1] = 0
    return m


def visible(masks, ray, n=None):
    """(n,) bool: record i is visible to a ray of mask `ray` under the table `masks` (records beyond it: 0xFFFFFFFF)"""
    masks = np.asarray(masks, np.uint32)
    n = masks.shape[0] if n is None else n
    full = np.full(n, ALL, np.uint32)
    full[:min(n, masks.shape[0])] = masks[:n]
    return (full & np.uint32(ray)) != 0


def twin(buf, vis):
    """The twin of `buf` for the visibility `vis` ((n_blas,) bool): a new dict, `buf` itself is left as it is."""
    vis = np.asarray(vis, bool)
    tris = np.asarray(buf["triangles"], F).reshape(-1, 40)
    nodes = np.asarray(buf["nodes"], F).reshape(-1, 8)
    blas = np.asarray(buf["blas"], F).reshape(-1, 20).copy()
    lookup = np.asarray(buf["tri_lookup"], F).reshape(-1)
    assert vis.shape == (blas.shape[0],)
    n_tri, n_slot, n_node = tris.shape[0], lookup.shape[0], nodes.shape[0]
    assert max(n_tri, n_slot, n_node) < 2 ** 24                     # the indices are float32 words
    leaf = np.zeros((1, 8), F)
    leaf[0, 3], leaf[0, 7] = n_slot, 1
    blas[~vis, 16] = n_node
    out = dict(buf)
    out.update(triangles=np.concatenate([tris, np.zeros((1, 40), F)]), tri_lookup=np.concatenate([lookup, np.array([n_tri], F)]),
               nodes=np.concatenate([nodes, leaf]), blas=blas)
    return out


def filter_hits(cand, vis):
    """all_triangle_hits' (ray, t, instance, prim) without the hits of invisible instances"""
    ray, t, inst, prim = cand
    keep = np.asarray(vis, bool)[inst]
    return ray[keep], t[keep], inst[keep], prim[keep]


def nearest_of(n, cand):
    """The nearest t within (0.001, 9999) of the candidates per ray, -1 where none: the float32 brute force's answer"""
    return k_smallest(n, 1, cand, F(0.001), F(9999.0))[0][:, 0]


def moving_trials(oracle, buf, o, d, masks):
    """How the reference alone answers under each trial: [(trial, rays hitting, rays whose t differs from the unmasked
    reference's)] -- a test that passes on answers that do not move shows nothing."""
    n_blas = np.asarray(buf["blas"]).reshape(-1, 20).shape[0]
    base = oracle.trace_tri_rays(buf, o, d)
    out = []
    for trial in TRIALS:
        t = oracle.trace_tri_rays(twin(buf, visible(masks, trial, n_blas)), o, d)
        out.append((trial, int((t != F(-1.0)).sum()), int((bits(t) != bits(base)).sum())))
    return out


def assert_trials_move(oracle, buf, o, d, masks, need=20):
    """In a scene of three or more records at least two trials leave `need` rays hitting and change the answer of `need` rays"""
    moved = moving_trials(oracle, buf, o, d, masks)
    good = [m for m in moved if m[1] >= need and m[2] >= need]
    assert len(good) >= 2, "the trials do not move the reference: %s" % (moved,)
    return moved
