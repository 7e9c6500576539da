"""Host side of the BLAS refit, checked without a GPU (the library loads and rt_refit_plan runs without a device): the walk that
validates the trees and lists, per node, the run of lookup slots its leaves cover (compute_raytracer_amd/csrc/rt_refit_plan.h
through rt_refit_plan of the C ABI), and the refit itself restated in numpy float32 (tests/refit_common.py: numpy_refit), which
must give back the boxes the builders made, bit for bit -- the statement the GPU test then holds the device to."""
import ctypes

import numpy as np
import pytest

import compute_raytracer_amd as rt
from compute_raytracer_amd import abi
from helpers import leafy_scene, random_sky, ref_fixture, tri_buffers, triangle_scene
from refit_common import (F, FP, LOOKUP, U32, bad_trees, deform, good_tree, mesh_ranges, numpy_refit, refit_plan, tree_by_hand, u32f,
                          B, H, W, view_scene)


def one_triangle_scene():
    """A mesh of one triangle (its root is a leaf) beside a tessellated sphere"""
    from compute_raytracer_amd.procedural import obj_uv_sphere
    one = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\nf 1/1/1 2/2/1 3/3/1\n"
    meshes = [rt.load_mesh(one, dict(color=[1.0, 0.5, 0.2, 1.0], alignBottom=False, scale=1.0)),
              rt.load_mesh(obj_uv_sphere(4, 5), dict(color=[0.3, 0.7, 0.9, 1.0], alignBottom=True, scale=1.0))]
    models = [dict(meshIndex=0, position=[0.5, 1.0, -3.0], eulers=[0, 0, 0]), dict(meshIndex=1, position=[-1.0, 0.0, -4.0], eulers=[0, 30, 0])]
    return rt.SceneRaytracing().createScene([]).createTriangleScene(meshes, models)


def builder_scenes():
    return {"procedural": lambda: triangle_scene(seed=40, n_models=3)[0], "reference": lambda: ref_fixture()[0],
            "one triangle": one_triangle_scene}


def check_plan(nodes, n_lookup, roots, plan):
    """every node under each root exactly once, each with the union of its leaves' runs as ONE run"""
    want = {}
    for r in roots:
        sub = tree_by_hand(nodes, r)
        assert not set(sub) & set(want)
        want.update(sub)
    assert sorted(plan[:, 0].tolist()) == sorted(want)                      # exactly once each
    for node, first, n in plan.tolist():
        assert n >= 1 and first + n <= n_lookup
        assert want[node] == set(range(first, first + n)), node


@pytest.mark.parametrize("name", list(builder_scenes()))
def test_builder_trees_refit_to_their_own_bytes(name):
    scene = builder_scenes()[name]()
    buf = tri_buffers(scene, rt.Material.white())
    nodes, n_lookup = buf["nodes"], len(buf["tri_lookup"])
    roots = sorted(set(int(m.root_node) for m in scene.meshes))
    rc, n_plan, plan = refit_plan(nodes, n_lookup, roots + roots[:1])        # a duplicated root is planned once
    assert rc == abi.RT_OK and n_plan == scene.blasNodesUsed == plan.shape[0]
    check_plan(nodes, n_lookup, roots, plan)
    if name == "one triangle":
        assert u32f(nodes[scene.meshes[0].root_node, 7]) == 1                # the root is a leaf
    refit = numpy_refit(nodes, buf["triangles"], buf["tri_lookup"], plan)
    assert np.array_equal(refit.view(np.uint32), np.asarray(nodes, F).view(np.uint32)), "the numpy refit does not reproduce the builder's boxes"
    # one root only: the other trees are not in the plan
    rc, n_plan, one = refit_plan(nodes, n_lookup, roots[:1])
    assert rc == abi.RT_OK and set(one[:, 0].tolist()) == set(tree_by_hand(nodes, roots[0]))


@pytest.mark.parametrize("per_leaf", [2, 4])
def test_leafy_scene_plan(per_leaf):
    """helpers.leafy_scene: a hand-made spine with `per_leaf` triangles per leaf.  Its boxes are hand-made too (they are not
    the bounds of what lies below them), so a refit cannot give them back: the plan is checked as for the builders' trees, and
    that the restated refit touches the planned boxes only."""
    scene = leafy_scene(per_leaf)
    buf = tri_buffers(scene, rt.Material.white())
    nodes, n_lookup = buf["nodes"], len(buf["tri_lookup"])
    rc, n_plan, plan = refit_plan(nodes, n_lookup, [1])
    assert rc == abi.RT_OK and n_plan == 19
    check_plan(nodes, n_lookup, [1], plan)
    assert plan[0].tolist() == [1, 0, 10 * per_leaf]                         # the root covers every slot
    refit = numpy_refit(nodes, buf["triangles"], buf["tri_lookup"], plan)
    p = plan[:, 0]
    assert sorted(p.tolist()) == list(range(1, 20))
    assert np.array_equal(refit[:, [3, 7]].view(np.uint32), nodes[:, [3, 7]].view(np.uint32))
    assert np.array_equal(refit[0].view(np.uint32), nodes[0].view(np.uint32))   # the top-level node is not the plan's


@pytest.mark.parametrize("name", list(bad_trees()))
def test_bad_trees_are_refused(name):
    nodes, roots, want = bad_trees()[name]
    rc, n_plan, _ = refit_plan(nodes, LOOKUP, roots)
    assert rc == want and n_plan == 0, (name, rc)
    assert abi.load().rt_last_error(None)                                    # a message says why


def test_good_tree_orders_and_adjacent_runs():
    rc, n, plan = refit_plan(good_tree(), LOOKUP, [0])
    assert rc == abi.RT_OK and plan.tolist() == [[0, 0, 5], [1, 0, 2], [2, 2, 3], [3, 2, 1], [4, 3, 2]]
    rc, n, plan = refit_plan(good_tree(), LOOKUP, [2, 2, 1])                 # two roots, one of them twice: ascending, once each
    assert rc == abi.RT_OK and plan.tolist() == [[1, 0, 2], [2, 2, 3], [3, 2, 1], [4, 3, 2]]
    # the right child's run directly before the left's: still one run
    t = np.zeros((3, 8), F); t[0] = [0, 0, 0, 1, 0, 0, 0, 0]; t[1] = [0, 0, 0, 2, 0, 0, 0, 3]; t[2] = [0, 0, 0, 0, 0, 0, 0, 2]
    rc, n, plan = refit_plan(t, LOOKUP, [0])
    assert rc == abi.RT_OK and plan.tolist() == [[0, 0, 5], [1, 2, 3], [2, 0, 2]]


def test_argument_checks_and_capacity():
    L = abi.load()
    g = np.ascontiguousarray(good_tree())
    roots = np.array([0], np.uint32)
    plan = np.zeros((8, 3), np.uint32)
    n = ctypes.c_uint32(77)
    args = lambda nodes=g.ctypes.data_as(FP), r=roots.ctypes.data_as(U32), nr=1, p=plan.ctypes.data_as(U32), cap=8, out=ctypes.byref(n): (
        nodes, 5, LOOKUP, r, nr, p, cap, out)
    assert L.rt_refit_plan(*args(nodes=None)) == abi.RT_ERR_INVALID_ARG
    assert L.rt_refit_plan(*args(r=None)) == abi.RT_ERR_INVALID_ARG
    assert L.rt_refit_plan(*args(out=None)) == abi.RT_ERR_INVALID_ARG
    assert L.rt_refit_plan(*args(r=None, nr=0)) == abi.RT_OK and n.value == 0            # no root: nothing to plan
    n.value = 77
    assert L.rt_refit_plan(*args(cap=4)) == abi.RT_ERR_CAPACITY and n.value == 5         # *n_plan is set all the same
    assert not plan.any()                                                                 # ... and nothing was written
    n.value = 77
    assert L.rt_refit_plan(*args(p=None, cap=0)) == abi.RT_ERR_CAPACITY and n.value == 5
    assert L.rt_refit_plan(*args(cap=5)) == abi.RT_OK and n.value == 5 and plan[:5, 0].tolist() == [0, 1, 2, 3, 4]
    assert L.rt_abi_version() == 4


@pytest.mark.parametrize("kind", ["grow", "shrink"])
def test_the_deformations_can_show_a_stale_box(oracle, kind):
    """The input condition of the GPU test's pixel checks, shown on the CPU: with the grown mesh and the OLD boxes the oracle
    renders another picture than with refitted boxes (a stale box cuts geometry), so a frame that equals the oracle on the
    refitted boxes shows that the refit reached the kernel.  The shrunk mesh stays inside its old ROOT box (the boxes below it
    are left by the triangles that move towards the mesh's centre): far fewer pixels can tell, the node bytes always do."""
    scene, mat = view_scene()
    sky = random_sky(31)
    buf = tri_buffers(scene, mat)
    root, first, count = mesh_ranges(scene)[1]
    tris = deform(buf["triangles"], first, count, kind)
    rc, _, plan = refit_plan(buf["nodes"], len(buf["tri_lookup"]), [root])
    assert rc == abi.RT_OK
    fresh = numpy_refit(buf["nodes"], tris, buf["tri_lookup"], plan)
    assert not np.array_equal(fresh, buf["nodes"])
    params = scene.pack_params(B)
    stale_img = oracle.render_tri(params, dict(buf, triangles=tris), sky.faces, W, H)[0]
    fresh_img = oracle.render_tri(params, dict(buf, triangles=tris, nodes=fresh), sky.faces, W, H)[0]
    differ = int((stale_img != fresh_img).any(axis=-1).sum())
    if kind == "grow":
        assert differ > 20, differ
        assert np.any(fresh[plan[:, 0], 0:3] < buf["nodes"][plan[:, 0], 0:3])          # the mesh left its old boxes
    else:
        r = np.nonzero(plan[:, 0] == root)[0][0]
        assert np.all(fresh[root, 0:3] >= buf["nodes"][root, 0:3]) and np.all(fresh[root, 4:7] <= buf["nodes"][root, 4:7])
        assert plan[r, 2] == count
