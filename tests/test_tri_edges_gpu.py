"""The triangle kernels against the CPU oracle at the edges of float32 (tests/tri_edge_common.py has the cases and the one
comparison rule; tests/test_tri_edges_cpu.py shows that the inputs reach the edges): frames in both kernel variants, the heatmap
kernel, frames in flight, the split-tile forms, every ray-query family in three walk forms, the frame-shaped queries, and refit
and device builds at the extremes of scale.  Bytes and integers are compared exactly, float words by the rule; every pixel and
every ray of every case is compared.  Each test prints the number of NaN-against-NaN words the rule let pass."""
import numpy as np
import pytest

import compute_raytracer_amd as rt
import query_common as qc
import shade_common
import tri_edge_common as te
from ao_common import ao_of, ao_rays, counts_from
from compute_raytracer_amd import abi
from helpers import diff_stats, expected_form, random_sky, tri_buffers
from query_common import F
from test_render_samples_cpu import resolve_np

pytestmark = pytest.mark.gpu

W, H = 72, 40
SKY = random_sky(5)
HONEST = [n for n in te.CASES if te.HAZARD_CLASS[n] != 5]
_frames = {}


def ref_frame(oracle, c, bounces, w=W, h=H):
    """(rgba8, float rgb, rays) of the oracle, computed once per (case, bounces, size)"""
    key = (c.name, bounces, w, h, c.buf["tri_lookup"].shape[0])
    if key not in _frames:
        _frames[key] = oracle.render_tri(c.scene.pack_params(bounces), c.buf, SKY.faces, w, h, want_float=True)
    return _frames[key]


def renderer(c, bounces=2, variant=0, w=W, h=H):
    r = rt.RendererRaytracing(w, h, c.scene, maxBounces=bounces).initialize(SKY, c.mat)
    r.set_variant(variant)
    return r


def awaited_form(c, variant=0):
    """rt_triangles.hip rt_tri_stack_form for an awaited frame: the small forms walk pair records (variant 0, every count, index
    and slot within 16 bits, leaves of at most three); the tiny form is the in-flight one"""
    nodes = c.buf["nodes"]
    words = nodes[:, [3, 7]]
    packed = len(c.buf["tri_lookup"]) <= 65536 and not (np.nan_to_num(words, nan=0.0) > 16383).any()
    if variant != 0 or not packed:
        return 0
    want = expected_form(c.scene, c.mat)
    return 1 if want == 2 else want


def report(c, cmp, what):
    print("NAN_MATCHES class %d %s %s: %d" % (te.HAZARD_CLASS.get(c.name, 0), c.name, what, cmp.nan_matches))


def float_frame_matches(r, c, ref_rgb, cmp, what):
    o, d = shade_common.camera_rays(c.scene.pack_params(r.maxBounces), r.width, r.height)
    got = r.shade_rays(o, d, compose=True)
    bad = cmp.differ(got[:, 0:3], ref_rgb.reshape(-1, 3)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d float pixels differ from the oracle's" % (what, int(bad.sum()), bad.size)


# ---- frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 6])
@pytest.mark.parametrize("name", list(te.CASES))
def test_frames(oracle, name, variant):
    """An awaited frame, its float colour, three frames in flight and (variant 0) the heatmap kernel, every pixel."""
    c = te.case(name)
    cmp = te.Comparator()
    ref, ref_rgb, rays = ref_frame(oracle, c, 2)
    r = renderer(c, 2, variant)
    try:
        r.render()
        img, st = r.read_pixels(), r.stats()
        assert np.array_equal(img, ref), diff_stats(img, ref)
        assert st["rays"] == rays and abi.KERNEL_IDS[st["kernel_id"]] == "triangles"
        assert st["tri_form"] == awaited_form(c, variant), (st["tri_form"], awaited_form(c, variant))
        float_frame_matches(r, c, ref_rgb, cmp, "awaited")
        # three frames in flight, twice: the library learns at rt_wait that its frames overlap, so the first batch still runs the
        # awaited form and the second the in-flight one (the tiny form where the tree fits it: rt_tri_stack_form)
        small = awaited_form(c, variant)
        for want in (small, expected_form(c.scene, c.mat) if small else 0):
            for _ in range(3):
                r.enqueue()
            r.wait()
            img, st = r.read_pixels(), r.stats()
            assert np.array_equal(img, ref), diff_stats(img, ref)
            assert st["tri_form"] == want and st["batch_frames"] == 3, (st["tri_form"], want)
        if variant == 0:
            want, _ = oracle.heatmap_tri(c.scene.pack_params(2), c.buf, W, H)
            r.showHeatmap()
            r.render()
            assert np.array_equal(r.read_pixels(), want) and abi.KERNEL_IDS[r.stats()["kernel_id"]] == "heatmap"
    finally:
        r.close()
    report(c, cmp, "frames v%d" % variant)


@pytest.mark.parametrize("bounces", [0, 8])
def test_no_bounce_and_eight(oracle, bounces):
    c = te.case("matrices")
    cmp = te.Comparator()
    ref, ref_rgb, rays = ref_frame(oracle, c, bounces)
    r = renderer(c, bounces)
    try:
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, ref), diff_stats(img, ref)
        assert r.stats()["rays"] == rays
        one, flt = r.render_samples(1, float_out=True)
        assert np.array_equal(one, ref)
        assert not cmp.differ(flt[:, :, 0:3], ref_rgb).any()
    finally:
        r.close()
    report(c, cmp, "bounces %d" % bounces)


def test_split_tile_forms(oracle):
    """512 x 512 = 4,096 tiles, from which on an awaited frame renders from the work list the frame before it on its stream left
    (and, where that list splits tiles, in the roles kernel): the mixed case at 8 bounces, twelve frames of an unchanged scene
    The oracle's per-tile work is skewed twentyfold here (most tiles are sky): the lists split tiles."""
    c = te.case("mixed")
    ref, _, rays = ref_frame(oracle, c, 8, 512, 512)
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 100
    r = renderer(c, 8, 0, 512, 512)
    kernels, wrong = [], []
    try:
        for f in range(12):
            r.render()
            img, st = r.read_pixels(), r.stats()
            kernels.append(abi.KERNEL_IDS[st["kernel_id"]])
            if not np.array_equal(img, ref) or st["rays"] != rays or st["tri_form"] != awaited_form(c):
                wrong.append((f, diff_stats(img, ref), st["rays"], rays, st["tri_form"]))
    finally:
        r.close()
    print("SPLIT_TILE kernels", kernels)
    assert not wrong, wrong[:3]
    assert set(kernels) <= {"triangles", "triangles_roles"} and "triangles_roles" in kernels[1:], kernels


# ---- ray queries ------------------------------------------------------------------------------------------------------------------
def beyond_the_packed_stack(name):
    """The case with a lookup table of more than 65,536 entries (its own plus unused padding): the walk that pushes node indices
    (tests/test_triangles_gpu.py: test_scenes_beyond_the_packed_stack_take_the_index_stack)"""
    c = te.CASES[name]()
    c.scene.static["tri_lookup"] = np.concatenate([np.asarray(c.scene.static["tri_lookup"], F), np.zeros(70000, F)])
    c.buf = tri_buffers(c.scene, c.mat)
    return c


WALKS = ("node", "pairs", "index")          # no frame yet: the node walk; after a frame: pair records; a long lookup table: index stacks


def query_subject(oracle, name, walk):
    c = beyond_the_packed_stack(name) if walk == "index" else te.case(name)
    r = renderer(c)
    if walk == "node":
        r.recalculateScene()
    else:
        r.render()
        assert np.array_equal(r.read_pixels(), ref_frame(oracle, c, 2)[0])
        assert r.stats()["tri_form"] == (awaited_form(c) if walk == "pairs" else 0)
    return c, r


def limits_about_the_hit(r, c, cmp):
    """tmax and tmin one value below, at and one value above the nearest t, against the brute force: both limits are strict"""
    o, d = c.o, c.d
    t = r.trace_rays(o, d)["t"]
    hit = t > 0
    _, about = te.limits_about(t)
    for tmin, tmax in ((np.full(o.shape[0], te.T_MIN, F), np.where(hit, about, te.T_MAX).astype(F)),
                       (np.where(hit, about, te.T_MIN).astype(F), np.full(o.shape[0], te.T_MAX, F))):
        h = r.trace_rays(o, d, tmin=tmin, tmax=tmax)
        with np.errstate(all="ignore"):
            best = qc.brute_triangles(c.buf, o, d, tmin, tmax, boxes=True)
        found = h["prim"] >= 0
        assert np.array_equal(found, np.isfinite(best)), "limits about the hit: %d rays" % int((found != np.isfinite(best)).sum())
        assert not cmp.differ(h["t"], np.where(found, best, F(-1.0))).any()
        assert np.array_equal(r.occluded(o, d, tmin, tmax), found)
    return int(hit.sum())


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", HONEST)
def test_every_query_family(oracle, name, walk):
    c, r = query_subject(oracle, name, walk)
    cmp = te.Comparator()
    try:
        hits = qc.check_all_queries(oracle, r, c.state(2, SKY), (c.o, c.d), differ=cmp.differ, boxes=True)
        assert hits == limits_about_the_hit(r, c, cmp)
        if name == "thresholds":                        # ties and near-ties: the hit the walk meets first (76 in one leaf, 78 across two)
            h = r.trace_rays(c.o, c.d)
            rays = np.nonzero((h["prim"] >= 76) & (h["prim"] <= 82) & (h["instance"] == 0))[0]
            won = [te.nearest_by_walk(c.buf, c.o[i], c.d[i]) for i in rays]
            assert np.array_equal(h["prim"][rays], [w[2] for w in won]) and np.array_equal(qc.bits(h["t"][rays]), qc.bits([w[0] for w in won]))
            assert (h["prim"][rays] == 76).sum() >= 50 and (h["prim"][rays] == 78).sum() >= 50
            assert not np.isin(h["prim"][rays], (77, 79)).any()
    finally:
        r.close()
    report(c, cmp, "queries %s, %d hits" % (walk, hits))


@pytest.mark.parametrize("walk", WALKS)
def test_queries_on_degenerate_geometry(oracle, walk):
    """Boxes that do not bound and words that are not counts: the oracle's own walk is the only reference.  Nearest and pick
    against it; a tmax at or below the nearest t is a miss (the limited walk visits a subset of the unlimited one's leaves in the
    same order) and the reference's limits under RT_QUERY_LIMITS change nothing; shaded rays against its float frame."""
    c, r = query_subject(oracle, "degenerate", walk)
    cmp = te.Comparator()
    try:
        o, d = c.o, c.d
        near = r.trace_rays(o, d)
        hits = qc.check_triangle_hits(oracle, c.buf, o, d, near, cmp.differ)
        assert hits >= 50
        hit = near["prim"] >= 0
        rng = np.random.default_rng(7)
        below = np.where(rng.random(o.shape[0]) < 0.3, near["t"], near["t"] * rng.uniform(0.0, 1.0, o.shape[0]).astype(F)).astype(F)
        h = r.trace_rays(o[hit], d[hit], tmax=below[hit])
        assert np.all(h["prim"] == -1) and np.all(h["t"] == F(-1.0))
        assert not r.occluded(o[hit], d[hit], te.T_MIN, below[hit]).any()
        same = r.trace_rays(o, d, tmin=te.T_MIN, tmax=te.T_MAX)
        for k in ("t", "u", "v", "normal"):
            assert not cmp.differ(same[k], near[k]).any(), k
        assert np.array_equal(same["prim"], near["prim"]) and np.array_equal(same["instance"], near["instance"])
        float_frame_matches(r, c, ref_frame(oracle, c, 2)[1], cmp, "shaded")
        ys, xs = np.mgrid[0:H:3, 0:W:3]
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        params = c.scene.pack_params(2)
        dirs = np.stack([oracle.ray_dir(params, W, H, int(x), int(y)) for x, y in zip(xs, ys)])
        qc.check_triangle_hits(oracle, c.buf, np.broadcast_to(params[0:3], dirs.shape).astype(F), dirs, r.pick(xs, ys), cmp.differ)
    finally:
        r.close()
    report(c, cmp, "queries %s, %d hits" % (walk, hits))


# ---- frame-shaped queries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boxes", "thresholds", "matrices"])
def test_frame_shaped_queries(oracle, name):
    c = te.case(name)
    cmp = te.Comparator()
    r = renderer(c)
    try:
        r.recalculateScene()
        ys, xs = np.mgrid[0:H, 0:W]
        p = r.pick(xs.reshape(-1), ys.reshape(-1))
        assert 0 < int((p["prim"] >= 0).sum()) < W * H
        # geometry frames: every plane is pick at every pixel
        g = r.render_gbuffer()
        planes = {"t": g["depth"].reshape(-1), "u": g["uv"][:, :, 0].reshape(-1), "v": g["uv"][:, :, 1].reshape(-1),
                  "normal": np.ascontiguousarray(g["normal"][:, :, 0:3]).reshape(-1, 3)}
        for k, v in planes.items():
            assert not cmp.differ(v, p[k]).any(), k
        assert np.array_equal(g["ids"][:, :, 0].reshape(-1), p["prim"]) and np.array_equal(g["ids"][:, :, 1].reshape(-1), p["instance"])
        assert np.all(qc.bits(g["normal"][:, :, 3]) == 0)
        # ambient occlusion, k = 8: pick -> ao_rays -> occluded -> sum
        k = 8
        dirs = rt.ao_directions(k)
        o, d = qc.camera_rays(c.scene, W, H)
        hit, rays = ao_rays(p, o, d, dirs, 0.001, 1.0)
        flat = rays.reshape(-1, 8)
        occ = r.occluded(flat[:, 0:3], flat[:, 4:7], flat[:, 3], flat[:, 7])
        want = counts_from(W * H, hit, occ, k).reshape(H, W)
        ao = r.render_ao(k=k, radius=1.0, planes=("count", "ao"))
        assert np.array_equal(ao["count"], want), "%d counts differ from the composition" % int((ao["count"] != want).sum())
        assert np.array_equal(qc.bits(ao["ao"]), qc.bits(ao_of(want, k)))
        # supersampled frames, s = 2: the oracle's 144 x 80 frame, box-averaged
        big = ref_frame(oracle, c, 2, 2 * W, 2 * H)[1]
        resolved = resolve_np(big, 2)
        img, flt = r.render_samples(2, float_out=True)
        bad = cmp.differ(flt[:, :, 0:3], resolved).any(axis=-1)
        assert not bad.any(), "%d float pixels differ from the resolved oracle frame" % int(bad.sum())
        assert np.array_equal(img[:, :, 0:3], shade_common.quantise(resolved)) and np.all(img[:, :, 3] == 255)
    finally:
        r.close()
    report(c, cmp, "frame-shaped")


# ---- refit and device build at the extremes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scale-60", "scale+60", "far23"])
def test_refit_and_rebuild_at_the_extremes(oracle, name):
    """refit(): the boxes against the numpy refit of the planned nodes; rebuild(): nodes and lookup against the host model of the
    build (rt_build_blas_host) and against the Python builder's tree; then a frame of what the device holds against the oracle.
    At 2^60 every SAH cost is beyond the builder's starting value of 1e30: there the Python builder still sweeps by plane 0.0 and
    the library's build keeps the node a leaf (rt_blas_build.h names this departure) -- one leaf of all 87 triangles."""
    from build_common import build_host, builder_arrays, canonical, mesh_rows
    from refit_common import numpy_refit, refit_plan
    c = te.case_scaled(int(name[5:]), full=True) if name.startswith("scale") else te.case_far(int(name[3:]), full=True)
    r = renderer(c)
    try:
        r.recalculateScene()
        before = tri_buffers(c.scene, c.mat)
        root = int(c.scene.meshes[0].root_node)
        rc, n_plan, plan = refit_plan(before["nodes"], len(before["tri_lookup"]), [root])
        assert rc == abi.RT_OK and n_plan > 40
        r.refit()
        want = numpy_refit(before["nodes"], before["triangles"], before["tri_lookup"], plan)
        got = r.read_nodes()
        bad = np.nonzero((qc.bits(got) != qc.bits(want)).any(axis=1))[0]
        assert bad.size == 0, "refit: nodes %s differ from the numpy refit" % bad[:8]
        rows = mesh_rows(c.scene)
        used = r.rebuild()
        rc, want_nodes, want_lookup, want_used = build_host(before["triangles"], before["tri_lookup"], got, rows)
        assert rc == abi.RT_OK and used == [int(want_used[0])]
        got_nodes, got_lookup = r.read_nodes(), r.read_tri_lookup()
        bad = np.nonzero((qc.bits(got_nodes) != qc.bits(want_nodes)).any(axis=1))[0]
        assert bad.size == 0, "rebuild: nodes %s differ from the host model" % bad[:8]
        assert np.array_equal(qc.bits(got_lookup), qc.bits(want_lookup))
        nodes_py, lookup_py, tree = builder_arrays(before["triangles"], root, 0)
        if name == "scale+60":
            assert used == [1] and tree.used == 3 and got_nodes[root, 7] == 87
        else:
            assert used == [tree.used]
            assert np.array_equal(qc.bits(got_nodes[root:root + tree.used]), qc.bits(nodes_py)), "the device build and the Python builder part"
            assert np.array_equal(canonical(got_lookup, got_nodes, root), canonical(lookup_py, got_nodes, root))
        c.buf = tri_buffers(c.scene, c.mat)                                        # the scene holds the device's bytes now
        assert np.array_equal(qc.bits(c.buf["nodes"]), qc.bits(got_nodes))
        ref, _, rays = oracle.render_tri(c.scene.pack_params(2), c.buf, SKY.faces, W, H)
        r.render()
        img = r.read_pixels()
        assert np.array_equal(img, ref), diff_stats(img, ref)
        assert r.stats()["rays"] == rays
        t_ref = oracle.trace_tri_rays(c.buf, c.o, c.d)
        assert np.array_equal(qc.bits(r.trace_rays(c.o, c.d)["t"]), qc.bits(t_ref))
    finally:
        r.close()
