// rt_closest.h -- the arithmetic, the walk and the serial model behind rt_closest_points / rt_closest_points_model -- under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_closest_sanitizers_cpu.py).
//   1. argv[1]: a scene file the driver wrote -- six counts {points, triangles, lookup slots, nodes, BLAS records, BLAS lookup} as
//      u32, then the points (4 floats each), the five scene arrays in that order and the records the numpy brute force expects
//      (32 bytes each).  The model must give those bytes, with and without a mask table, and count its candidate tests.
//   2. hand-made trees deeper than the stacks: a bottom-level spine of 40 levels and a top-level spine of 25, searched from both
//      ends with every radius -- the pushes the stacks cannot hold are dropped; every record must be a true candidate (its dist2 is
//      the leaf function's for the pair it names) and, from the end where nothing is dropped, the nearest one.
//   3. indices beyond every array (they clamp) and garbage floats in boxes, records and points: no bad access, no UB.
//   4. the bad arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../compute_raytracer_amd/csrc/rt_closest.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

struct Scene {
    std::vector<float> triangles, tri_lookup, nodes, blas, blas_lookup;
};

static int run(const Scene& s, const std::vector<float>& points, const std::vector<uint32_t>& masks, uint32_t ray_mask,
               std::vector<rt_closest>& out, uint64_t* tests) {
    const uint32_t n = (uint32_t)(points.size() / 4u);
    out.resize(n + 1u);
    std::memset(out.data(), 0x5A, out.size() * sizeof(rt_closest));
    const char* why = "";
    const int rc = rt_cp_model(points.data(), n, s.triangles.data(), (uint32_t)(s.triangles.size() / 40u), s.tri_lookup.data(),
                               (uint32_t)s.tri_lookup.size(), s.nodes.data(), (uint32_t)(s.nodes.size() / 8u), s.blas.data(),
                               (uint32_t)(s.blas.size() / 20u), s.blas_lookup.data(), (uint32_t)s.blas_lookup.size(),
                               masks.empty() ? nullptr : masks.data(), (uint32_t)masks.size(), ray_mask, out.data(), tests, &why);
    unsigned char guard[sizeof(rt_closest)];
    std::memset(guard, 0x5A, sizeof guard);
    CHECK(std::memcmp(&out[n], guard, sizeof guard) == 0, "the record behind the last one was written");
    return rc;
}

static void node(Scene& s, uint32_t i, float lo, float hi, float left, float count) {
    if (s.nodes.size() < 8u * (size_t)(i + 1u)) s.nodes.resize(8u * (size_t)(i + 1u), 0.0f);
    float* p = &s.nodes[8u * (size_t)i];
    p[0] = lo; p[1] = -1.0f; p[2] = -1.0f; p[3] = left;
    p[4] = hi; p[5] = 1.0f; p[6] = 1.0f; p[7] = count;
}

static void identity_record(Scene& s, float tx, float root) {
    float r[20] = {0};
    r[0] = r[5] = r[10] = r[15] = 1.0f;
    r[12] = -tx;                                                     // the record is the INVERSE model: world -> object
    r[16] = root;
    s.blas.insert(s.blas.end(), r, r + 20);
}

// triangle k of the spine: in the plane x = k, within y, z in [-1, 1]
static void spine_triangle(Scene& s, uint32_t k) {
    float t[40] = {0};
    t[0] = (float)k; t[1] = -1.0f; t[2] = -1.0f;
    t[12] = (float)k; t[13] = 1.0f; t[14] = -1.0f;
    t[24] = (float)k; t[25] = 0.0f; t[26] = 1.0f;
    s.triangles.insert(s.triangles.end(), t, t + 40);
    s.tri_lookup.push_back((float)k);
}

// a bottom-level spine of `depth` leaves from node `first`: inner node i has the leaf of triangle i and the rest of the spine
static void bottom_spine(Scene& s, uint32_t first, uint32_t depth) {
    for (uint32_t k = 0; k < depth; ++k) spine_triangle(s, k);
    uint32_t at = first;
    for (uint32_t k = 0; k + 1u < depth; ++k) {
        node(s, at, (float)k, (float)(depth - 1u), (float)(at + 1u), 0.0f);
        node(s, at + 1u, (float)k, (float)k, (float)k, 1.0f);
        at += 2u;
    }
    node(s, at, (float)(depth - 1u), (float)(depth - 1u), (float)(depth - 1u), 1.0f);
}

static bool true_candidate(const Scene& s, const float* p, const rt_closest& r) {
    if (r.prim < 0) return r.instance == -1 && r.dist2 == -1.0f;
    float w[kCpInstWords];
    RtCpHostScene h;
    std::memset(&h, 0, sizeof h);
    h.nodes = s.nodes.data(); h.n_nodes = (uint32_t)(s.nodes.size() / 8u);
    const float* rec = &s.blas[20u * (size_t)r.instance];
    const RtCpNode root = h.node(rt_bb_u32f(rec[16]));
    rt_cp_inst(rec, root.lo, root.hi, w);
    const float* t = &s.triangles[40u * (size_t)r.prim];
    float A[3], B[3], C[3];
    for (int k = 0; k < 3; ++k) { A[k] = rt_cp_corner(w, t, k); B[k] = rt_cp_corner(w, t + 12, k); C[k] = rt_cp_corner(w, t + 24, k); }
    const RtCpLeaf f = rt_cp_leaf(p, A, B, C);
    return std::memcmp(&f.dist2, &r.dist2, 4) == 0 && std::memcmp(f.point, r.point, 12) == 0 && f.dist2 <= p[3] * p[3];
}

static void deep_trees() {
    const float inf = std::numeric_limits<float>::infinity();
    // one instance, a bottom-level spine of 40 levels under a one-leaf top level
    Scene s;
    node(s, 0, -1e6f, 1e6f, 0.0f, 1.0f);
    bottom_spine(s, 1, 40);
    identity_record(s, 0.0f, 1.0f);
    s.blas_lookup.push_back(0.0f);
    const float radii[] = {inf, 200.0f, 0.5f, 0.0f, -1.0f, std::nanf("")};
    for (float radius : radii) {
        // from x = 100 the rest of the spine is always the nearer child: 39 leaves are pushed, the stack holds 32
        const std::vector<float> pts = {100.0f, 0.0f, 0.0f, radius, -100.0f, 0.2f, 0.1f, radius, 39.0f, 0.0f, 0.0f, radius};
        std::vector<rt_closest> out;
        uint64_t tests = 0;
        CHECK(run(s, pts, {}, 0xFFFFFFFFu, out, &tests) == RT_OK, "deep bottom level");
        for (uint32_t i = 0; i < 3u; ++i) CHECK(true_candidate(s, &pts[4u * i], out[i]), "deep bottom level: point %u is no true candidate", i);
        if (radius >= 200.0f) {
            CHECK(out[0].prim == 39 && out[0].dist2 == 61.0f * 61.0f, "from the far end: prim %d dist2 %g", out[0].prim, out[0].dist2);
            CHECK(out[1].prim == 0 && out[2].prim == 39 && out[2].dist2 == 0.0f, "from the near end: prim %d", out[1].prim);
        }
        if (!(radius >= 0.0f)) CHECK(out[0].prim == -1 && out[1].prim == -1 && tests == 0u, "a negative or NaN radius is a miss");
    }
    // 25 instances of a two-level tree along x under a top-level spine of 25 levels
    Scene t;
    const uint32_t n_inst = 25u, top = 2u * n_inst - 1u;
    uint32_t at = 0;
    for (uint32_t k = 0; k + 1u < n_inst; ++k) {
        node(t, at, 10.0f * (float)k - 1.0f, 10.0f * (float)(n_inst - 1u) + 2.0f, (float)(at + 1u), 0.0f);
        node(t, at + 1u, 10.0f * (float)k - 1.0f, 10.0f * (float)k + 2.0f, (float)k, 1.0f);
        at += 2u;
    }
    node(t, at, 10.0f * (float)(n_inst - 1u) - 1.0f, 10.0f * (float)(n_inst - 1u) + 2.0f, (float)(n_inst - 1u), 1.0f);
    bottom_spine(t, top, 2);
    for (uint32_t k = 0; k < n_inst; ++k) { identity_record(t, 10.0f * (float)k, (float)top); t.blas_lookup.push_back((float)k); }
    for (float radius : radii) {
        const std::vector<float> pts = {1000.0f, 0.0f, 0.0f, radius, -1000.0f, 0.0f, 0.0f, radius, 121.0f, 0.3f, 0.0f, radius};
        std::vector<rt_closest> out;
        CHECK(run(t, pts, {}, 0xFFFFFFFFu, out, nullptr) == RT_OK, "deep top level");
        for (uint32_t i = 0; i < 3u; ++i) CHECK(true_candidate(t, &pts[4u * i], out[i]), "deep top level: point %u is no true candidate", i);
        if (radius == inf) CHECK(out[0].instance == 24 && out[0].prim == 1 && out[1].instance == 0 && out[1].prim == 0 && out[2].instance == 12,
                                 "deep top level: instances %d %d %d", out[0].instance, out[1].instance, out[2].instance);
    }
    // masks: only instance 7 is visible
    std::vector<uint32_t> masks(n_inst, 2u);
    masks[7] = 5u;
    std::vector<rt_closest> out;
    CHECK(run(t, {0.0f, 0.0f, 0.0f, inf}, masks, 4u, out, nullptr) == RT_OK && out[0].instance == 7, "masks: instance %d", out[0].instance);
    CHECK(run(t, {0.0f, 0.0f, 0.0f, inf}, masks, 8u, out, nullptr) == RT_OK && out[0].instance == -1 && out[0].dist2 == -1.0f, "a mask that hides all");
}

static void garbage() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const float junk[] = {nan, inf, -inf, 3e38f, -3e38f, 1e-45f, 0.0f, -0.0f, 4294967296.0f, -5.0f};
    const uint32_t n_junk = (uint32_t)(sizeof junk / sizeof junk[0]);
    uint32_t seed = 12345u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 200; ++round) {
        Scene s;
        node(s, 0, -1e6f, 1e6f, 1.0f, 0.0f);
        node(s, 1, -1e6f, 1e6f, 0.0f, 1.0f);
        node(s, 2, -1e6f, 1e6f, 1.0f, 1.0f);
        bottom_spine(s, 3, 6);
        identity_record(s, 0.0f, 3.0f);
        identity_record(s, 3.0f, 3.0f);
        s.blas_lookup = {0.0f, 1.0f};
        std::vector<float> pts = {0.5f, 0.1f, 0.2f, inf, 7.0f, 0.0f, 0.0f, 2.0f};
        switch (round % 5) {
        case 0: for (int k = 0; k < 6; ++k) { const uint32_t i = next() % (uint32_t)(s.nodes.size() / 8u); s.nodes[8u * i + (next() % 3u) + 4u * (next() % 2u)] = junk[next() % n_junk]; } break;
        case 1: for (int k = 0; k < 6; ++k) s.blas[next() % 16u + 20u * (next() % 2u)] = junk[next() % n_junk]; break;
        case 2: for (int k = 0; k < 4; ++k) pts[next() % 8u] = junk[next() % n_junk]; break;
        case 3: for (int k = 0; k < 6; ++k) s.triangles[40u * (next() % 6u) + 12u * (next() % 3u) + next() % 3u] = junk[next() % n_junk]; break;
        default:
            // indices beyond every array: leaves (their runs and lookup positions), lookup words, roots -- they clamp; the last node
            // is a leaf, so every walk ends
            s.blas_lookup[next() % 2u] = junk[next() % n_junk];
            s.tri_lookup[next() % 6u] = junk[next() % n_junk];
            s.blas[16u + 20u * (next() % 2u)] = (next() % 2u) ? 1e9f : junk[next() % n_junk];
            s.nodes[8u * 1u + 3u] = (float)(next() % 5u);
            s.nodes[8u * 13u + 3u] = 4.0f; s.nodes[8u * 13u + 7u] = 9.0f;     // the last leaf's run passes the end of the lookup table
            break;
        }
        std::vector<rt_closest> out;
        uint64_t tests = 0;
        CHECK(run(s, pts, {}, 0xFFFFFFFFu, out, &tests) == RT_OK, "garbage round %d", round);
        for (uint32_t i = 0; i < 2u; ++i)
            CHECK((out[i].prim == -1 && out[i].instance == -1 && out[i].dist2 == -1.0f) || (out[i].prim >= 0 && out[i].prim < 6 && out[i].instance >= 0 &&
                   out[i].instance < 2 && out[i].dist2 >= 0.0f), "garbage round %d: record %u {%g, %d, %d}", round, i, out[i].dist2, out[i].prim, out[i].instance);
    }
}

static void bad_arguments() {
    Scene s;
    node(s, 0, -1e6f, 1e6f, 0.0f, 1.0f);
    bottom_spine(s, 1, 2);
    identity_record(s, 0.0f, 1.0f);
    s.blas_lookup.push_back(0.0f);
    const float p[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    rt_closest out;
    const char* why = "";
    uint64_t tests = 77u;
    auto call = [&](const float* pts, uint32_t n, const float* tri, uint32_t n_tri, const float* nodes, uint32_t n_nodes, const uint32_t* masks,
                    uint32_t n_masks, rt_closest* o) {
        return rt_cp_model(pts, n, tri, n_tri, s.tri_lookup.data(), (uint32_t)s.tri_lookup.size(), nodes, n_nodes, s.blas.data(), 1u,
                           s.blas_lookup.data(), 1u, masks, n_masks, 0xFFFFFFFFu, o, &tests, &why);
    };
    const uint32_t n_nodes = (uint32_t)(s.nodes.size() / 8u);
    CHECK(call(p, 1u, s.triangles.data(), 2u, s.nodes.data(), n_nodes, nullptr, 0u, &out) == RT_OK && tests == 1u && out.prim == 0,
          "the good call: %llu tests (the second leaf is a unit away and is skipped when it is popped)", (unsigned long long)tests);
    CHECK(call(nullptr, 0u, nullptr, 0u, nullptr, 0u, nullptr, 0u, nullptr) == RT_OK && tests == 0u, "n == 0");
    CHECK(call(nullptr, 1u, s.triangles.data(), 2u, s.nodes.data(), n_nodes, nullptr, 0u, &out) == RT_ERR_INVALID_ARG, "NULL points");
    CHECK(call(p, 1u, s.triangles.data(), 2u, s.nodes.data(), n_nodes, nullptr, 0u, nullptr) == RT_ERR_INVALID_ARG, "NULL out");
    CHECK(call(p, 1u, nullptr, 2u, s.nodes.data(), n_nodes, nullptr, 0u, &out) == RT_ERR_INVALID_ARG, "NULL triangles");
    CHECK(call(p, 1u, s.triangles.data(), 2u, nullptr, n_nodes, nullptr, 0u, &out) == RT_ERR_INVALID_ARG, "NULL nodes");
    CHECK(call(p, 1u, s.triangles.data(), 2u, s.nodes.data(), n_nodes, nullptr, 3u, &out) == RT_ERR_INVALID_ARG, "NULL masks with a count");
    CHECK(call(p, 1u, s.triangles.data(), 0u, s.nodes.data(), n_nodes, nullptr, 0u, &out) == RT_ERR_STATE, "no triangles");
    CHECK(call(p, 1u, s.triangles.data(), 2u, s.nodes.data(), 0u, nullptr, 0u, &out) == RT_ERR_STATE, "no nodes");
}

static bool read_all(std::FILE* f, void* dst, size_t bytes) { return bytes == 0u || std::fread(dst, 1, bytes, f) == bytes; }

static void scene_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    uint32_t c[6];
    Scene s;
    std::vector<float> pts;
    std::vector<rt_closest> want;
    bool ok = read_all(f, c, sizeof c);
    if (ok) {
        pts.resize(4u * (size_t)c[0]); s.triangles.resize(40u * (size_t)c[1]); s.tri_lookup.resize(c[2]); s.nodes.resize(8u * (size_t)c[3]);
        s.blas.resize(20u * (size_t)c[4]); s.blas_lookup.resize(c[5]); want.resize(c[0]);
        ok = read_all(f, pts.data(), pts.size() * 4u) && read_all(f, s.triangles.data(), s.triangles.size() * 4u) &&
             read_all(f, s.tri_lookup.data(), s.tri_lookup.size() * 4u) && read_all(f, s.nodes.data(), s.nodes.size() * 4u) &&
             read_all(f, s.blas.data(), s.blas.size() * 4u) && read_all(f, s.blas_lookup.data(), s.blas_lookup.size() * 4u) &&
             read_all(f, want.data(), want.size() * sizeof(rt_closest));
    }
    std::fclose(f);
    CHECK(ok && c[0] > 0u, "short scene file");
    if (!ok) return;
    std::vector<rt_closest> out;
    uint64_t tests = 0;
    CHECK(run(s, pts, {}, 0xFFFFFFFFu, out, &tests) == RT_OK, "the scene file");
    uint32_t bad = 0;
    for (uint32_t i = 0; i < c[0]; ++i) bad += std::memcmp(&out[i], &want[i], sizeof(rt_closest)) != 0 ? 1u : 0u;
    CHECK(bad == 0u, "%u of %u records differ from the brute force", bad, c[0]);
    CHECK(tests > 0u, "no candidate was tested");
    std::vector<uint32_t> masks(c[4], 0xFFFFFFFFu);
    std::vector<rt_closest> again;
    CHECK(run(s, pts, masks, 1u, again, nullptr) == RT_OK && std::memcmp(out.data(), again.data(), c[0] * sizeof(rt_closest)) == 0, "a table of all ones changes nothing");
    std::printf("scene file: %u points, %llu candidate tests\n", c[0], (unsigned long long)tests);
}

int main(int argc, char** argv) {
    static_assert(sizeof(rt_closest) == 32, "rt_closest is 32 bytes");
    if (argc > 1) scene_file(argv[1]);
    deep_trees();
    garbage();
    bad_arguments();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("closest ok\n");
    return 0;
}
