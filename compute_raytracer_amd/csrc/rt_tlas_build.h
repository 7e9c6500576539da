// rt_tlas_build.h -- the top level over tight instance boxes (include/rt355.h: rt_build_tlas) as plain float32 / float64
// arithmetic: the pieces the device build (rt_tlas.hip) and the host model (rt_build_tlas_host) both call, the argument checks
// they share and the serial driver of the model.  No HIP needed: tests/c/tlas_build_test.cpp compiles it with g++ under ASan +
// UBSan (tests/test_build_tlas_sanitizers_cpu.py).
//
// What is computed is a pure function of float32 data, restated from instances.py:
//   * BLAS record i = {invert(models[i]), (float)roots[i], 0, 0, 0}; invert is invert_mat4: the float32 inputs as float64, the
//     twelve 2 x 2 minors, the determinant and the sixteen cofactors in that function's expression order, each cofactor times
//     1 / det, ONE rounding to float32; det == 0 (and only that: a NaN determinant gives NaNs) gives the identity;
//   * world box of instance i = world_boxes on the node record at roots[i]: each of its eight corners (x: bit 2, y: bit 1,
//     z: bit 0 takes max) through models[i], products and sums left to right in float64, w = m3 x + m7 y + m11 z + m15 with the
//     `w || 1` rule (0 and NaN -> 1), the division, one rounding to float32, fminf / fmaxf from +-(float)1e30;
//   * the pad: m = the largest |bound| of the six, pad = m * 2^-16 in float32, lo - pad and hi + pad in float32.  Without it rays
//     grazing a zero-height box (a flat floor) lose hits: the instance's box test runs in world space, the triangle test in the
//     instance's space, and the two round differently (DESIGN.md 4.7i has the counts);
//   * centroid = (lo + hi) * 0.5f of the padded bounds; raw = (float)i.
// The tree over these primitives is rt_blas_build.h's (rt_bb_build_tree), rooted at node 0 with first slot 0.
// Everything must be compiled without FMA contraction (-ffp-contract=off).
#pragma once
#include "rt_blas_build.h"

constexpr uint32_t kTlMaxInstances = 1u << 20;
constexpr uint32_t kTlMaxDepth = 20u;        // the walks keep twenty stack slots, nearer-child-first needs one per level (rt_tlas_fit.h)

// out = invert_mat4(m), column-major 4 x 4
RT_BB_HD inline void rt_tl_invert(const float* m, float* out) {
    double a[16];
    for (int i = 0; i < 16; ++i) a[i] = (double)m[i];
    const double b00 = a[0] * a[5] - a[1] * a[4], b01 = a[0] * a[6] - a[2] * a[4];
    const double b02 = a[0] * a[7] - a[3] * a[4], b03 = a[1] * a[6] - a[2] * a[5];
    const double b04 = a[1] * a[7] - a[3] * a[5], b05 = a[2] * a[7] - a[3] * a[6];
    const double b06 = a[8] * a[13] - a[9] * a[12], b07 = a[8] * a[14] - a[10] * a[12];
    const double b08 = a[8] * a[15] - a[11] * a[12], b09 = a[9] * a[14] - a[10] * a[13];
    const double b10 = a[9] * a[15] - a[11] * a[13], b11 = a[10] * a[15] - a[11] * a[14];
    const double det = b00 * b11 - b01 * b10 + b02 * b09 + b03 * b08 - b04 * b07 + b05 * b06;
    if (det == 0.0) {
        for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        return;
    }
    const double inv = 1.0 / det;
    const double cof[16] = {
        a[5] * b11 - a[6] * b10 + a[7] * b09,    a[2] * b10 - a[1] * b11 - a[3] * b09,
        a[13] * b05 - a[14] * b04 + a[15] * b03, a[10] * b04 - a[9] * b05 - a[11] * b03,
        a[6] * b08 - a[4] * b11 - a[7] * b07,    a[0] * b11 - a[2] * b08 + a[3] * b07,
        a[14] * b02 - a[12] * b05 - a[15] * b01, a[8] * b05 - a[10] * b02 + a[11] * b01,
        a[4] * b10 - a[5] * b08 + a[7] * b06,    a[1] * b08 - a[0] * b10 - a[3] * b06,
        a[12] * b04 - a[13] * b02 + a[15] * b00, a[9] * b02 - a[8] * b04 - a[11] * b00,
        a[5] * b07 - a[4] * b09 - a[6] * b06,    a[0] * b09 - a[1] * b07 + a[2] * b06,
        a[13] * b01 - a[12] * b03 - a[14] * b00, a[8] * b03 - a[9] * b01 + a[10] * b00};
    for (int i = 0; i < 16; ++i) out[i] = (float)(cof[i] * inv);
}

// rec: the eight floats of the node record at the instance's root {min.xyz, -, max.xyz, -}
RT_BB_HD inline void rt_tl_world_box(const float* m, const float* rec, float* lo, float* hi) {
    double a[16];
    for (int i = 0; i < 16; ++i) a[i] = (double)m[i];
    for (int k = 0; k < 3; ++k) { lo[k] = kBbHuge; hi[k] = -kBbHuge; }
    for (int c = 0; c < 8; ++c) {
        const double px = (double)rec[(c & 4) ? 4 : 0], py = (double)rec[(c & 2) ? 5 : 1], pz = (double)rec[(c & 1) ? 6 : 2];
        double w = a[3] * px + a[7] * py + a[11] * pz + a[15];
        if (w == 0.0 || w != w) w = 1.0;
        for (int k = 0; k < 3; ++k) {
            const float q = (float)((a[k] * px + a[4 + k] * py + a[8 + k] * pz + a[12 + k]) / w);
            lo[k] = fminf(lo[k], q);
            hi[k] = fmaxf(hi[k], q);
        }
    }
}

RT_BB_HD inline void rt_tl_pad(float* lo, float* hi) {
    float m = 0.0f;
    for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
    const float pad = m * 1.52587890625e-05f;                  // 2^-16
    for (int k = 0; k < 3; ++k) { lo[k] = lo[k] - pad; hi[k] = hi[k] + pad; }
}

// instance i as a primitive of the builder
RT_BB_HD inline void rt_tl_prim(const float* m, const float* rec, uint32_t i, RtBbPrim& p) {
    rt_tl_world_box(m, rec, p.lo, p.hi);
    rt_tl_pad(p.lo, p.hi);
    for (int k = 0; k < 3; ++k) p.cen[k] = (p.lo[k] + p.hi[k]) * 0.5f;
    p.raw = (float)i;
}

RT_BB_HD inline void rt_tl_record(const float* m, uint32_t root, float* rec20) {
    rt_tl_invert(m, rec20);
    rec20[16] = (float)root;
    rec20[17] = rec20[18] = rec20[19] = 0.0f;
}

// ---- the arguments of a call: rt_build_tlas and rt_build_tlas_host refuse the same ones ------------------------------------------
inline const char* rt_tl_check_args(const uint32_t* roots, uint32_t n, uint32_t node_cap, uint32_t n_nodes) {
    if (n == 0u) return "no instances";
    if (n > kTlMaxInstances) return "more than 2^20 instances";
    if (node_cap > n_nodes) return "node_cap beyond the nodes written";
    for (uint32_t i = 0; i < n; ++i) {
        if (roots[i] >= n_nodes) return "a root beyond the nodes written";
        if (roots[i] < node_cap) return "a root inside the top level's nodes";
    }
    return nullptr;
}

// what the tree in `nodes` (used records, root 0, as rt_bb_build_tree numbers them) looks like
inline rt_tlas_info rt_tl_info(const float* nodes, uint32_t used) {
    rt_tlas_info info = {used, 0u, 0u, 0u};
    struct Item { uint32_t i, depth; };
    std::vector<Item> todo(1, Item{0u, 0u});
    uint32_t visited = 0u;
    while (!todo.empty() && visited < used) {                  // (a well-formed tree visits each node once)
        const Item it = todo.back();
        todo.pop_back();
        if (it.i >= used) continue;
        ++visited;
        const float* p = nodes + 8u * (size_t)it.i;
        const uint32_t count = rt_bb_u32f(p[7]);
        info.depth = std::max(info.depth, it.depth);
        if (count != 0u) { ++info.leaves; info.max_leaf = std::max(info.max_leaf, count); continue; }
        const uint32_t left = rt_bb_u32f(p[3]);
        if (left >= used - 1u && used >= 1u) continue;
        todo.push_back(Item{left + 1u, it.depth + 1u});
        todo.push_back(Item{left, it.depth + 1u});
    }
    return info;
}

// What a finished tree may be committed as: RT_OK, RT_ERR_CAPACITY or RT_ERR_UNSUPPORTED (the two entry points decide alike)
inline int rt_tl_verdict(const rt_tlas_info& info, uint32_t node_cap, const char** why) {
    if (info.nodes_used > node_cap) { *why = "the tree needs more nodes than node_cap"; return RT_ERR_CAPACITY; }
    if (info.depth > kTlMaxDepth) { *why = "the tree is deeper than twenty levels"; return RT_ERR_UNSUPPORTED; }
    return RT_OK;
}

// ---- the model: the whole call on caller arrays, serially.  Nothing is stored unless the call succeeds. ---------------------------
inline int rt_tl_build_host(const float* models, const uint32_t* roots, uint32_t n, const float* nodes, uint32_t n_nodes,
                            float* tlas_nodes, float* blas, float* blas_lookup, uint32_t node_cap, rt_tlas_info* info, const char** why) {
    *why = "";
    if (!models || !roots || !nodes || !tlas_nodes || !blas || !blas_lookup) { *why = "NULL argument"; return RT_ERR_INVALID_ARG; }
    if (const char* bad = rt_tl_check_args(roots, n, node_cap, n_nodes)) { *why = bad; return RT_ERR_INVALID_ARG; }
    std::vector<RtBbPrim> prims(n);
    for (uint32_t i = 0; i < n; ++i) rt_tl_prim(models + 16u * (size_t)i, nodes + 8u * (size_t)roots[i], i, prims[i]);
    std::vector<float> recs;
    std::vector<uint32_t> order;
    rt_bb_build_tree(prims, 0u, 0u, recs, order);
    const rt_tlas_info got = rt_tl_info(recs.data(), (uint32_t)(recs.size() / 8u));
    if (info) *info = got;
    { const int rc = rt_tl_verdict(got, node_cap, why); if (rc != RT_OK) return rc; }
    std::memset(tlas_nodes, 0, (size_t)node_cap * 32u);
    std::memcpy(tlas_nodes, recs.data(), recs.size() * 4u);
    for (uint32_t i = 0; i < n; ++i) {
        rt_tl_record(models + 16u * (size_t)i, roots[i], blas + 20u * (size_t)i);
        blas_lookup[i] = prims[order[i]].raw;
    }
    return RT_OK;
}
