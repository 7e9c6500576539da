// rt_blas_build.h -- the SAH builder of acceleration/bvh.py (build_tree) as plain float32 / float64 arithmetic: the pieces the device
// build (rt_build.hip) and the host model (rt_build_blas_host) both call, and the serial driver of the model beside them.
// No HIP needed: tests/c/blas_build_test.cpp compiles it with g++ under ASan + UBSan (tests/test_build_blas_sanitizers_cpu.py).
//
// What build_tree computes is a pure function of float32 data:
//   * a triangle's box is the float32 min / max of its three corners, its centroid ((c0 + c1 -> f32) + c2 -> f32) / 3 -> f32
//     (soup.py forms each step in float64 and rounds: innocuous double rounding, 53 >= 2 * 24 + 2, so plain float32 add / divide);
//   * candidate plane s of 9 on an axis is a (1 - s/10) + b (s/10) in float64, a / b the node's box on that axis;
//   * a triangle goes left when its centroid (as float64) is < the plane; each side's box is the fminf / fmaxf of its triangles'
//     boxes from +-(float)1e30, which does not depend on the order they are met in;
//   * a side's area is 2 (ex ey + ey ez + ez ex), extents float32, products and sums float64, in that order;
//   * cost = areaL nL + areaR nR in float64; the FIRST strict minimum in (axis, plane) order below 1e30 wins; the node stays a
//     leaf when it has fewer than two triangles, when staying is cheaper (area * count < best) or when one side would be empty.
//     (One departure: when NO cost is below 1e30 -- boxes some 1e14 wide, or non-finite -- build_tree sweeps by plane 0.0 of axis
//     0; here the node stays a leaf.)
// The one sequential thing in build_tree is its two-pointer sweep, and only the order of the slots inside a leaf depends on it:
// the boxes, counts and numbering are functions of the SETS.  Here a split is a STABLE partition (left ones first, each side in
// its previous order), so a leaf keeps its slots in the order they had before the build.
// Everything must be compiled without FMA contraction (-ffp-contract=off): the plane, the area and the cost are sums of products.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rt355.h"

#if defined(__HIPCC__)
#define RT_BB_HD __host__ __device__
#else
#define RT_BB_HD
#endif

constexpr uint32_t kBbPlanes = 27u;          // 3 axes x 9 planes, axis-major
constexpr float kBbHuge = 1e30f;             // bvh.py: _F32_HUGE

struct RtBbPrim {                            // 40 bytes per lookup slot
    float lo[3], hi[3], cen[3];
    float raw;                               // the slot's lookup word as it was written (carried, never re-derived)
};
struct RtBbSide { float lo[3], hi[3]; uint32_t n; };
struct RtBbChoice { double best, plane; uint32_t axis, index; };      // index: which of the 27 (kBbPlanes: none was below 1e30)

RT_BB_HD inline uint32_t rt_bb_u32f(float f) {             // WGSL u32(f32): truncating, saturating, NaN -> 0
    if (!(f > 0.0f)) return 0u;
    return f >= 4294967040.0f ? 4294967295u : (uint32_t)f;
}
RT_BB_HD inline float rt_bb_centroid(float a, float b, float c) { return ((a + b) + c) / 3.0f; }

// the slot's triangle: corners at floats 0, 12 and 24 of a 40-float record
RT_BB_HD inline void rt_bb_prim(const float* tri, float raw, RtBbPrim& p) {
    for (int a = 0; a < 3; ++a) {
        const float c0 = tri[a], c1 = tri[12 + a], c2 = tri[24 + a];
        p.lo[a] = fminf(fminf(c0, c1), c2);
        p.hi[a] = fmaxf(fmaxf(c0, c1), c2);
        p.cen[a] = rt_bb_centroid(c0, c1, c2);
    }
    p.raw = raw;
}
RT_BB_HD inline void rt_bb_side_clear(RtBbSide& s) {
    for (int a = 0; a < 3; ++a) { s.lo[a] = kBbHuge; s.hi[a] = -kBbHuge; }
    s.n = 0u;
}
RT_BB_HD inline void rt_bb_side_add(RtBbSide& s, const float* lo, const float* hi, uint32_t n) {
    for (int a = 0; a < 3; ++a) { s.lo[a] = fminf(s.lo[a], lo[a]); s.hi[a] = fmaxf(s.hi[a], hi[a]); }
    s.n += n;
}
RT_BB_HD inline double rt_bb_plane(float a, float b, uint32_t s) {     // s in 1 .. 9
    const double f = (double)s / 10.0;
    return (double)a * (1.0 - f) + (double)b * f;
}
RT_BB_HD inline uint32_t rt_bb_axis_of(uint32_t index) { return index / 9u; }
RT_BB_HD inline double rt_bb_plane_of(const float* lo, const float* hi, uint32_t index) {
    return rt_bb_plane(lo[index / 9u], hi[index / 9u], index % 9u + 1u);
}
RT_BB_HD inline bool rt_bb_goes_left(const RtBbPrim& p, uint32_t axis, double plane) { return (double)p.cen[axis] < plane; }
RT_BB_HD inline double rt_bb_area(const float* lo, const float* hi) {
    const double ex = (double)(hi[0] - lo[0]), ey = (double)(hi[1] - lo[1]), ez = (double)(hi[2] - lo[2]);
    return 2.0 * (ex * ey + ey * ez + ez * ex);
}
RT_BB_HD inline double rt_bb_cost(const RtBbSide& l, const RtBbSide& r) {
    return (0.0 + rt_bb_area(l.lo, l.hi) * (double)l.n) + rt_bb_area(r.lo, r.hi) * (double)r.n;
}
RT_BB_HD inline RtBbChoice rt_bb_choose(const double* cost, const float* lo, const float* hi) {
    RtBbChoice c;
    c.best = 1e30; c.plane = 0.0; c.axis = 0u; c.index = kBbPlanes;
    for (uint32_t i = 0; i < kBbPlanes; ++i)
        if (cost[i] < c.best) { c.best = cost[i]; c.index = i; c.axis = rt_bb_axis_of(i); c.plane = rt_bb_plane_of(lo, hi, i); }
    return c;
}
// n_left: triangles left of the chosen plane
RT_BB_HD inline bool rt_bb_is_leaf(uint32_t count, const float* lo, const float* hi, const RtBbChoice& c, uint32_t n_left) {
    const double best = c.best;
    if (count < 2u || c.index >= kBbPlanes) return true;
    if (rt_bb_area(lo, hi) * (double)count < best) return true;
    return n_left == 0u || n_left == count;
}

// ---- the ranges of a call: rt_build_blas and rt_build_blas_host refuse the same ones -------------------------------------------
inline const char* rt_bb_check_ranges(const rt_blas_range* r, uint32_t n, uint32_t n_nodes, uint32_t n_slots) {
    for (uint32_t i = 0; i < n; ++i) {
        if (r[i].n_slots == 0u) return "a range of no slots";
        if (r[i].node_cap == 0u) return "a range of no nodes";
        if (r[i].root_node == 0u) return "a range that covers node 0";
        if ((uint64_t)r[i].root_node + r[i].node_cap > n_nodes) return "a range beyond the nodes written";
        if ((uint64_t)r[i].first_slot + r[i].n_slots > n_slots) return "a range beyond the lookup slots written";
    }
    std::vector<uint32_t> by(n);
    for (uint32_t i = 0; i < n; ++i) by[i] = i;
    std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return r[a].root_node < r[b].root_node; });
    for (uint32_t i = 1; i < n; ++i)
        if ((uint64_t)r[by[i - 1u]].root_node + r[by[i - 1u]].node_cap > r[by[i]].root_node) return "two ranges overlap in nodes";
    std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return r[a].first_slot < r[b].first_slot; });
    for (uint32_t i = 1; i < n; ++i)
        if ((uint64_t)r[by[i - 1u]].first_slot + r[by[i - 1u]].n_slots > r[by[i]].first_slot) return "two ranges overlap in lookup slots";
    return nullptr;
}

// ---- the model: one tree, serially, numbered as build_tree numbers it (an explicit stack, the left subtree first) ---------------
// prims: one per slot of the range, in slot order.  nodes: (used, 8) float32 records with child indices rebased by `root_node`
// and leaf runs by `first_slot`; order: per slot of the range, which of `prims` ends up there.
inline void rt_bb_build_tree(const std::vector<RtBbPrim>& prims, uint32_t root_node, uint32_t first_slot,
                             std::vector<float>& nodes, std::vector<uint32_t>& order) {
    const uint32_t n = (uint32_t)prims.size();
    order.resize(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    nodes.assign(8u, 0.0f);
    struct Node { uint32_t first, count; };
    std::vector<Node> meta(1, Node{0u, n});
    {
        RtBbSide s;
        rt_bb_side_clear(s);
        for (const RtBbPrim& p : prims) rt_bb_side_add(s, p.lo, p.hi, 1u);
        std::memcpy(&nodes[0], s.lo, 12); std::memcpy(&nodes[4], s.hi, 12);
    }
    std::vector<uint32_t> todo(1, 0u), tmp;
    while (!todo.empty()) {
        const uint32_t node = todo.back();
        todo.pop_back();
        const uint32_t first = meta[node].first, count = meta[node].count;
        float lo[3], hi[3];
        std::memcpy(lo, &nodes[8u * (size_t)node], 12); std::memcpy(hi, &nodes[8u * (size_t)node + 4u], 12);
        bool leaf = count < 2u;
        RtBbSide l[kBbPlanes], r[kBbPlanes];
        RtBbChoice c = {};
        uint32_t n_left = 0u;
        if (!leaf) {
            double cost[kBbPlanes];
            for (uint32_t i = 0; i < kBbPlanes; ++i) {
                const uint32_t axis = rt_bb_axis_of(i);
                const double plane = rt_bb_plane_of(lo, hi, i);
                rt_bb_side_clear(l[i]); rt_bb_side_clear(r[i]);
                for (uint32_t k = 0; k < count; ++k) {
                    const RtBbPrim& p = prims[order[first + k]];
                    rt_bb_side_add(rt_bb_goes_left(p, axis, plane) ? l[i] : r[i], p.lo, p.hi, 1u);
                }
                cost[i] = rt_bb_cost(l[i], r[i]);
            }
            c = rt_bb_choose(cost, lo, hi);
            if (c.index < kBbPlanes) n_left = l[c.index].n;
            leaf = rt_bb_is_leaf(count, lo, hi, c, n_left);
        }
        float* rec = &nodes[8u * (size_t)node];
        if (leaf) { rec[3] = (float)(first_slot + first); rec[7] = (float)count; continue; }
        const RtBbSide &sl = l[c.index], &sr = r[c.index];         // the children's boxes: the winning plane's two sides
        tmp.assign(order.begin() + first, order.begin() + first + count);
        uint32_t a = first, b = first + n_left;
        for (uint32_t id : tmp)
            order[rt_bb_goes_left(prims[id], c.axis, c.plane) ? a++ : b++] = id;
        const uint32_t child = (uint32_t)meta.size();
        rec[3] = (float)(root_node + child); rec[7] = 0.0f;
        meta.push_back(Node{first, n_left});
        meta.push_back(Node{first + n_left, count - n_left});
        nodes.resize(nodes.size() + 16u, 0.0f);
        float* cl = &nodes[8u * (size_t)child];
        std::memcpy(cl, sl.lo, 12); std::memcpy(cl + 4, sl.hi, 12);
        std::memcpy(cl + 8, sr.lo, 12); std::memcpy(cl + 12, sr.hi, 12);
        todo.push_back(child + 1u);
        todo.push_back(child);
    }
}

// The whole call on caller arrays, in place: the checks of rt_build_blas, every tree built aside, and only then -- when each fits
// its node_cap -- the records and the permuted lookup words stored.  Returns an rt_status; *why names a refusal.
inline int rt_bb_build_host(const float* triangles, uint32_t n_triangles, float* tri_lookup, uint32_t n_tri_lookup, float* nodes,
                            uint32_t n_nodes, const rt_blas_range* ranges, uint32_t n, uint32_t* used, const char** why) {
    *why = "";
    if (!ranges && n) { *why = "NULL ranges"; return RT_ERR_INVALID_ARG; }
    if (!triangles || !n_triangles || !tri_lookup || !n_tri_lookup || !nodes || !n_nodes) { *why = "no triangle scene"; return RT_ERR_STATE; }
    if (n == 0u) return RT_OK;
    if (const char* bad = rt_bb_check_ranges(ranges, n, n_nodes, n_tri_lookup)) { *why = bad; return RT_ERR_INVALID_ARG; }
    std::vector<std::vector<float>> recs(n);
    std::vector<std::vector<float>> words(n);
    bool fits = true;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_blas_range& g = ranges[i];
        std::vector<RtBbPrim> prims(g.n_slots);
        for (uint32_t k = 0; k < g.n_slots; ++k) {
            const float raw = tri_lookup[g.first_slot + k];
            uint32_t ti = rt_bb_u32f(raw);
            if (ti >= n_triangles) ti = n_triangles - 1u;
            rt_bb_prim(triangles + 40u * (size_t)ti, raw, prims[k]);
        }
        std::vector<uint32_t> order;
        rt_bb_build_tree(prims, g.root_node, g.first_slot, recs[i], order);
        words[i].resize(g.n_slots);
        for (uint32_t k = 0; k < g.n_slots; ++k) words[i][k] = prims[order[k]].raw;
        const uint32_t u = (uint32_t)(recs[i].size() / 8u);
        if (used) used[i] = u;
        if (u > g.node_cap) fits = false;
    }
    if (!fits) { *why = "a tree needs more nodes than its node_cap"; return RT_ERR_CAPACITY; }
    for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(nodes + 8u * (size_t)ranges[i].root_node, recs[i].data(), recs[i].size() * 4u);
        std::memcpy(tri_lookup + ranges[i].first_slot, words[i].data(), words[i].size() * 4u);
    }
    return RT_OK;
}
