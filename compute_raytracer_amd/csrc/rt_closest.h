// rt_closest.h -- closest-point queries (include/rt355.h: rt_closest_points) as plain float32 / float64 arithmetic: the leaf
// function, the per-instance constants, the lower bounds and the distance-ordered walk of both levels, written once for the
// kernel (rt_closest.hip) and for the host model (rt_closest_points_model), which differ only in where the walk finds its data
// (the `S` of rt_cp_search).  No HIP needed: tests/c/closest_test.cpp compiles it with g++ under ASan + UBSan
// (tests/test_closest_sanitizers_cpu.py).  Everything must be compiled without FMA contraction (-ffp-contract=off).
//
// THIS HEADER IS THE DEFINITION of what a query reports.  Reported values (rt_closest), per point p = {x, y, z, radius}:
//   * candidates: every (instance bi, lookup slot) with bi named by a leaf of the top-level tree, (mask of bi & ray mask) != 0 and
//     the slot in a leaf under the root of bi's record; indices clamp as in the ray walks (node -> last node, lookup position -> last
//     entry, bi -> last record, slot -> last slot, triangle -> last triangle).  Back faces count.
//   * world corners (rt_cp_corner): Fm = rt_tl_invert(record words 0..15) in float32; component k of a corner (x, y, z) is
//     ((Fm[k] x + Fm[4+k] y) + Fm[8+k] z) + Fm[12+k] in float64, left to right, rounded once to float32.  Affine: row 3 is not read.
//   * leaf (rt_cp_leaf): the closest point of the float32 p on the float32 world triangle, in float64, by the region tests of
//     Ericson, Real-Time Collision Detection 5.1.5, in the order vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior;
//     every dot product (x x' + y y') + z z'; d2 = (ex ex + ey ey) + ez ez with e = p - q.  dist2, u, v (weights of B and C) and the
//     point are those float64 values rounded once to float32.  No square root touches a reported value.
//   * acceptance: r2 = radius * radius in float32; a candidate counts iff dist2 <= r2 on the rounded value.  !(radius >= 0) -- a
//     negative or NaN radius -- reports the miss record; +inf searches without bound.  A NaN dist2 is no candidate.
//   * winner: the smallest candidate under (dist2, instance, prim); miss: dist2 = -1, prim = instance = -1, the rest 0.
// So the answer does not depend on the walk.
//
// Pruning is conservative, not bit-exact, and in float64 throughout.  `reach` is the square root of the float32 NEXT ABOVE the
// best dist2 so far (initially r2): every float64 d2 that rounds to a float32 <= best is below reach^2, so a candidate that only
// ties -- and may win by its indices -- is never behind a pruned box.  A box is skipped iff its lower bound is strictly beyond:
//   * top-level node: d2(p, world box) > (reach + 2^-20 max|bound|)^2;
//   * instance and bottom-level nodes: with p_obj = record (p, 1), L the record's 3 x 3 linear part (world -> object) and g the
//     largest absolute row sum of L^T L (Gershgorin: ||L||_2^2 <= g), |x_obj - y_obj| <= sqrt(g) |x_w - y_w|, so anything whose
//     object point lies in the box is at least d(p_obj, box) / sqrt(g) away in the world: skipped iff
//     d2(p_obj, box) > g (reach + slack)^2, slack = 2^-20 M, M = max over k of |Fm[k]| ax + |Fm[4+k]| ay + |Fm[8+k]| az + |Fm[12+k]|
//     with a the largest |bound| of the root box per axis.  The float32 rounding of Fm and of the world corners moves a corner by
//     at most about sqrt(3) 2^-23 M; the slack is more than four times that.  g and slack are stored as float32, rounded UP.
//     The bound needs Fm to be the record's inverse to float32 accuracy: rt_cp_inst checks record x Fm against the identity
//     entry by entry (2^-22 of the sum of the products' magnitudes) and stores g = NaN where it fails -- a singular record (whose
//     Fm is the identity by rt_tl_invert's rule), a projective bottom row, NaNs --, and nothing under such an instance is skipped.
//   * every comparison is written so that a NaN bound, slack or g skips nothing.
// Descent: the nearer child first, the farther pushed if its box is not beyond reach and tested again when popped; at a top-level
// leaf the instances in slot order.
//
// Stacks: kCpTopStack top-level and kCpBotStack bottom-level entries.  Nearer-first needs one entry per level, so every tree of
// rt_build_tlas (at most twenty levels) and of the project's BLAS builders is searched exhaustively.  A hand-made tree deeper
// than that: a push that finds its stack full is dropped -- memory-safe, every record still a true candidate, no more promised.
#pragma once
#include "rt_tlas_build.h"

constexpr uint32_t kCpTopStack = 20u, kCpBotStack = 32u;
constexpr uint32_t kCpInstWords = 16u;      // per instance: w[3 c + k] = Fm[4 c + k] (c < 4, k < 3), [12] g, [13] slack, [14..15] 0

RT_BB_HD inline double rt_cp_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// component k of the world corner of the object point c under w (the instance's constants)
RT_BB_HD inline float rt_cp_corner(const float* w, const float* c, int k) {
    return (float)((((double)w[k] * (double)c[0] + (double)w[3 + k] * (double)c[1]) + (double)w[6 + k] * (double)c[2]) + (double)w[9 + k]);
}

struct RtCpLeaf { float dist2, u, v, point[3]; };

// p: the point; A, B, C: the world corners
RT_BB_HD inline RtCpLeaf rt_cp_leaf(const float* p, const float* A, const float* B, const float* C) {
    const double a[3] = {(double)A[0], (double)A[1], (double)A[2]};
    const double b[3] = {(double)B[0], (double)B[1], (double)B[2]};
    const double c[3] = {(double)C[0], (double)C[1], (double)C[2]};
    const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {q[0] - a[0], q[1] - a[1], q[2] - a[2]};
    double u, v, s[3];
    const double d1 = rt_cp_dot(ab, ap), d2 = rt_cp_dot(ac, ap);
    const double bp[3] = {q[0] - b[0], q[1] - b[1], q[2] - b[2]};
    const double d3 = rt_cp_dot(ab, bp), d4 = rt_cp_dot(ac, bp);
    const double cp[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
    const double d5 = rt_cp_dot(ab, cp), d6 = rt_cp_dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {                                    // vertex A
        u = 0.0; v = 0.0;
        s[0] = a[0]; s[1] = a[1]; s[2] = a[2];
    } else if (d3 >= 0.0 && d4 <= d3) {                              // vertex B
        u = 1.0; v = 0.0;
        s[0] = b[0]; s[1] = b[1]; s[2] = b[2];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                // edge AB
        u = d1 / (d1 - d3); v = 0.0;
        s[0] = a[0] + u * ab[0]; s[1] = a[1] + u * ab[1]; s[2] = a[2] + u * ab[2];
    } else if (d6 >= 0.0 && d5 <= d6) {                              // vertex C
        u = 0.0; v = 1.0;
        s[0] = c[0]; s[1] = c[1]; s[2] = c[2];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                // edge AC
        u = 0.0; v = d2 / (d2 - d6);
        s[0] = a[0] + v * ac[0]; s[1] = a[1] + v * ac[1]; s[2] = a[2] + v * ac[2];
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {  // edge BC
        v = (d4 - d3) / ((d4 - d3) + (d5 - d6)); u = 1.0 - v;
        s[0] = b[0] + v * (c[0] - b[0]); s[1] = b[1] + v * (c[1] - b[1]); s[2] = b[2] + v * (c[2] - b[2]);
    } else {                                                         // interior
        const double denom = 1.0 / ((va + vb) + vc);
        u = vb * denom; v = vc * denom;
        s[0] = (a[0] + ab[0] * u) + ac[0] * v; s[1] = (a[1] + ab[1] * u) + ac[1] * v; s[2] = (a[2] + ab[2] * u) + ac[2] * v;
    }
    const double e[3] = {q[0] - s[0], q[1] - s[1], q[2] - s[2]};
    RtCpLeaf r;
    r.dist2 = (float)rt_cp_dot(e, e);
    r.u = (float)u; r.v = (float)v;
    r.point[0] = (float)s[0]; r.point[1] = (float)s[1]; r.point[2] = (float)s[2];
    return r;
}

// the larger of two magnitudes; a NaN stays
RT_BB_HD inline double rt_cp_larger(double a, double b) { return (b > a || b != b) ? b : a; }
// x as float32, never below it (NaN stays NaN)
RT_BB_HD inline float rt_cp_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, HUGE_VALF);
    return f;
}

// the constants of the instance whose record is rec (20 words) and whose root node has the box lo / hi -> w[kCpInstWords]
RT_BB_HD inline void rt_cp_inst(const float* rec, const float* lo, const float* hi, float* w) {
    float Fm[16];
    rt_tl_invert(rec, Fm);
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 3; ++k) w[3 * c + k] = Fm[4 * c + k];
    // g: the largest absolute row sum of L^T L, (L^T L)[i][j] = sum over r of rec[4 i + r] rec[4 j + r]
    double g = 0.0;
    for (int i = 0; i < 3; ++i) {
        double row = 0.0;
        for (int j = 0; j < 3; ++j) {
            double e = 0.0;
            for (int r = 0; r < 3; ++r) e += (double)rec[4 * i + r] * (double)rec[4 * j + r];
            row += fabs(e);
        }
        g = rt_cp_larger(g, row);
    }
    // is Fm the record's inverse, as affine maps?  (record x Fm)[r][c] = sum over j < 3 of rec[4 j + r] Fm[4 c + j] (+ rec[12 + r], c = 3)
    bool inverse = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double sum = 0.0, mag = 0.0;
            for (int j = 0; j < 3; ++j) {
                const double t = (double)rec[4 * j + r] * (double)Fm[4 * c + j];
                sum += t; mag += fabs(t);
            }
            if (c == 3) { sum += (double)rec[12 + r]; mag += fabs((double)rec[12 + r]); }
            if (c == r) { sum -= 1.0; mag += 1.0; }
            if (!(fabs(sum) <= mag * 2.384185791015625e-07)) inverse = false;      // 2^-22
        }
    if (!inverse) g = (double)NAN;
    double M = 0.0;
    for (int k = 0; k < 3; ++k) {
        double m = fabs((double)Fm[12 + k]);
        for (int c = 0; c < 3; ++c) m += fabs((double)Fm[4 * c + k]) * rt_cp_larger(fabs((double)lo[c]), fabs((double)hi[c]));
        M = rt_cp_larger(M, m);
    }
    w[12] = rt_cp_up(g);
    w[13] = rt_cp_up(M * 9.5367431640625e-07);                       // 2^-20
    w[14] = w[15] = 0.0f;
}

// squared distance from q to the box, float64; a NaN (a NaN bound or coordinate) counts as 0: such a box is nearest and never skipped
RT_BB_HD inline double rt_cp_box_d2(const double* q, const float* lo, const float* hi) {
    double e[3];
    for (int k = 0; k < 3; ++k) {
        const double below = (double)lo[k] - q[k], above = q[k] - (double)hi[k];
        if (below != below || above != above) return 0.0;
        const double d = below > above ? below : above;
        e[k] = d > 0.0 ? d : 0.0;
    }
    const double d2 = rt_cp_dot(e, e);
    return d2 == d2 ? d2 : 0.0;
}

// the slack of a top-level box: 2^-20 times its largest |bound|
RT_BB_HD inline double rt_cp_top_slack(const float* lo, const float* hi) {
    double m = 0.0;
    for (int k = 0; k < 3; ++k) m = rt_cp_larger(m, rt_cp_larger(fabs((double)lo[k]), fabs((double)hi[k])));
    return m * 9.5367431640625e-07;
}

// is a box at squared distance d2 beyond (reach + slack), scaled by g?  (false for any NaN; the 2^-40 covers the roundings here)
RT_BB_HD inline bool rt_cp_beyond(double d2, double g, double reach, double slack) {
    const double r = reach + slack;
    return d2 > (g * (r * r)) * (1.0 + 9.094947017729282e-13);
}

// reach for a best dist2 of `best` (float32, >= 0 or +inf)
RT_BB_HD inline double rt_cp_reach(float best) { return sqrt((double)nextafterf(best, HUGE_VALF)); }

struct RtCpNode { float lo[3], hi[3]; uint32_t left, count; };

// The search for one point.  S gives the scene:
//   uint32_t n_nodes, n_blas, n_blas_lookup, n_tri_lookup;  uint32_t ray_mask;
//   RtCpNode top(uint32_t i), node(uint32_t i)     a node of the top level / below an instance, i clamped to the last node
//   uint32_t instance_at(uint32_t li)              u32(blasLookup[li]), li < n_blas_lookup, not clamped
//   const float* record(uint32_t bi)               the 20 words; uint32_t mask(uint32_t bi); const float* consts(uint32_t bi)
//   void corners(uint32_t slot, float* A, float* B, float* C);  int prim(uint32_t slot)
//   T& tstack(uint32_t k), T& bstack(uint32_t k)   k < kCpTopStack / kCpBotStack; entries hold clamped node indices
// tests (COUNT): the candidates evaluated.
template <bool COUNT, class S>
RT_BB_HD inline void rt_cp_search(S& s, const float* p, rt_closest& out, uint64_t* tests) {
    out.dist2 = -1.0f; out.u = out.v = 0.0f; out.prim = -1; out.instance = -1;
    out.point[0] = out.point[1] = out.point[2] = 0.0f;
    const float radius = p[3];
    if (!(radius >= 0.0f)) return;
    float best = radius * radius;                                     // accepted: dist2 <= best, ties by (instance, prim)
    int best_inst = 0x7FFFFFFF, best_prim = 0x7FFFFFFF;
    double reach = rt_cp_reach(best);
    const double pw[3] = {(double)p[0], (double)p[1], (double)p[2]};
    uint32_t tsp = 0;
    RtCpNode tn = s.top(0u);
    bool have = !rt_cp_beyond(rt_cp_box_d2(pw, tn.lo, tn.hi), 1.0, reach, rt_cp_top_slack(tn.lo, tn.hi));
    for (;;) {
        if (have && tn.count == 0u) {
            RtCpNode c1 = s.top(tn.left), c2 = s.top(tn.left + 1u);
            uint32_t i2 = tn.left + 1u;
            double e1 = rt_cp_box_d2(pw, c1.lo, c1.hi), e2 = rt_cp_box_d2(pw, c2.lo, c2.hi);
            if (e1 > e2) { const RtCpNode t = c1; c1 = c2; c2 = t; const double e = e1; e1 = e2; e2 = e; i2 = tn.left; }
            if (!rt_cp_beyond(e2, 1.0, reach, rt_cp_top_slack(c2.lo, c2.hi)) && tsp < kCpTopStack) { s.tstack(tsp) = i2 < s.n_nodes ? i2 : s.n_nodes - 1u; tsp += 1u; }
            have = !rt_cp_beyond(e1, 1.0, reach, rt_cp_top_slack(c1.lo, c1.hi));
            tn = c1;
            if (have) continue;
        } else if (have) {
            for (uint32_t i = 0; i < tn.count; ++i) {
                uint32_t li = i + tn.left;
                if (li >= s.n_blas_lookup) li = s.n_blas_lookup - 1u;
                uint32_t bi = s.instance_at(li);
                if (bi >= s.n_blas) bi = s.n_blas - 1u;
                if ((s.mask(bi) & s.ray_mask) == 0u) continue;
                const float* m = s.record(bi);
                const float* w = s.consts(bi);
                const double po[3] = {(((double)m[0] * pw[0] + (double)m[4] * pw[1]) + (double)m[8] * pw[2]) + (double)m[12],
                                      (((double)m[1] * pw[0] + (double)m[5] * pw[1]) + (double)m[9] * pw[2]) + (double)m[13],
                                      (((double)m[2] * pw[0] + (double)m[6] * pw[1]) + (double)m[10] * pw[2]) + (double)m[14]};
                const double g = (double)w[12], slack = (double)w[13];
                uint32_t bsp = 0;
                RtCpNode bn = s.node(rt_bb_u32f(m[16]));
                bool bhave = !rt_cp_beyond(rt_cp_box_d2(po, bn.lo, bn.hi), g, reach, slack);
                for (;;) {
                    if (bhave && bn.count == 0u) {
                        RtCpNode c1 = s.node(bn.left), c2 = s.node(bn.left + 1u);
                        uint32_t i2 = bn.left + 1u;
                        double e1 = rt_cp_box_d2(po, c1.lo, c1.hi), e2 = rt_cp_box_d2(po, c2.lo, c2.hi);
                        if (e1 > e2) { const RtCpNode t = c1; c1 = c2; c2 = t; const double e = e1; e1 = e2; e2 = e; i2 = bn.left; }
                        if (!rt_cp_beyond(e2, g, reach, slack) && bsp < kCpBotStack) { s.bstack(bsp) = i2 < s.n_nodes ? i2 : s.n_nodes - 1u; bsp += 1u; }
                        bhave = !rt_cp_beyond(e1, g, reach, slack);
                        bn = c1;
                        if (bhave) continue;
                    } else if (bhave) {
                        for (uint32_t j = 0; j < bn.count; ++j) {
                            uint32_t slot = j + bn.left;
                            if (slot >= s.n_tri_lookup) slot = s.n_tri_lookup - 1u;
                            float oa[3], ob[3], oc[3], A[3], B[3], C[3];
                            s.corners(slot, oa, ob, oc);
                            for (int k = 0; k < 3; ++k) { A[k] = rt_cp_corner(w, oa, k); B[k] = rt_cp_corner(w, ob, k); C[k] = rt_cp_corner(w, oc, k); }
                            const RtCpLeaf f = rt_cp_leaf(p, A, B, C);
                            if (COUNT) *tests += 1u;
                            if (!(f.dist2 <= best)) continue;         // (a NaN is no candidate)
                            const int prim = s.prim(slot);
                            if (f.dist2 < best || (int)bi < best_inst || ((int)bi == best_inst && prim < best_prim)) {
                                best = f.dist2; best_inst = (int)bi; best_prim = prim;
                                reach = rt_cp_reach(best);
                                out.dist2 = f.dist2; out.u = f.u; out.v = f.v; out.prim = prim; out.instance = (int)bi;
                                out.point[0] = f.point[0]; out.point[1] = f.point[1]; out.point[2] = f.point[2];
                            }
                        }
                    }
                    if (bsp == 0u) break;
                    bsp -= 1u;
                    bn = s.node(s.bstack(bsp));
                    bhave = !rt_cp_beyond(rt_cp_box_d2(po, bn.lo, bn.hi), g, reach, slack);
                }
            }
        }
        if (tsp == 0u) break;
        tsp -= 1u;
        tn = s.top(s.tstack(tsp));
        have = !rt_cp_beyond(rt_cp_box_d2(pw, tn.lo, tn.hi), 1.0, reach, rt_cp_top_slack(tn.lo, tn.hi));
    }
}

// ---- the model: the whole call on caller arrays, serially (rt_closest_points_model) -----------------------------------------------
struct RtCpHostScene {
    const float *triangles, *tri_lookup, *nodes, *blas, *blas_lookup, *cst;
    const uint32_t* masks;
    uint32_t n_tri, n_tri_lookup, n_nodes, n_blas, n_blas_lookup, n_masks, ray_mask;
    uint32_t ts[kCpTopStack], bs[kCpBotStack];
    RtCpNode node(uint32_t i) const {
        if (i >= n_nodes) i = n_nodes - 1u;
        const float* q = nodes + 8u * (size_t)i;
        RtCpNode n;
        for (int k = 0; k < 3; ++k) { n.lo[k] = q[k]; n.hi[k] = q[4 + k]; }
        n.left = rt_bb_u32f(q[3]); n.count = rt_bb_u32f(q[7]);
        return n;
    }
    RtCpNode top(uint32_t i) const { return node(i); }
    uint32_t instance_at(uint32_t li) const { return rt_bb_u32f(blas_lookup[li]); }
    const float* record(uint32_t bi) const { return blas + 20u * (size_t)bi; }
    uint32_t mask(uint32_t bi) const { return bi < n_masks ? masks[bi] : 0xFFFFFFFFu; }
    const float* consts(uint32_t bi) const { return cst + kCpInstWords * (size_t)bi; }
    uint32_t tri_of(uint32_t slot) const {
        const uint32_t ti = rt_bb_u32f(tri_lookup[slot]);
        return ti >= n_tri ? n_tri - 1u : ti;
    }
    void corners(uint32_t slot, float* A, float* B, float* C) const {
        const float* t = triangles + 40u * (size_t)tri_of(slot);
        for (int k = 0; k < 3; ++k) { A[k] = t[k]; B[k] = t[12 + k]; C[k] = t[24 + k]; }
    }
    int prim(uint32_t slot) const { return (int)tri_of(slot); }
    uint32_t& tstack(uint32_t k) { return ts[k]; }
    uint32_t& bstack(uint32_t k) { return bs[k]; }
};

inline int rt_cp_model(const float* points, uint32_t n, const float* triangles, uint32_t n_triangles, const float* tri_lookup,
                       uint32_t n_tri_lookup, const float* nodes, uint32_t n_nodes, const float* blas, uint32_t n_blas,
                       const float* blas_lookup, uint32_t n_blas_lookup, const uint32_t* masks, uint32_t n_masks, uint32_t ray_mask,
                       rt_closest* out, uint64_t* tests, const char** why) {
    *why = "";
    if (tests) *tests = 0u;
    if (n == 0u) return RT_OK;
    if (!points || !out || !triangles || !tri_lookup || !nodes || !blas || !blas_lookup || (n_masks && !masks)) {
        *why = "NULL argument";
        return RT_ERR_INVALID_ARG;
    }
    if (!n_triangles || !n_tri_lookup || !n_nodes || !n_blas || !n_blas_lookup) { *why = "an empty scene array"; return RT_ERR_STATE; }
    std::vector<float> consts((size_t)n_blas * kCpInstWords);
    RtCpHostScene s;
    s.triangles = triangles; s.tri_lookup = tri_lookup; s.nodes = nodes; s.blas = blas; s.blas_lookup = blas_lookup;
    s.cst = consts.data(); s.masks = masks;
    s.n_tri = n_triangles; s.n_tri_lookup = n_tri_lookup; s.n_nodes = n_nodes; s.n_blas = n_blas; s.n_blas_lookup = n_blas_lookup;
    s.n_masks = n_masks; s.ray_mask = ray_mask;
    for (uint32_t bi = 0; bi < n_blas; ++bi) {
        const RtCpNode root = s.node(rt_bb_u32f(blas[20u * (size_t)bi + 16u]));
        rt_cp_inst(blas + 20u * (size_t)bi, root.lo, root.hi, consts.data() + kCpInstWords * (size_t)bi);
    }
    uint64_t count = 0u;
    for (uint32_t i = 0; i < n; ++i) rt_cp_search<true>(s, points + 4u * (size_t)i, out[i], &count);
    if (tests) *tests = count;
    return RT_OK;
}
