// rt_build.hip -- the device side of rt_build_blas (include/rt355.h): the SAH trees acceleration/bvh.py builds, made level by level.
//
// The arithmetic is rt_blas_build.h's, the same inline functions the host model (rt_build_blas_host) calls; this file is only the
// order the work is done in.  Built with -ffp-contract=off -fno-slp-vectorize: the planes, areas and costs are float64 sums of
// products and must stay so.  Nothing here depends on timing: no atomics, every reduction is a min / max or an integer sum, every
// append goes to a place a prefix sum names -- two builds of the same triangles leave the same bytes, in the scratch state too.
//
//   prep      per slot: the triangle's float32 box and centroid (RtBbPrim, 40 bytes), order[0] = identity; per range: the root.
//             (rt_build_tlas: the slots are instances, and rt_tlas.hip makes their prims from world boxes instead.)
//   price     per node of the level: lane p of a 32-lane group prices plane p of the 27 over every group-th triangle of the run
//             (the prim of an iteration is one address per group: a broadcast load out of L2), the groups' sides are merged by
//             fminf / fmaxf / +, lane p forms cost p in float64, every lane picks the first strict minimum.  A run of up to
//             kBuildShort triangles is one wave's (two groups), a longer one the workgroup's (eight): a block takes four nodes,
//             its waves one each first, then the long ones together.
//   scan      one block: the rank of every split among the level's splits -> the children's place in the next level, and the
//             next level's node count, the ONE word the host reads per level.
//   split     per node: a leaf copies its run to final_order; a split partitions its run stably into the other order buffer
//             (ballot and popcount in a wave, a carried prefix across chunks and waves) and writes its children's records --
//             their boxes are the winning plane's two sides, no second pass over the triangles.
//   count_up / rank_down   per level, last to first and back: splits per subtree, then preorder ranks -- the children of the
//             split of rank k sit at root_node + 1 + 2k, as build_tree numbers them.
//   emit      the 32-byte records into every version of the node buffer, the permuted words into the lookup table.
// Every index read from device memory is clamped before it addresses anything.
#include "rt_build.h"

namespace rtk {

constexpr uint32_t kBuildShort = 256u;       // the longest run a single wave prices and partitions

__device__ inline uint32_t bmin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the node with its run clamped into the lookup table
__device__ inline RtBuildNode build_node(const RtBuildArgs& A, uint32_t i) {
    RtBuildNode nd = A.node[bmin(i, A.node_cap - 1u)];
    nd.first = bmin(nd.first, A.n_slots);
    nd.count = bmin(nd.count, A.n_slots - nd.first);
    return nd;
}
__device__ inline uint32_t build_child(const RtBuildArgs& A, uint32_t off_next, uint32_t child) {      // the left child's place; + 1 stays inside
    const uint32_t c = off_next + child;
    return c < A.node_cap - 1u && c >= off_next ? c : (A.node_cap >= 2u ? A.node_cap - 2u : 0u);
}

__device__ inline void side_merge_xor32(RtBbSide& s) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = fminf(s.lo[a], __shfl_xor(s.lo[a], 32, 64));
        s.hi[a] = fmaxf(s.hi[a], __shfl_xor(s.hi[a], 32, 64));
    }
    s.n += __shfl_xor(s.n, 32, 64);
}

// ---- prep ----
__global__ __launch_bounds__(256) void build_prep(RtBuildArgs A, uint32_t range_base) {
    const uint32_t r = range_base + blockIdx.y, k = blockIdx.x * 256u + threadIdx.x;
    if (r >= A.n_ranges) return;
    const rt_blas_range g = A.ranges[r];
    if (k >= g.n_slots || g.first_slot >= A.n_slots || k >= A.n_slots - g.first_slot) return;
    const uint32_t slot = g.first_slot + k;
    const float raw = A.lookup[slot];
    uint32_t ti = rt_bb_u32f(raw);
    if (ti >= A.n_tri) ti = A.n_tri - 1u;                  // as tri_corners clamps it
    RtBbPrim p;
    rt_bb_prim(A.tri + 40u * (size_t)ti, raw, p);
    A.prim[slot] = p;
    A.order[0][slot] = slot;
}

// one block per range: the root's box, and where the tree goes
__global__ __launch_bounds__(256) void build_root(RtBuildArgs A) {
    __shared__ RtBbSide s_side[4];
    const uint32_t r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (r >= A.n_ranges || r >= A.node_cap) return;
    const rt_blas_range g = A.ranges[r];
    const uint32_t first = bmin(g.first_slot, A.n_slots), n = bmin(g.n_slots, A.n_slots - first);
    RtBbSide s;
    rt_bb_side_clear(s);
    for (uint32_t k = threadIdx.x; k < n; k += 256u) {
        const RtBbPrim& p = A.prim[first + k];
        rt_bb_side_add(s, p.lo, p.hi, 1u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s.lo[a] = fminf(s.lo[a], __shfl_xor(s.lo[a], off, 64));
            s.hi[a] = fmaxf(s.hi[a], __shfl_xor(s.hi[a], off, 64));
        }
    if (lane == 0u) s_side[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < 4u; ++w) rt_bb_side_add(s, s_side[w].lo, s_side[w].hi, 0u);
        RtBuildNode nd;
        for (int a = 0; a < 3; ++a) { nd.lo[a] = s.lo[a]; nd.hi[a] = s.hi[a]; }
        nd.first = first; nd.count = n;
        A.node[r] = nd;
        A.rank[r] = 0u;
        A.index[r] = g.root_node;
        A.root[r] = g.root_node;
    }
}

// ---- price ----
// GROUPS 32-lane groups of one team stride over the run; returns every plane's two sides in lanes p < 27 of every wave of the team
template <int GROUPS>
__device__ inline void price_sides(const RtBuildArgs& A, const RtBuildNode& nd, const uint32_t* src, uint32_t group, uint32_t p,
                                   RtBbSide& l, RtBbSide& r) {
    const uint32_t axis = rt_bb_axis_of(p);
    const double plane = rt_bb_plane_of(nd.lo, nd.hi, p);
    rt_bb_side_clear(l);
    rt_bb_side_clear(r);
    for (uint32_t k = group; k < nd.count; k += GROUPS) {
        const RtBbPrim& q = A.prim[bmin(src[nd.first + k], A.n_slots - 1u)];
        if (rt_bb_goes_left(q, axis, plane)) rt_bb_side_add(l, q.lo, q.hi, 1u);
        else rt_bb_side_add(r, q.lo, q.hi, 1u);
    }
    side_merge_xor32(l);
    side_merge_xor32(r);
}

// every lane of the wave holds plane min(lane & 31, 26)'s sides of the WHOLE run: decide, and let the deciding lanes store
__device__ inline void price_decide(const RtBuildArgs& A, uint32_t i, const RtBuildNode& nd, const RtBbSide& l, const RtBbSide& r,
                                    uint32_t lane, bool store) {
    const double mine = rt_bb_cost(l, r);
    double cost[kBbPlanes];
#pragma unroll
    for (uint32_t q = 0; q < kBbPlanes; ++q) cost[q] = __shfl(mine, (int)q, 64);
    const RtBbChoice c = rt_bb_choose(cost, nd.lo, nd.hi);
    const uint32_t n_left = c.index < kBbPlanes ? (uint32_t)__shfl((int)l.n, (int)c.index, 64) : 0u;
    const bool leaf = rt_bb_is_leaf(nd.count, nd.lo, nd.hi, c, n_left);
    if (!store) return;
    RtBuildDec& d = A.dec[i];
    if (lane == 0u) {
        d.plane = c.plane; d.axis = c.axis; d.n_left = n_left; d.split = leaf ? 0u : 1u; d.child = 0xFFFFFFFFu;
    }
    if (!leaf && lane == c.index) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { d.box[a] = l.lo[a]; d.box[3 + a] = l.hi[a]; d.box[6 + a] = r.lo[a]; d.box[9 + a] = r.hi[a]; }
    }
}

__global__ __launch_bounds__(256) void build_price(RtBuildArgs A, uint32_t level, uint32_t off, uint32_t cnt) {
    __shared__ RtBbSide s_side[4][2][kBbPlanes];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, p = bmin(lane & 31u, kBbPlanes - 1u);
    const uint32_t* src = A.order[level & 1u];
    const uint32_t base = blockIdx.x * 4u;
    {   // a wave per short node
        const uint32_t i = base + wave;
        if (i < cnt && off + i < A.node_cap) {
            const RtBuildNode nd = build_node(A, off + i);
            if (nd.count < 2u) {
                if (lane == 0u) { RtBuildDec& d = A.dec[off + i]; d.plane = 0.0; d.axis = 0u; d.n_left = 0u; d.split = 0u; d.child = 0xFFFFFFFFu; }
            } else if (nd.count <= kBuildShort) {
                RtBbSide l, r;
                price_sides<2>(A, nd, src, lane >> 5, p, l, r);
                price_decide(A, off + i, nd, l, r, lane, true);
            }
        }
    }
    // the long ones: the whole block, one after the other (every condition is uniform in the block)
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = base + j;
        if (i >= cnt || off + i >= A.node_cap) break;
        const RtBuildNode nd = build_node(A, off + i);
        if (nd.count <= kBuildShort) continue;
        RtBbSide l, r;
        price_sides<8>(A, nd, src, threadIdx.x >> 5, p, l, r);
        __syncthreads();                                   // (the previous long node's reads of s_side)
        if (lane < kBbPlanes) { s_side[wave][0][lane] = l; s_side[wave][1][lane] = r; }
        __syncthreads();
        rt_bb_side_clear(l);
        rt_bb_side_clear(r);
        for (uint32_t w = 0; w < 4u; ++w) {
            const RtBbSide &a = s_side[w][0][p], &b = s_side[w][1][p];
            rt_bb_side_add(l, a.lo, a.hi, a.n);
            rt_bb_side_add(r, b.lo, b.hi, b.n);
        }
        price_decide(A, off + i, nd, l, r, lane, wave == 0u);
    }
}

// ---- scan ----
__global__ __launch_bounds__(256) void build_scan(RtBuildArgs A, uint32_t off, uint32_t cnt) {
    __shared__ uint32_t s_n[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < cnt; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < cnt && off + i < A.node_cap;
        const bool f = in && A.dec[off + i].split != 0u;
        const unsigned long long m = __ballot(f);
        if (lane == 0u) s_n[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s_n[w]; total += s_n[w]; }
        if (f) A.dec[off + i].child = 2u * (carry + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0u) *A.next_count = 2u * carry;
}

// ---- split ----
__device__ inline void split_children(const RtBuildArgs& A, const RtBuildNode& nd, const RtBuildDec& d, uint32_t n_left, uint32_t off_next) {
    const uint32_t c = build_child(A, off_next, d.child);
    RtBuildNode a, b;
    for (int k = 0; k < 3; ++k) { a.lo[k] = d.box[k]; a.hi[k] = d.box[3 + k]; b.lo[k] = d.box[6 + k]; b.hi[k] = d.box[9 + k]; }
    a.first = nd.first; a.count = n_left;
    b.first = nd.first + n_left; b.count = nd.count - n_left;
    A.node[c] = a;
    A.node[c + 1u] = b;
}

__global__ __launch_bounds__(256) void build_split(RtBuildArgs A, uint32_t level, uint32_t off, uint32_t cnt) {
    __shared__ uint32_t s_n[4][2];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t* src = A.order[level & 1u];
    uint32_t* dst = A.order[(level + 1u) & 1u];
    const uint32_t base = blockIdx.x * 4u, off_next = off + cnt;
    const unsigned long long below = (1ull << lane) - 1ull;
    {   // a wave per short node
        const uint32_t i = base + wave;
        if (i < cnt && off + i < A.node_cap) {
            const RtBuildNode nd = build_node(A, off + i);
            if (nd.count <= kBuildShort) {
                const RtBuildDec& d = A.dec[off + i];
                if (!d.split || A.node_cap < 2u) {
                    for (uint32_t k = lane; k < nd.count; k += 64u) A.final_order[nd.first + k] = src[nd.first + k];
                } else {
                    const uint32_t axis = bmin(d.axis, 2u), n_left = bmin(d.n_left, nd.count);
                    const double plane = d.plane;
                    uint32_t nl = 0u, nr = 0u;
                    for (uint32_t b0 = 0; b0 < nd.count; b0 += 64u) {
                        const uint32_t k = b0 + lane;
                        const bool valid = k < nd.count;
                        const uint32_t id = valid ? bmin(src[nd.first + k], A.n_slots - 1u) : 0u;
                        const bool left = valid && rt_bb_goes_left(A.prim[id], axis, plane);
                        const unsigned long long ml = __ballot(left), mr = __ballot(valid && !left);
                        if (valid) {
                            const uint32_t pos = left ? nl + (uint32_t)__popcll(ml & below) : n_left + nr + (uint32_t)__popcll(mr & below);
                            dst[nd.first + bmin(pos, nd.count - 1u)] = id;
                        }
                        nl += (uint32_t)__popcll(ml);
                        nr += (uint32_t)__popcll(mr);
                    }
                    if (lane == 0u) split_children(A, nd, d, n_left, off_next);
                }
            }
        }
    }
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = base + j;
        if (i >= cnt || off + i >= A.node_cap) break;
        const RtBuildNode nd = build_node(A, off + i);
        if (nd.count <= kBuildShort) continue;
        const RtBuildDec& d = A.dec[off + i];
        if (!d.split || A.node_cap < 2u) {
            for (uint32_t k = threadIdx.x; k < nd.count; k += 256u) A.final_order[nd.first + k] = src[nd.first + k];
            continue;
        }
        const uint32_t axis = bmin(d.axis, 2u), n_left = bmin(d.n_left, nd.count);
        const double plane = d.plane;
        uint32_t nl = 0u, nr = 0u;
        for (uint32_t b0 = 0; b0 < nd.count; b0 += 256u) {
            const uint32_t k = b0 + threadIdx.x;
            const bool valid = k < nd.count;
            const uint32_t id = valid ? bmin(src[nd.first + k], A.n_slots - 1u) : 0u;
            const bool left = valid && rt_bb_goes_left(A.prim[id], axis, plane);
            const unsigned long long ml = __ballot(left), mr = __ballot(valid && !left);
            __syncthreads();                               // (the previous chunk's reads of s_n)
            if (lane == 0u) { s_n[wave][0] = (uint32_t)__popcll(ml); s_n[wave][1] = (uint32_t)__popcll(mr); }
            __syncthreads();
            uint32_t bl = 0u, br = 0u, tl = 0u, tr = 0u;
            for (uint32_t w = 0; w < 4u; ++w) {
                if (w < wave) { bl += s_n[w][0]; br += s_n[w][1]; }
                tl += s_n[w][0]; tr += s_n[w][1];
            }
            if (valid) {
                const uint32_t pos = left ? nl + bl + (uint32_t)__popcll(ml & below) : n_left + nr + br + (uint32_t)__popcll(mr & below);
                dst[nd.first + bmin(pos, nd.count - 1u)] = id;
            }
            nl += tl;
            nr += tr;
        }
        if (threadIdx.x == 0u) split_children(A, nd, d, n_left, off_next);
    }
}

// ---- number ----
__global__ __launch_bounds__(256) void build_count_up(RtBuildArgs A, uint32_t off, uint32_t cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cnt || off + i >= A.node_cap) return;
    const RtBuildDec& d = A.dec[off + i];
    uint32_t s = 0u;
    if (d.split && A.node_cap >= 2u) {
        const uint32_t c = build_child(A, off + cnt, d.child);
        s = 1u + A.sub[c] + A.sub[c + 1u];
    }
    A.sub[off + i] = s;
}

__global__ __launch_bounds__(256) void build_rank_down(RtBuildArgs A, uint32_t off, uint32_t cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cnt || off + i >= A.node_cap) return;
    const RtBuildDec& d = A.dec[off + i];
    if (!d.split || A.node_cap < 2u) return;
    const uint32_t c = build_child(A, off + cnt, d.child);
    const uint32_t rank = A.rank[off + i], root = A.root[off + i];
    A.rank[c] = rank + 1u;
    A.rank[c + 1u] = rank + 1u + A.sub[c];
    A.index[c] = root + 1u + 2u * rank;
    A.index[c + 1u] = root + 2u + 2u * rank;
    A.root[c] = root;
    A.root[c + 1u] = root;
}

// ---- emit ----
// `off_next` of a node is not kept: a split names its left child by dec.child relative to the next level, so emit runs per level
__global__ __launch_bounds__(256) void build_emit_nodes(RtBuildArgs A, uint32_t off, uint32_t cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cnt || off + i >= A.node_cap) return;
    const RtBuildNode nd = build_node(A, off + i);
    const RtBuildDec& d = A.dec[off + i];
    const uint32_t at = A.index[off + i];
    if (at >= A.n_nodes) return;
    const bool split = d.split && A.node_cap >= 2u;
    const float w3 = split ? (float)A.index[build_child(A, off + cnt, d.child)] : (float)nd.first;
    const float w7 = split ? 0.0f : (float)nd.count;
    const float4 a = make_float4(nd.lo[0], nd.lo[1], nd.lo[2], w3), b = make_float4(nd.hi[0], nd.hi[1], nd.hi[2], w7);
#pragma unroll
    for (uint32_t v = 0; v < kBuildVersions; ++v)
        if (A.nodes[v]) {
            float4* rec = reinterpret_cast<float4*>(A.nodes[v]) + 2u * (size_t)at;
            rec[0] = a;
            rec[1] = b;
        }
}

__global__ __launch_bounds__(256) void build_emit_lookup(RtBuildArgs A, uint32_t range_base) {
    const uint32_t r = range_base + blockIdx.y, k = blockIdx.x * 256u + threadIdx.x;
    if (r >= A.n_ranges) return;
    const rt_blas_range g = A.ranges[r];
    if (k >= g.n_slots || g.first_slot >= A.n_slots || k >= A.n_slots - g.first_slot) return;
    const uint32_t slot = g.first_slot + k;
    A.lookup[slot] = A.prim[bmin(A.final_order[slot], A.n_slots - 1u)].raw;
}

}  // namespace rtk

static uint32_t build_max_slots(const rt_blas_range* h_ranges, uint32_t n) {
    uint32_t m = 0u;
    for (uint32_t i = 0; i < n; ++i) m = h_ranges[i].n_slots > m ? h_ranges[i].n_slots : m;
    return m;
}

hipError_t rt_launch_build_prep(const RtBuildArgs& a, const rt_blas_range* h_ranges, hipStream_t s) {
    if (a.inst.models) {                                   // the instance front end (rt_tlas.hip) makes the prims of the one range
        const hipError_t e = rt_launch_tlas_prep(a, s);
        if (e != hipSuccess) return e;
    } else {
        const uint32_t bx = (build_max_slots(h_ranges, a.n_ranges) + 255u) / 256u;
        for (uint32_t r0 = 0; r0 < a.n_ranges; r0 += 65535u) {
            const uint32_t ny = a.n_ranges - r0 < 65535u ? a.n_ranges - r0 : 65535u;
            hipLaunchKernelGGL(rtk::build_prep, dim3(bx, ny), dim3(256), 0, s, a, r0);
        }
    }
    hipLaunchKernelGGL(rtk::build_root, dim3(a.n_ranges), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t rt_launch_build_level(const RtBuildArgs& a, uint32_t level, uint32_t off, uint32_t cnt, hipStream_t s) {
    hipLaunchKernelGGL(rtk::build_price, dim3((cnt + 3u) / 4u), dim3(256), 0, s, a, level, off, cnt);
    hipLaunchKernelGGL(rtk::build_scan, dim3(1), dim3(256), 0, s, a, off, cnt);
    hipLaunchKernelGGL(rtk::build_split, dim3((cnt + 3u) / 4u), dim3(256), 0, s, a, level, off, cnt);
    return hipGetLastError();
}

hipError_t rt_launch_build_count_up(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s) {
    hipLaunchKernelGGL(rtk::build_count_up, dim3((cnt + 255u) / 256u), dim3(256), 0, s, a, off, cnt);
    return hipGetLastError();
}

hipError_t rt_launch_build_rank_down(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s) {
    hipLaunchKernelGGL(rtk::build_rank_down, dim3((cnt + 255u) / 256u), dim3(256), 0, s, a, off, cnt);
    return hipGetLastError();
}

hipError_t rt_launch_build_emit_nodes(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s) {
    hipLaunchKernelGGL(rtk::build_emit_nodes, dim3((cnt + 255u) / 256u), dim3(256), 0, s, a, off, cnt);
    return hipGetLastError();
}

hipError_t rt_launch_build_emit_lookup(const RtBuildArgs& a, const rt_blas_range* h_ranges, hipStream_t s) {
    const uint32_t bx = (build_max_slots(h_ranges, a.n_ranges) + 255u) / 256u;
    for (uint32_t r0 = 0; r0 < a.n_ranges; r0 += 65535u) {
        const uint32_t ny = a.n_ranges - r0 < 65535u ? a.n_ranges - r0 : 65535u;
        hipLaunchKernelGGL(rtk::build_emit_lookup, dim3(bx, ny), dim3(256), 0, s, a, r0);
    }
    return hipGetLastError();
}
