// rt_closest.hip -- closest-point queries on gfx950 (include/rt355.h: rt_closest_points): for each caller point the nearest
// surface point of a triangle scene within a radius.  Compiled like rt_query.hip with -ffp-contract=off -fno-slp-vectorize: every
// reported bit comes from rt_closest.h (rt_cp_leaf, rt_cp_corner), which the host model (rt_closest_points_model) compiles too, and
// that header is the definition of the answer.  The walk is rt_cp_search over a device view of the scene (CpDevice below).
//
// CDNA4 mapping: one point per lane, wave64, kQueryWaves waves per workgroup, as the ray queries.  A point is one float4
// {x, y, z, radius} and a result two float4 {dist2, u, v, prim}, {instance, point}: a wave reads 1 KB and writes 2 KB, coalesced.
//   closest_inst: one thread per instance, in front of the search on the same stream -- Fm (rt_tl_invert of the record), g and the
//     slack of rt_closest.h into a buffer the context owns (16 words per instance), so that no point pays for a matrix inverse.
//     The records come from the kernel's arguments when the instance data travels with the call (INST), else from T.blas.
//   closest_points: the head of the node buffer and the instance records staged by stage_head exactly as in query_triangles (the
//     node buffer that lies wholly inside the head included); both stacks in LDS, slot-major (entry k of a lane at k * threads +
//     lane), kCpTopStack + kCpBotStack entries of two bytes while the node buffer has at most 65,536 nodes and of four beyond.
//     Float64 (full rate on this part) carries the leaves and the box distances; nothing is counted and nothing printed.
#include "rt_device.h"
#include "rt_tri_types.h"
#include "rt_tri_device.h"
#include "rt_query_device.h"
#include "rt_closest.h"

namespace rtk {

__device__ __forceinline__ RtCpNode cp_node(const NodeR& n) {
    RtCpNode r;
    r.lo[0] = n.lo.x; r.lo[1] = n.lo.y; r.lo[2] = n.lo.z;
    r.hi[0] = n.hi.x; r.hi[1] = n.hi.y; r.hi[2] = n.hi.z;
    r.left = u32f(n.left); r.count = u32f(n.count);
    return r;
}

// the scene as rt_cp_search reads it
template <typename STK>
struct CpDevice {
    const RtTriScene& T;
    const TriLds& L;
    const RtQueryMask& M;
    const float* cst;
    STK *ts, *bs;
    uint32_t n_nodes, n_blas, n_blas_lookup, n_tri_lookup, ray_mask;
    __device__ __forceinline__ RtCpNode top(uint32_t i) const { return cp_node(load_node_head(T, L, i)); }
    __device__ __forceinline__ RtCpNode node(uint32_t i) const { return cp_node(load_node(T, i)); }
    __device__ __forceinline__ uint32_t instance_at(uint32_t li) const { return u32f(li < L.n_lookup ? L.blas[20u * li + 19u] : T.blas_lookup[li]); }
    __device__ __forceinline__ const float* record(uint32_t bi) const { return bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi; }
    __device__ __forceinline__ uint32_t mask(uint32_t bi) const {
        if (bi < L.n_blas) return __float_as_uint(L.blas[20u * bi + 18u]);
        return bi < M.n ? M.table[bi] : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ const float* consts(uint32_t bi) const { return cst + kCpInstWords * (size_t)bi; }
    __device__ __forceinline__ void corners(uint32_t slot, float* A, float* B, float* C) const {
        const float4* tr = T.corners + 3u * (size_t)slot;
        const float4 a = tr[0], b = tr[1], c = tr[2];
        A[0] = a.x; A[1] = a.y; A[2] = a.z;
        B[0] = b.x; B[1] = b.y; B[2] = b.z;
        C[0] = c.x; C[1] = c.y; C[2] = c.z;
    }
    __device__ __forceinline__ int prim(uint32_t slot) const { return (int)tri_of(T, (int)slot); }
    __device__ __forceinline__ STK& tstack(uint32_t k) const { return ts[k * kQueryThreads]; }
    __device__ __forceinline__ STK& bstack(uint32_t k) const { return bs[k * kQueryThreads]; }
};

// INST: the instance data came with the arguments (T.inst, stage_head<..., true>), as in query_triangles
template <typename STK, bool INST>
__global__ __launch_bounds__(kQueryThreads) void closest_points(const RtTriScene T, const RtQueryMask M, const float* __restrict__ cst,
                                                                const float4* __restrict__ points, float4* __restrict__ out, uint32_t n) {
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kCpTopStack * kQueryThreads];
    __shared__ STK bstacks[kCpBotStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;
    RtTriScene Tq = T;                             // (as in query_triangles: a node buffer wholly inside the head is current only there)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    CpDevice<STK> s = {Tq, L, M, cst, tstacks + threadIdx.x, bstacks + threadIdx.x,
                       T.n_nodes, T.n_blas, T.n_blas_lookup, T.n_tri_lookup, M.nearest};
    const float4 q = points[i];
    const float p[4] = {q.x, q.y, q.z, q.w};
    rt_closest r;
    rt_cp_search<false>(s, p, r, nullptr);
    out[2u * i] = make_float4(r.dist2, r.u, r.v, __int_as_float(r.prim));
    out[2u * i + 1u] = make_float4(__int_as_float(r.instance), r.point[0], r.point[1], r.point[2]);
}

// the constants of instance bi = blockIdx.x * kQueryThreads + threadIdx.x
template <bool INST>
__global__ __launch_bounds__(kQueryThreads) void closest_inst(const RtTriScene T, float* __restrict__ cst) {
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas);
    const uint32_t bi = blockIdx.x * kQueryThreads + threadIdx.x;
    if (bi >= T.n_blas) return;
    RtTriScene Tq = T;
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    float rec[20];
    const float* m = bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi;
#pragma unroll
    for (int k = 0; k < 17; ++k) rec[k] = m[k];
    const RtCpNode root = cp_node(load_node(Tq, u32f(rec[16])));
    float w[kCpInstWords];
    rt_cp_inst(rec, root.lo, root.hi, w);
    float4* o = reinterpret_cast<float4*>(cst + kCpInstWords * (size_t)bi);
    o[0] = make_float4(w[0], w[1], w[2], w[3]);
    o[1] = make_float4(w[4], w[5], w[6], w[7]);
    o[2] = make_float4(w[8], w[9], w[10], w[11]);
    o[3] = make_float4(w[12], w[13], w[14], w[15]);
}

}  // namespace rtk

// cst: room for 16 words per BLAS record of t (the context's buffer)
hipError_t rt_launch_closest_points(const RtTriScene& t, int inst, float* cst, const float4* points, float4* out, uint32_t n, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (n == 0 || t.n_blas == 0) return hipSuccess;
    const uint32_t iblocks = (t.n_blas + rtk::kQueryThreads - 1u) / rtk::kQueryThreads;
    if (inst) hipLaunchKernelGGL(rtk::closest_inst<true>, dim3(iblocks), dim3(rtk::kQueryThreads), 0, s, t, cst);
    else      hipLaunchKernelGGL(rtk::closest_inst<false>, dim3(iblocks), dim3(rtk::kQueryThreads), 0, s, t, cst);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return e; }
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    const bool small = t.n_nodes <= 65536u;
    if (inst && small)  hipLaunchKernelGGL((rtk::closest_points<uint16_t, true>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, t, m, cst, points, out, n);
    else if (inst)      hipLaunchKernelGGL((rtk::closest_points<uint32_t, true>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, t, m, cst, points, out, n);
    else if (small)     hipLaunchKernelGGL((rtk::closest_points<uint16_t, false>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, t, m, cst, points, out, n);
    else                hipLaunchKernelGGL((rtk::closest_points<uint32_t, false>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, t, m, cst, points, out, n);
    return hipGetLastError();
}

static const bool rt_closest_registered = (rt_closest_launch = &rt_launch_closest_points, true);
