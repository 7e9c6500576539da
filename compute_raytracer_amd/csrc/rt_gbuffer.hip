// rt_gbuffer.hip -- geometry frames on gfx950 (include/rt355.h: rt_render_gbuffer, rt_render_gbuffer_host): per pixel of a rectangle
// of the frame the nearest hit of its primary ray -- what rt_pick reports for that pixel -- stored as up to four dense planes: depth,
// normal, ids, barycentrics.  Compiled like rt_query.hip with -ffp-contract=off -fno-slp-vectorize; the ray is pick_rays' (rt_device.h:
// primary_dir), the walks are query_triangles' and query_spheres' own (rt_tri_device.h: trace_tlas, hit_normal; rt_shade_device.h:
// search_spheres, the literal loop in staged chunks), so a pixel is bit for bit the rt_hit of rt_pick and of the oracle
// (oracle/rt_oracle.c: rt_oracle_trace_tri_rays, hit_sphere).
//
// CDNA4 mapping: one pixel per lane, wave64, kQueryWaves waves per workgroup.  A wave is an 8 x 8 pixel tile, as in the frame
// kernels -- its rays stay in step through the trees --, and a workgroup four tiles side by side, 32 x 8 pixels; tiles are counted
// from the rectangle's corner, so a rectangle need not be tile-aligned.  A lane builds its ray in registers: there is no ray buffer
// and no coordinate buffer, and nothing is read per pixel.  A lane outside the rectangle carries no ray and stores nothing.  A wave
// stores a plane in eight row segments -- 32 B of depth, 64 B of ids or uv, 128 B of normal each -- and the four waves of a workgroup
// complete 128 B, 256 B and 512 B of a row between them; a plane that was not asked for costs no store.  Pixel indices are 64-bit:
// w h may pass 2^32.
//   gbuffer_triangles: trace_tlas in the forms and with the LDS of query_triangles.
//   gbuffer_spheres: search_spheres -- every sphere in index order, for rt_query.hip's reason; every lane meets every barrier.
#include <type_traits>

#include "rt_shade_device.h"

namespace rtk {

// rt_hit as planes: pixel (x, y) of the rectangle
__device__ __forceinline__ void store_planes(const RtGbufferOut& O, uint32_t x, uint32_t y, float t, float u, float v, int prim, int inst,
                                             v3 n) {
    const size_t i = (size_t)y * O.w + x;
    if (O.depth) O.depth[i] = t;
    if (O.normal) O.normal[i] = make_float4(n.x, n.y, n.z, 0.0f);
    if (O.ids) O.ids[i] = make_int2(prim, inst);
    if (O.uv) O.uv[i] = make_float2(u, v);
}
__device__ __forceinline__ void store_miss_planes(const RtGbufferOut& O, uint32_t x, uint32_t y) {
    store_planes(O, x, y, -1.0f, 0.0f, 0.0f, -1, -1, V(0.0f, 0.0f, 0.0f));
}

// STK / PACKED / PAIRS / P16 / INST as in query_triangles
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void gbuffer_triangles(const RtFrameArgs A, const RtTriScene T, const RtQueryMask M, const RtGbufferOut O) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    uint32_t x, y;
    if (!pixel_of_lane(O, x, y)) return;           // (stage_head's barrier was the last one)
    const Scene sc = unpack_scene(A);
    const v3 o = sc.cameraPos, d = primary_dir(A, sc, O.x0 + x, O.y0 + y);
    RtTriScene Tq = T;                             // (as in query_triangles: a node buffer wholly inside the staged head)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    float traces = 0.0f;
    const TriVis vis = {M.table, M.n, M.nearest};
    const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, o, d, tstacks + threadIdx.x, bstacks + threadIdx.x,
                                                                 kQueryThreads, traces, 0.0f, 0.0f, &vis);
    if (h.tri < 0) { store_miss_planes(O, x, y); return; }
    // RK:334-338 for the winner (the staged record keeps the matrix in words 0-15)
    const uint32_t bi = (uint32_t)h.blas;
    const float* m = bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi;
    v3 nrm = V(0.0f, 0.0f, 0.0f);
    if (O.normal) nrm = hit_normal(T, h, m);
    const int prim = O.ids ? (int)tri_of(T, h.tri) : 0;
    store_planes(O, x, y, h.t, h.u, h.v, prim, h.blas, nrm);
}

__global__ __launch_bounds__(kQueryThreads) void gbuffer_spheres(const RtFrameArgs A, const float* __restrict__ records, uint32_t n_spheres,
                                                                 const RtGbufferOut O) {
    __shared__ float4 s_geo[kSphereChunk];
    uint32_t x, y;
    const bool live = pixel_of_lane(O, x, y);      // every lane stages and meets every barrier: no return before the last one
    const Scene sc = unpack_scene(A);
    const v3 o = sc.cameraPos;
    v3 d = V(0.0f, 0.0f, 0.0f);
    if (live) d = primary_dir(A, sc, O.x0 + x, O.y0 + y);
    float nearest;
    int idx;
    search_spheres(records, n_spheres, s_geo, /*resident=*/false, live, o, d, nearest, idx);
    if (!live) return;
    if (idx < 0) { store_miss_planes(O, x, y); return; }
    v3 nrm = V(0.0f, 0.0f, 0.0f);
    if (O.normal) {
        const float* s = records + 8u * (size_t)idx;
        const v3 position = add(o, scale(nearest, d));                 // HK:319
        nrm = normalize(sub(position, V(s[0], s[1], s[2])));            // HK:320
    }
    store_planes(O, x, y, nearest, 0.0f, 0.0f, idx, -1, nrm);
}

}  // namespace rtk

// the rectangle lies in the frame the rays are made for, some plane is asked for, and the grid is one the launch can have
static bool gbuffer_args_ok(const RtFrameArgs& a, const RtGbufferOut& o) {
    return o.W && o.H && a.W == o.W && a.H == o.H && o.w && o.h && (uint64_t)o.x0 + o.w <= o.W && (uint64_t)o.y0 + o.h <= o.H &&
           (o.depth || o.normal || o.ids || o.uv) && rtk::frame_blocks(o) <= 0x7FFFFFFFull;
}

hipError_t rt_launch_gbuffer_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtGbufferOut& o, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (!gbuffer_args_ok(a, o)) return hipErrorInvalidValue;
    rtk::query_form(t, inst, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::gbuffer_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3((uint32_t)rtk::frame_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, t, m, o);
    });
    return hipGetLastError();
}

hipError_t rt_launch_gbuffer_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtGbufferOut& o, hipStream_t s) {
    if (!gbuffer_args_ok(a, o)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtk::gbuffer_spheres, dim3((uint32_t)rtk::frame_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, records, n_spheres, o);
    return hipGetLastError();
}
