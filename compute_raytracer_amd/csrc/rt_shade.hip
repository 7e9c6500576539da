// rt_shade.hip -- shaded ray queries on gfx950 (include/rt355.h: rt_shade_rays, rt_shade_rays_host): what the renderer would show
// along rays the caller supplies -- rayColor (RK:101-144) for any origin and direction, and optionally pixelColor (RK:91-96) on top
// of it -- as four floats {r, g, b, dist} per ray.  Compiled like rt_query.hip with -ffp-contract=off -fno-slp-vectorize: traversal,
// hit attributes, light term and sky filter are the frame kernels' own device functions (rt_tri_device.h, rt_device.h,
// rt_filter.h), every expression in the oracle's order, so a result is bit for bit the oracle's (oracle/rt_oracle.c: ray_color,
// shade_pixel).
//
// CDNA4 mapping: one ray per lane, wave64, kQueryWaves waves per workgroup, like the other queries.  A ray is two float4 and a
// result one: a wave reads 2 KB and writes 1 KB in coalesced rows.
//   shade_triangles: the bounce loop of trace_triangles (rt_triangles.hip) without tiles, work list, ray counters or parking: per
//     bounce trace_tlas along the path, the hit's normal, albedo and texture sample, the reflection, trace_tlas from the light, the
//     shadow test, the running mean.  The forms and the LDS of limited_triangles (rt_query.hip).
//   shade_spheres: the literal test (HK:307-331) over every sphere in index order for the path ray and the shadow ray, the records
//     staged through LDS -- once per workgroup when the scene is at most one chunk, otherwise chunk by chunk in every search.  Not
//     the bounding-sphere hierarchy, for rt_query.hip's reason: caller rays promise neither unit directions nor origins within
//     rt_plan's reach.  Every lane of the workgroup reaches every barrier, lanes without a ray and lanes whose path has ended
//     included; the workgroup leaves the bounce loop when none of its lanes has a path left.
// The sky a path escapes into (RK:122-125) is sampled after the loop and, under RT_SHADE_COMPOSE, the fog colour along the ray as
// given (RK:92) through the same one copy of the cube filter, as in trace_triangles.  The two bounce loops and the end of a path are
// in rt_shade_device.h, shared with the camera samples of rt_sample.hip.
#include <type_traits>

#include "rt_shade_device.h"

namespace rtk {

// path_colour (rt_shade_device.h) under `flags` -- the fog colour: the sky along the ray as the caller gave it, read again from the
// ray buffer rather than carried through the bounce loop -- and the one store.
__device__ __forceinline__ void shade_finish(const RtFrameArgs& A, const Scene& sc, const float4* __restrict__ rays, uint32_t flags,
                                             float4* __restrict__ out, size_t i, const PathEnd& e) {
    const v3 color = path_colour(A, sc, e, (flags & RT_SHADE_COMPOSE) != 0u, [&]() {
        const float4 b = rays[2u * i + 1u];
        return V(b.x, b.y, b.z);
    });
    out[i] = make_float4(color.x, color.y, color.z, e.dist);               // RK:143
}

// STK / PACKED / PAIRS / P16 / INST as in limited_triangles (rt_query.hip)
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void shade_triangles(const RtFrameArgs A, const RtTriScene T, const RtQueryMask M,
                                                                 const float4* __restrict__ rays, uint32_t flags, float4* __restrict__ out,
                                                                 uint32_t n) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;                            // (no barrier after the staging)
    v3 ro, rd;
    load_ray(rays, i, ro, rd);
    RtTriScene Tq = T;                             // (as in query_triangles: a node buffer wholly inside the staged head)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    const Scene sc = unpack_scene(A);
    const TriVis vis = {M.table, M.n, M.nearest};
    const PathEnd e = path_triangles<STK, PACKED, PAIRS, P16>(T, Tq, L, sc, ro, rd, tstacks + threadIdx.x, bstacks + threadIdx.x, vis);
    shade_finish(A, sc, rays, flags, out, i, e);
}

__global__ __launch_bounds__(kQueryThreads) void shade_spheres(const RtFrameArgs A, const float* __restrict__ records, uint32_t n_spheres,
                                                               const float4* __restrict__ rays, uint32_t flags, float4* __restrict__ out,
                                                               uint32_t n) {
    __shared__ float4 s_geo[kSphereChunk];
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;                       // every lane stages and meets every barrier: no return before the last one
    const bool resident = n_spheres <= kSphereChunk;
    if (resident) {
        stage_spheres(records, 0u, n_spheres, s_geo);
        __syncthreads();
    }
    v3 ro = V(0.0f, 0.0f, 0.0f), rd = V(0.0f, 0.0f, 0.0f);
    if (live) load_ray(rays, i, ro, rd);
    const Scene sc = unpack_scene(A);
    const PathEnd e = path_spheres(records, n_spheres, s_geo, resident, sc, live, ro, rd);
    if (!live) return;
    shade_finish(A, sc, rays, flags, out, i, e);
}

}  // namespace rtk

hipError_t rt_launch_shade_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const float4* rays, uint32_t flags, float4* out,
                                     uint32_t n, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    rtk::query_form(t, inst, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::shade_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, a, t, m, rays, flags, out, n);
    });
    return hipGetLastError();
}

hipError_t rt_launch_shade_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags,
                                   float4* out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    hipLaunchKernelGGL(rtk::shade_spheres, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, a, records, n_spheres, rays, flags, out, n);
    return hipGetLastError();
}
