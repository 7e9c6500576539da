// rt_ao.hip -- ambient-occlusion frames on gfx950 (include/rt355.h: rt_render_ao, rt_render_ao_host): per pixel of a rectangle of the
// frame, how many of k rays from the point the camera sees there, spread over the hemisphere of its shading normal, are blocked within
// (tmin, radius).  Compiled like rt_gbuffer.hip with -ffp-contract=off -fno-slp-vectorize: the primary ray and its walk are
// rt_gbuffer.hip's (rt_device.h: primary_dir; rt_tri_device.h: trace_tlas, hit_normal; rt_shade_device.h: search_spheres), the k
// walks are rt_occluded's (trace_tlas<LIMITS, ANY>; the literal sphere loop with exact_full<false, true> up to the first accepted
// sphere), and what lies between them -- hit point, basis, directions -- is one float32 operation per line in the header's order.  So a
// pixel's count is the sum of what rt_occluded reports for the k rays the header describes, made from what rt_pick reports.
//
// CDNA4 mapping: the geometry frame's -- one pixel per lane, a wave an 8 x 8 tile, kQueryWaves tiles per workgroup.  After the primary
// walk a lane keeps the hit point, T, B, n and its count in registers (13 VGPRs) and walks the k rays one after the other on the LDS
// stacks the primary walk used.  The loop over the rays is wave-uniform and direction j comes from the kernel's own arguments through
// a uniform address: scalar loads, no ray in memory and none in vector registers beyond the one being walked.  The 64 lanes of a tile
// walk the same tangent direction from neighbouring points under neighbouring normals.  A lane whose primary ray missed stores its
// 0 / 1.0f and leaves; a lane outside the rectangle stores nothing.  One store per plane per pixel: a wave writes 8 B (count) and 32 B
// (ao) per row of its tile, the four waves of a workgroup 32 B and 128 B of a row between them.
//   ao_triangles: the forms and the LDS of gbuffer_triangles.
//   ao_spheres: every lane meets every barrier; a scene of one chunk is staged once and stays in LDS for all k + 1 searches, a larger
//     one is staged again by every search, and the workgroup stops staging for a ray once none of its lanes still searches.
#include <type_traits>

#include "rt_shade_device.h"

namespace rtk {

// Steps 3 - 5 of the header: the point the primary ray (o, d) reaches at t, and the tangent frame of the normal n there
struct AoFrame {
    v3 p, T, B, n;
};
__device__ __forceinline__ AoFrame ao_frame(v3 o, v3 d, float t, v3 n) {
    AoFrame f;
    f.p = add(o, scale(t, d));                                     // HK:319
    f.n = n;
    const float s = n.z >= 0.0f ? 1.0f : -1.0f;                    // (-0 gives +1, NaN gives -1)
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    f.T = V(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    f.B = V(b, s + (n.y * n.y) * a, -n.y);
    return f;
}
// step 6: direction j of the kernel's arguments in that frame
__device__ __forceinline__ v3 ao_dir(const AoFrame& f, const RtAoOut& O, uint32_t j) {
    const float dx = O.dirs[3u * j], dy = O.dirs[3u * j + 1u], dz = O.dirs[3u * j + 2u];
    return V((dx * f.T.x + dy * f.B.x) + dz * f.n.x, (dx * f.T.y + dy * f.B.y) + dz * f.n.y, (dx * f.T.z + dy * f.B.z) + dz * f.n.z);
}

// pixel (x, y) of the rectangle: `count` of the O.k rays are occluded
__device__ __forceinline__ void store_ao(const RtAoOut& O, uint32_t x, uint32_t y, uint32_t count) {
    const size_t i = (size_t)y * O.w + x;
    if (O.count) O.count[i] = (uint8_t)count;
    if (O.ao) O.ao[i] = (float)(O.k - count) / (float)O.k;
}

// STK / PACKED / PAIRS / P16 / INST as in query_triangles
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void ao_triangles(const RtFrameArgs A, const RtTriScene T, const RtQueryMask M, const RtAoOut O) {
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
    const TriVis vis = {M.table, M.n, M.nearest};      // the primary ray: a nearest-hit search
    const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, o, d, tstacks + threadIdx.x, bstacks + threadIdx.x,
                                                                 kQueryThreads, traces, 0.0f, 0.0f, &vis);
    if (h.tri < 0) { store_ao(O, x, y, 0u); return; }
    const uint32_t bi = (uint32_t)h.blas;
    const AoFrame f = ao_frame(o, d, h.t, hit_normal(T, h, bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi));
    uint32_t count = 0u;
    const TriVis avis = {M.table, M.n, M.occlusion};   // the k rays: rt_occluded's
#pragma unroll 1
    for (uint32_t j = 0; j < O.k; ++j) {
        const TriHit a = trace_tlas<false, STK, PACKED, PAIRS, P16, kStack, /*LIMITS=*/true, /*ANY=*/true>(
            Tq, L, f.p, ao_dir(f, O, j), tstacks + threadIdx.x, bstacks + threadIdx.x, kQueryThreads, traces, O.tmin, O.radius, &avis);
        count += a.tri >= 0 ? 1u : 0u;
    }
    store_ao(O, x, y, count);
}

// occlude_spheres' search for one ray of every lane (rt_query.hip): the literal loop over (tmin, tmax) up to the first accepted
// sphere.  EVERY lane of the workgroup calls it, `on` or not; resident: the whole scene is in s_geo already.
__device__ __forceinline__ bool occlude_search(const float* __restrict__ records, uint32_t n_spheres, float4* s_geo, bool resident, bool on,
                                               v3 o, v3 d, float tmin, float tmax) {
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    float nearest = tmax;
    int idx = -1;
    bool searching = on;
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        if (!resident) {
            // the previous chunk is done with -- and when no lane of the workgroup still searches, no chunk more is staged (the
            // barrier's answer is the same in every lane: all of them leave together)
            if (!__syncthreads_or(searching)) break;
            stage_spheres(records, base, m, s_geo);
            __syncthreads();
        }
        if (searching) {
            for (uint32_t k = 0; k < m; ++k) {
                const float4 g = s_geo[k];
                exact_full<false, true>(V(g.x, g.y, g.z), g.w, (int)(base + k), o, d, fa, ta, nearest, idx, tmin);
                if (idx >= 0) { searching = false; break; }
            }
        }
    }
    return idx >= 0;
}

__global__ __launch_bounds__(kQueryThreads) void ao_spheres(const RtFrameArgs A, const float* __restrict__ records, uint32_t n_spheres,
                                                            const RtAoOut O) {
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
    const bool resident = n_spheres <= kSphereChunk;               // the primary search left the one chunk there is in s_geo
    const bool hit = live && idx >= 0;
    AoFrame f = {V(0.0f, 0.0f, 0.0f), V(0.0f, 0.0f, 0.0f), V(0.0f, 0.0f, 0.0f), V(0.0f, 0.0f, 0.0f)};
    if (hit) {
        const float* s = records + 8u * (size_t)idx;
        const v3 position = add(o, scale(nearest, d));             // HK:319
        f = ao_frame(o, d, nearest, normalize(sub(position, V(s[0], s[1], s[2]))));   // HK:320
    }
    uint32_t count = 0u;
#pragma unroll 1
    for (uint32_t j = 0; j < O.k; ++j)
        count += occlude_search(records, n_spheres, s_geo, resident, hit, f.p, ao_dir(f, O, j), O.tmin, O.radius) ? 1u : 0u;
    if (live) store_ao(O, x, y, count);
}

}  // namespace rtk

// the four argument blocks of ao_triangles travel by value: together they must fit the 4 KB a kernel's arguments may take
static_assert(sizeof(RtFrameArgs) + sizeof(RtTriScene) + sizeof(RtQueryMask) + sizeof(RtAoOut) <= 4096, "ao_triangles' arguments exceed the kernarg segment");

// the rectangle lies in the frame the rays are made for, some plane is asked for, k is in range, and the grid is one the launch can have
static bool ao_args_ok(const RtFrameArgs& a, const RtAoOut& o) {
    return o.W && o.H && a.W == o.W && a.H == o.H && o.w && o.h && (uint64_t)o.x0 + o.w <= o.W && (uint64_t)o.y0 + o.h <= o.H &&
           (o.count || o.ao) && o.k >= 1u && o.k <= RT355_MAX_AO_RAYS && rtk::frame_blocks(o) <= 0x7FFFFFFFull;
}

// (one form for the primary walk and the k occlusion walks: a ray is walked in the form rt_occluded walks it in)
hipError_t rt_launch_ao_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtAoOut& o, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (!ao_args_ok(a, o)) return hipErrorInvalidValue;
    rtk::query_form(t, inst, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::ao_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3((uint32_t)rtk::frame_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, t, m, o);
    });
    return hipGetLastError();
}

hipError_t rt_launch_ao_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtAoOut& o, hipStream_t s) {
    if (!ao_args_ok(a, o)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtk::ao_spheres, dim3((uint32_t)rtk::frame_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, records, n_spheres, o);
    return hipGetLastError();
}
