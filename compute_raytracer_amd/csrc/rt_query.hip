// rt_query.hip -- ray queries on gfx950 (include/rt355.h: rt_trace_rays, rt_trace_rays_host, rt_pick): the nearest hit of
// rays the caller supplies, against the scene the next frame would render.  Compiled like rt_triangles.hip with
// -ffp-contract=off -fno-slp-vectorize: the traversal and the tests are the frame kernels' own device functions
// (rt_tri_device.h, rt_filter.h), so a query's t, barycentrics and normal are bit for bit what the oracle computes for the
// same ray (oracle/rt_oracle.c: rt_oracle_trace_tri_rays, hit_sphere).
//
// CDNA4 mapping: one ray per lane, wave64, kQueryWaves waves per workgroup.  A ray is two float4 {origin, -}, {dir, -} and a
// hit two float4 {t, u, v, prim}, {instance, normal}: a wave reads and writes 2 KB in two coalesced 1 KB rows.
//   query_triangles: traceTLAS (RK:168-244) with the twenty-slot top-level stack and the reference's guard, so that any
//     top-level tree gives the oracle's answer; both stacks in LDS, slot-major as in trace_triangles.  The head of the
//     top-level tree and the instance records are staged by stage_head -- from the kernel's arguments when the instance data
//     travels with the frame (RtTriInst), from the per-frame buffers otherwise.
//   query_spheres: the literal test (HK:307-331) over every sphere in index order, the records staged through LDS in chunks
//     (any sphere count).  Not the bounding-sphere hierarchy: its no-lost-hit proof (rt_bvh.hip) assumes unit directions and
//     origins within rt_plan's reach, and caller rays promise neither.
//   pick_rays: the primary ray of pixel (x, y) (RK:76-86, rt_device.h: primary_dir) into a ray buffer.
// The limited and occlusion forms (rt_trace_rays_ex, rt_occluded): the same walks over (tmin, tmax), from ray words 3 and 7
// under RT_QUERY_LIMITS and (0.001, 9999) otherwise -- the literal bounds, so a lane without limits does what the forms above do.
//   limited_triangles<..., ANY>: trace_tlas<LIMITS, ANY>; the occlusion form (ANY) leaves both loops at the first accepted
//     triangle and writes one byte: no normal, no triangle lookup.  The same LDS as query_triangles.
//   limited_spheres / occlude_spheres: the literal loop with exact_full<LIMITS>.  In occlude_spheres a lane stops testing at its
//     first accepted sphere, and the workgroup stops staging chunks once none of its lanes is still searching.
// The multi-hit form (rt_trace_rays_multi): the k nearest hits in the order (t, instance, prim), k records per ray.
//   multi_triangles<K, ...>: multi_tlas (rt_tri_device.h) -- the same walk under the t of the lane's k-th hit, which it keeps with
//     the others in a sorted register list of capacity K (4 or 8).  multi_spheres<K>: the literal loop into the same list.
// Instance visibility masks (rt_write_instance_masks, rt_set_query_masks): every triangle kernel here, and those of rt_shade.hip,
//   rt_sample.hip, rt_gbuffer.hip and rt_ao.hip, takes an RtQueryMask M beside the scene -- the device table of instance masks and
//   the call's two ray masks.  stage_head puts the masks of the staged records into their word 18; the walks get a TriVis
//   {table, n, ray mask} and leave an instance whose mask shares no bit with the ray's before its ray transform (rt_tri_device.h).
//   The sphere kernels take no masks: a sphere scene has no instances.
#include <type_traits>

#include "rt_device.h"
#include "rt_tri_types.h"
#include "rt_tri_device.h"
#include "rt_filter.h"
#include "rt_query_device.h"

namespace rtk {

// rt_hit: {t, u, v, prim}, {instance, normal.xyz}
__device__ __forceinline__ void store_hit(float4* __restrict__ hits, size_t i, float t, float u, float v, int prim, int inst, v3 n) {
    hits[2u * i] = make_float4(t, u, v, __int_as_float(prim));
    hits[2u * i + 1u] = make_float4(__int_as_float(inst), n.x, n.y, n.z);
}
__device__ __forceinline__ void store_miss(float4* __restrict__ hits, size_t i) {
    store_hit(hits, i, -1.0f, 0.0f, 0.0f, -1, -1, V(0.0f, 0.0f, 0.0f));
}

// STK / PACKED / PAIRS / P16 as in trace_tlas; INST: the instance data came with the arguments (T.inst, stage_head<..., true>)
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void query_triangles(const RtTriScene T, const RtQueryMask M,
                                                                 const float4* __restrict__ rays, float4* __restrict__ hits, uint32_t n) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);   // (INST: roots in T.inst)
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;
    v3 o, d;
    load_ray(rays, i, o, d);
    // A node buffer that lies wholly inside the head (RR's buffer for a scene of small meshes) was written as per-frame data: its
    // BLAS nodes too are current only in the staged copy (the device versions are brought up to date by frames of the
    // twenty-slot form alone) -- the node walk then reads them from LDS, through the generic address.
    RtTriScene Tq = T;
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    float traces = 0.0f;
    const TriVis vis = {M.table, M.n, M.nearest};
    const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, o, d, tstacks + threadIdx.x, bstacks + threadIdx.x,
                                                                 kQueryThreads, traces, 0.0f, 0.0f, &vis);
    if (h.tri < 0) { store_miss(hits, i); return; }
    // RK:334-338 for the winner (the staged record keeps the matrix in words 0-15)
    const uint32_t bi = (uint32_t)h.blas;
    const float* m = bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi;
    const v3 nrm = hit_normal(T, h, m);
    store_hit(hits, i, h.t, h.u, h.v, (int)tri_of(T, h.tri), h.blas, nrm);
}

// RK:311-322 over spheres with hitSphere (HK:307-331): tMin 0.001, the running nearest hit as tMax, the lowest index on a tie
__global__ __launch_bounds__(kQueryThreads) void query_spheres(const float* __restrict__ records, uint32_t n_spheres,
                                                               const float4* __restrict__ rays, float4* __restrict__ hits, uint32_t n) {
    __shared__ float4 s_geo[kSphereChunk];
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;                       // every lane stages: no return before the last barrier
    v3 o = V(0.0f, 0.0f, 0.0f), d = V(0.0f, 0.0f, 0.0f);
    if (live) load_ray(rays, i, o, d);
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    float nearest = 9999.0f;                       // RK:172
    int idx = -1;
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        __syncthreads();                           // the previous chunk is done with
        for (uint32_t k = threadIdx.x; k < m; k += kQueryThreads) {
            const float4* r = reinterpret_cast<const float4*>(records + 8u * ((size_t)base + k));
            const float4 c = r[0], w = r[1];
            s_geo[k] = make_float4(c.x, c.y, c.z, w.w * w.w);       // radius * radius (HK:310)
        }
        __syncthreads();
        if (live) {
            for (uint32_t k = 0; k < m; ++k) {
                const float4 g = s_geo[k];
                exact_full<false>(V(g.x, g.y, g.z), g.w, (int)(base + k), o, d, fa, ta, nearest, idx);
            }
        }
    }
    if (!live) return;
    if (idx < 0) { store_miss(hits, i); return; }
    const float* s = records + 8u * (size_t)idx;
    const v3 position = add(o, scale(nearest, d));                     // HK:319
    const v3 nrm = normalize(sub(position, V(s[0], s[1], s[2])));       // HK:320
    store_hit(hits, i, nearest, 0.0f, 0.0f, idx, -1, nrm);
}

// ---- RT_QUERY_LIMITS and occlusion -------------------------------------------------------------------------------------------
// (tmin, tmax) of ray i: words 3 and 7 under RT_QUERY_LIMITS, else the reference's 0.001 and 9999
__device__ __forceinline__ void load_ray_limits(const float4* __restrict__ rays, size_t i, bool limits, v3& o, v3& d,
                                                float& tmin, float& tmax) {
    const float4 a = rays[2u * i], b = rays[2u * i + 1u];
    o = V(a.x, a.y, a.z);
    d = V(b.x, b.y, b.z);
    tmin = limits ? a.w : 0.001f;
    tmax = limits ? b.w : 9999.0f;
}

// query_triangles over (tmin, tmax); ANY: rt_occluded (one byte per ray in `occ`, the rays carry M.occlusion), else rt_hit records
// in `hits` (M.nearest)
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST, bool ANY>
__global__ __launch_bounds__(kQueryThreads) void limited_triangles(const RtTriScene T, const RtQueryMask M, const float4* __restrict__ rays,
                                                                   uint32_t flags, float4* __restrict__ hits, uint8_t* __restrict__ occ,
                                                                   uint32_t n) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;
    v3 o, d;
    float tmin, tmax;
    load_ray_limits(rays, i, (flags & RT_QUERY_LIMITS) != 0u, o, d, tmin, tmax);
    RtTriScene Tq = T;                             // (as in query_triangles)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    float traces = 0.0f;
    const TriVis vis = {M.table, M.n, ANY ? M.occlusion : M.nearest};
    const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16, kStack, /*LIMITS=*/true, ANY>(
        Tq, L, o, d, tstacks + threadIdx.x, bstacks + threadIdx.x, kQueryThreads, traces, tmin, tmax, &vis);
    if (ANY) { occ[i] = h.tri >= 0 ? 1u : 0u; return; }
    if (h.tri < 0) { store_miss(hits, i); return; }
    const uint32_t bi = (uint32_t)h.blas;
    const float* m = bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi;
    const v3 nrm = hit_normal(T, h, m);
    store_hit(hits, i, h.t, h.u, h.v, (int)tri_of(T, h.tri), h.blas, nrm);
}

// query_spheres over (tmin, tmax): the running nearest hit starts at tmax
__global__ __launch_bounds__(kQueryThreads) void limited_spheres(const float* __restrict__ records, uint32_t n_spheres,
                                                                 const float4* __restrict__ rays, uint32_t flags,
                                                                 float4* __restrict__ hits, uint32_t n) {
    __shared__ float4 s_geo[kSphereChunk];
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;                       // every lane stages: no return before the last barrier
    v3 o = V(0.0f, 0.0f, 0.0f), d = V(0.0f, 0.0f, 0.0f);
    float tmin = 0.001f, tmax = 9999.0f;
    if (live) load_ray_limits(rays, i, (flags & RT_QUERY_LIMITS) != 0u, o, d, tmin, tmax);
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    float nearest = tmax;
    int idx = -1;
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        __syncthreads();                           // the previous chunk is done with
        for (uint32_t k = threadIdx.x; k < m; k += kQueryThreads) {
            const float4* r = reinterpret_cast<const float4*>(records + 8u * ((size_t)base + k));
            const float4 c = r[0], w = r[1];
            s_geo[k] = make_float4(c.x, c.y, c.z, w.w * w.w);       // radius * radius (HK:310)
        }
        __syncthreads();
        if (live) {
            for (uint32_t k = 0; k < m; ++k) {
                const float4 g = s_geo[k];
                exact_full<false, true>(V(g.x, g.y, g.z), g.w, (int)(base + k), o, d, fa, ta, nearest, idx, tmin);
            }
        }
    }
    if (!live) return;
    if (idx < 0) { store_miss(hits, i); return; }
    const float* s = records + 8u * (size_t)idx;
    const v3 position = add(o, scale(nearest, d));                     // HK:319
    const v3 nrm = normalize(sub(position, V(s[0], s[1], s[2])));       // HK:320
    store_hit(hits, i, nearest, 0.0f, 0.0f, idx, -1, nrm);
}

// limited_spheres up to the first accepted sphere: that acceptance is the nearest search's first too (nearest is still tmax),
// so a lane is occluded exactly when limited_spheres would report a hit
__global__ __launch_bounds__(kQueryThreads) void occlude_spheres(const float* __restrict__ records, uint32_t n_spheres,
                                                                 const float4* __restrict__ rays, uint32_t flags,
                                                                 uint8_t* __restrict__ occ, uint32_t n) {
    __shared__ float4 s_geo[kSphereChunk];
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;                       // every lane stages: no return before the last barrier
    v3 o = V(0.0f, 0.0f, 0.0f), d = V(0.0f, 0.0f, 0.0f);
    float tmin = 0.001f, tmax = 9999.0f;
    if (live) load_ray_limits(rays, i, (flags & RT_QUERY_LIMITS) != 0u, o, d, tmin, tmax);
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    float nearest = tmax;
    int idx = -1;
    bool searching = live;
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        // the previous chunk is done with -- and when no lane of the workgroup still searches, no chunk more is staged (the
        // barrier's answer is the same in every lane: all of them leave together)
        if (!__syncthreads_or(searching)) break;
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        for (uint32_t k = threadIdx.x; k < m; k += kQueryThreads) {
            const float4* r = reinterpret_cast<const float4*>(records + 8u * ((size_t)base + k));
            const float4 c = r[0], w = r[1];
            s_geo[k] = make_float4(c.x, c.y, c.z, w.w * w.w);       // radius * radius (HK:310)
        }
        __syncthreads();
        if (searching) {
            for (uint32_t k = 0; k < m; ++k) {
                const float4 g = s_geo[k];
                exact_full<false, true>(V(g.x, g.y, g.z), g.w, (int)(base + k), o, d, fa, ta, nearest, idx, tmin);
                if (idx >= 0) { searching = false; break; }
            }
        }
    }
    if (!live) return;
    occ[i] = idx >= 0 ? 1u : 0u;
}

// ---- the k nearest hits (rt_trace_rays_multi) ---------------------------------------------------------------------------------
// hits [n][k] rt_hit: ray i's records at i*k .., sorted by (t, instance, prim), then miss records.  The list of a lane is a
// HitList<K> in registers (rt_tri_device.h), K = 4 or 8 by k; LDS is limited_triangles' (both stacks and the staged head).

// multi_tlas, then for each survivor what query_triangles stores for its winner: u and v are formed again by the arithmetic that
// accepted the triangle (the same operations on the same operands: the same bits), the normal and the triangle index once each
template <int K, typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void multi_triangles(const RtTriScene T, const RtQueryMask M, const float4* __restrict__ rays,
                                                                 uint32_t flags, uint32_t k, float4* __restrict__ hits, uint32_t n) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;
    v3 o, d;
    float tmin, tmax;
    load_ray_limits(rays, i, (flags & RT_QUERY_LIMITS) != 0u, o, d, tmin, tmax);
    RtTriScene Tq = T;                             // (as in query_triangles)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    HitList<K, true> list;
    const TriVis vis = {M.table, M.n, M.nearest};
    multi_tlas<K, STK, PACKED, PAIRS, P16>(Tq, L, o, d, list, k, tstacks + threadIdx.x, bstacks + threadIdx.x, kQueryThreads, tmin, tmax, &vis);
    for (uint32_t j = 0; j < k; ++j) {
        TriHit h;
        int prim;
        list.get(j, h.t, h.blas, prim, h.tri);
        if (h.tri < 0) { store_miss(hits, i * k + j); continue; }
        const uint32_t bi = (uint32_t)h.blas;
        const float* m = bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi;
        v3 oo, od;
        instance_ray(m, o, d, oo, od);
        float t;
        (void)triangle_tuv(T, (uint32_t)h.tri, oo, od, t, h.u, h.v);
        const v3 nrm = hit_normal(T, h, m);
        store_hit(hits, i * k + j, h.t, h.u, h.v, prim, h.blas, nrm);
    }
}

// limited_spheres' loop; every sphere whose near root lies in (tmin, tmax) goes to the list (exact_full against tmax alone is that
// acceptance, and leaves the root in `t`)
template <int K>
__global__ __launch_bounds__(kQueryThreads) void multi_spheres(const float* __restrict__ records, uint32_t n_spheres,
                                                               const float4* __restrict__ rays, uint32_t flags, uint32_t k,
                                                               float4* __restrict__ hits, uint32_t n) {
    __shared__ float4 s_geo[kSphereChunk];
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;                       // every lane stages: no return before the last barrier
    v3 o = V(0.0f, 0.0f, 0.0f), d = V(0.0f, 0.0f, 0.0f);
    float tmin = 0.001f, tmax = 9999.0f;
    if (live) load_ray_limits(rays, i, (flags & RT_QUERY_LIMITS) != 0u, o, d, tmin, tmax);
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    HitList<K, false> list;
    list.init(tmax);
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        __syncthreads();                           // the previous chunk is done with
        for (uint32_t q = threadIdx.x; q < m; q += kQueryThreads) {
            const float4* r = reinterpret_cast<const float4*>(records + 8u * ((size_t)base + q));
            const float4 c = r[0], w = r[1];
            s_geo[q] = make_float4(c.x, c.y, c.z, w.w * w.w);       // radius * radius (HK:310)
        }
        __syncthreads();
        if (live) {
            for (uint32_t q = 0; q < m; ++q) {
                const float4 g = s_geo[q];
                float t = tmax;
                int idx = -1;
                exact_full<false, true>(V(g.x, g.y, g.z), g.w, (int)(base + q), o, d, fa, ta, t, idx, tmin);
                if (idx >= 0 && t <= list.bound) list.insert(k, t, 0, idx, 0);
            }
        }
    }
    if (!live) return;
    for (uint32_t j = 0; j < k; ++j) {
        float t;
        int idx, unused_inst, unused_slot;
        list.get(j, t, unused_inst, idx, unused_slot);
        if (idx == 0x7FFFFFFF) { store_miss(hits, i * k + j); continue; }
        const float* s = records + 8u * (size_t)idx;
        const v3 position = add(o, scale(t, d));                           // HK:319
        const v3 nrm = normalize(sub(position, V(s[0], s[1], s[2])));       // HK:320
        store_hit(hits, i * k + j, t, 0.0f, 0.0f, idx, -1, nrm);
    }
}

// the primary ray of pixel (x, y) (RK:76-86): the ray that pixel of the next frame starts with
__global__ __launch_bounds__(256) void pick_rays(const RtFrameArgs A, const uint32_t* __restrict__ xy, float4* __restrict__ rays, uint32_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Scene sc = unpack_scene(A);
    const v3 d = primary_dir(A, sc, xy[2u * i], xy[2u * i + 1u]);
    rays[2u * i] = make_float4(sc.cameraPos.x, sc.cameraPos.y, sc.cameraPos.z, 0.0f);
    rays[2u * i + 1u] = make_float4(d.x, d.y, d.z, 0.0f);
}

}  // namespace rtk

hipError_t rt_launch_multi_triangles(const RtTriScene& t, int inst, const float4* rays, uint32_t flags, uint32_t k, float4* hits,
                                     uint32_t n, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (n == 0) return hipSuccess;
    if (k == 0 || k > RT355_MAX_HITS) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    // K, the capacity of a lane's list, is the outer choice; the scene's form the inner one
    const auto launch = [&](auto f, auto cap) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::multi_triangles<decltype(cap)::value, typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3(blocks),
                           dim3(rtk::kQueryThreads), 0, s, t, m, rays, flags, k, hits, n);
    };
    if (k <= 4u) rtk::query_form(t, inst, [&](auto f) { launch(f, std::integral_constant<int, 4>()); });
    else         rtk::query_form(t, inst, [&](auto f) { launch(f, std::integral_constant<int, 8>()); });
    return hipGetLastError();
}

hipError_t rt_launch_multi_spheres(const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags, uint32_t k, float4* hits,
                                   uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (k == 0 || k > RT355_MAX_HITS) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    if (k <= 4u) hipLaunchKernelGGL(rtk::multi_spheres<4>, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, records, n_spheres, rays, flags, k, hits, n);
    else         hipLaunchKernelGGL(rtk::multi_spheres<8>, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, records, n_spheres, rays, flags, k, hits, n);
    return hipGetLastError();
}

hipError_t rt_launch_query_triangles(const RtTriScene& t, int inst, const float4* rays, float4* hits, uint32_t n, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    rtk::query_form(t, inst, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::query_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3(blocks), dim3(rtk::kQueryThreads), 0, s, t, m, rays, hits, n);
    });
    return hipGetLastError();
}

hipError_t rt_launch_query_spheres(const float* records, uint32_t n_spheres, const float4* rays, float4* hits, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    hipLaunchKernelGGL(rtk::query_spheres, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, records, n_spheres, rays, hits, n);
    return hipGetLastError();
}

hipError_t rt_launch_limited_triangles(const RtTriScene& t, int inst, const float4* rays, uint32_t flags, bool any, void* out,
                                       uint32_t n, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    // ANY is the outer choice, the scene's form the inner one
    const auto launch = [&](auto f, auto any_form) {
        typedef decltype(f) F;
        constexpr bool ANY = decltype(any_form)::value;
        hipLaunchKernelGGL((rtk::limited_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST, ANY>), dim3(blocks), dim3(rtk::kQueryThreads),
                           0, s, t, m, rays, flags, ANY ? nullptr : static_cast<float4*>(out), ANY ? static_cast<uint8_t*>(out) : nullptr, n);
    };
    if (any) rtk::query_form(t, inst, [&](auto f) { launch(f, std::true_type()); });
    else     rtk::query_form(t, inst, [&](auto f) { launch(f, std::false_type()); });
    return hipGetLastError();
}

hipError_t rt_launch_limited_spheres(const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags, bool any, void* out,
                                     uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    if (any) hipLaunchKernelGGL(rtk::occlude_spheres, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, records, n_spheres, rays, flags,
                                static_cast<uint8_t*>(out), n);
    else     hipLaunchKernelGGL(rtk::limited_spheres, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, records, n_spheres, rays, flags,
                                static_cast<float4*>(out), n);
    return hipGetLastError();
}

hipError_t rt_launch_pick_rays(const RtFrameArgs& a, const uint32_t* xy, float4* rays, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::pick_rays, dim3((uint32_t)(((size_t)n + 255u) / 256u)), dim3(256), 0, s, a, xy, rays, n);
    return hipGetLastError();
}
