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
// given (RK:92) through the same one copy of the cube filter, as in trace_triangles.
#include <type_traits>

#include "rt_device.h"
#include "rt_tri_types.h"
#include "rt_tri_device.h"
#include "rt_filter.h"
#include "rt_query_device.h"

namespace rtk {

// RK:122-125 for a path that escaped along `rd`, then RK:91-96 under RT_SHADE_COMPOSE (the fog colour: the sky along the ray as the
// caller gave it, read again from the ray buffer rather than carried through the bounce loop), and the one store.
__device__ __forceinline__ void shade_finish(const RtFrameArgs& A, const Scene& sc, const float4* __restrict__ rays, uint32_t flags,
                                             float4* __restrict__ out, size_t i, v3 color, float dist, bool missed, v3 rd,
                                             float affect, float sum) {
    const bool compose = (flags & RT_SHADE_COMPOSE) != 0u;
    v3 fog = V(0.0f, 0.0f, 0.0f);
    v3 dir = rd;
#pragma unroll 1
    for (int k = missed ? 0 : 1; k < (compose ? 2 : 1); ++k) {             // one copy of the cube filter for both samples
        if (k == 1) { const float4 b = rays[2u * i + 1u]; dir = V(b.x, b.y, b.z); }
        const v3 sky = scale(sc.minIntensity, cube_sample(A, dir));        // RK:123 / RK:92
        if (k == 0) color = divs(add(scale(sum, color), scale(affect, sky)), affect + sum);   // RK:120, 124
        else fog = sky;
    }
    if (compose) color = compose_color_sky(fog, color, dist);              // RK:94-96
    out[i] = make_float4(color.x, color.y, color.z, dist);                 // RK:143
}

// STK / PACKED / PAIRS / P16 / INST as in limited_triangles (rt_query.hip)
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void shade_triangles(const RtFrameArgs A, const RtTriScene T, const float4* __restrict__ rays,
                                                                 uint32_t flags, float4* __restrict__ out, uint32_t n) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas);
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    if (i >= n) return;                            // (no barrier after the staging)
    v3 ro, rd;
    load_ray(rays, i, ro, rd);
    RtTriScene Tq = T;                             // (as in query_triangles: a node buffer wholly inside the staged head)
    if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
    STK* tstack = tstacks + threadIdx.x;
    BSTK* bstack = bstacks + threadIdx.x;
    const Scene sc = unpack_scene(A);
    float dummy = 0.0f;
    v3 color = V(1.0f, 1.0f, 1.0f);                // RK:103
    float dist = 0.0f;                             // RK:102: 0 unless the first ray hits (RK:116-118)
    float affect = 1.0f, sum = 0.0f;               // RK:111-112
    bool missed = false;
    for (uint32_t bounce = 0; bounce < sc.bounces; ++bounce) {                       // RK:113
        const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, ro, rd, tstack, bstack, kQueryThreads, dummy);   // RK:114
        if (h.tri < 0) { missed = true; break; }                                     // RK:122-126: sampled after the loop
        if (bounce == 0) dist = h.t;                                                 // RK:116-118
        const float next = affect + sum;                                             // RK:120
        const uint32_t bi = (uint32_t)h.blas;
        const v3 normal = hit_normal(T, h, bi < L.n_blas ? L.blas + 20u * bi : T.blas + 20u * (size_t)bi);
        const Albedo s = hit_albedo(T, h.tri, h.u, h.v);
        ro = add(ro, scale(h.t, rd));                                                // RK:129
        rd = normalize(reflect(rd, normal));                                         // RK:130
        // RK:146-166 lightIntensity: everything but the shadow ray's verdict is formed before the ray is cast
        const v3 sdir = normalize(sub(ro, sc.lightPos));                             // RK:147
        const float distance = length(sdir);                                         // RK:148
        const float power = clampf(dot(normal, V(-sdir.x, -sdir.y, -sdir.z)), sc.minIntensity, 1.0f);   // RK:160
        const float cap = sc.lightIntensity / (sc.lightIntensity + distance);                           // RK:161
        const float lit = power * cap;                                                                  // RK:162
        const v3 diffuseColor = scale(s.w, s.rgb);                                   // RK:133
        const v3 samplerColor = scale(1.0f - s.w, tex2d_sample(T, s.u, s.v));        // RK:134
        const v3 albedo = add(diffuseColor, samplerColor);                           // RK:135, the sum
        const TriHit sh = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, sc.lightPos, sdir, tstack, bstack, kQueryThreads, dummy);   // RK:153
        float intensity = sc.minIntensity;                                           // RK:165
        if (sh.tri >= 0) {                                                           // RK:155
            const v3 hp = add(sc.lightPos, scale(sh.t, sdir));                       // RK:156
            const v3 dv = sub(hp, ro);                                               // RK:157-159: see light_term (rt_device.h)
            if (dot(dv, dv) < 0x1.a36e2cp-16f) intensity = lit;
        }
        const v3 blended = scale(intensity, albedo);                                 // RK:135
        color = divs(add(scale(sum, color), scale(affect, blended)), next);          // RK:136
        affect = affect / 2.0f;                                                      // RK:139
        sum = next;                                                                  // RK:140
    }
    shade_finish(A, sc, rays, flags, out, i, color, dist, missed, rd, affect, sum);
}

// one chunk of sphere records into LDS as {centre, radius * radius} (HK:310); the caller places the barriers
__device__ __forceinline__ void stage_spheres(const float* __restrict__ records, uint32_t base, uint32_t m, float4* s_geo) {
    for (uint32_t k = threadIdx.x; k < m; k += kQueryThreads) {
        const float4* r = reinterpret_cast<const float4*>(records + 8u * ((size_t)base + k));
        const float4 c = r[0], w = r[1];
        s_geo[k] = make_float4(c.x, c.y, c.z, w.w * w.w);
    }
}
// RK:311-322 over spheres with hitSphere (HK:307-331), as query_spheres searches: tMin 0.001, the running nearest hit as tMax, the
// lowest index on a tie.  EVERY lane of the workgroup calls it, `on` or not: a scene of more than one chunk is staged here, between
// barriers.  resident: the whole scene is in s_geo already.
__device__ __forceinline__ void search_spheres(const float* __restrict__ records, uint32_t n_spheres, float4* s_geo, bool resident,
                                               bool on, v3 o, v3 d, float& nearest, int& idx) {
    const float a = dot(d, d);                     // HK:308
    const float fa = 4.0f * a;                     // the (4*a) of HK:311
    const float ta = 2.0f * a;                     // HK:317
    nearest = 9999.0f;                             // RK:172
    idx = -1;
    for (uint32_t base = 0; base < n_spheres; base += kSphereChunk) {
        const uint32_t m = n_spheres - base < kSphereChunk ? n_spheres - base : kSphereChunk;
        if (!resident) {
            __syncthreads();                       // the previous chunk is done with
            stage_spheres(records, base, m, s_geo);
            __syncthreads();
        }
        if (on) {
            for (uint32_t k = 0; k < m; ++k) {
                const float4 g = s_geo[k];
                exact_full<false>(V(g.x, g.y, g.z), g.w, (int)(base + k), o, d, fa, ta, nearest, idx);
            }
        }
    }
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
    v3 color = V(1.0f, 1.0f, 1.0f);                // RK:103
    float dist = 0.0f;                             // RK:102
    float affect = 1.0f, sum = 0.0f;               // RK:111-112
    bool alive = live, missed = false;
    for (uint32_t bounce = 0; bounce < sc.bounces; ++bounce) {                       // RK:113
        if (!__syncthreads_or(alive)) break;       // no path left in the workgroup (the answer is every lane's: all leave together)
        float t, st;
        int idx, sidx;
        search_spheres(records, n_spheres, s_geo, resident, alive, ro, rd, t, idx);  // RK:114
        v3 normal = V(0.0f, 0.0f, 0.0f), sdir = V(0.0f, 0.0f, 0.0f), diffuse = V(0.0f, 0.0f, 0.0f);
        float distance = 0.0f;
        if (alive) {
            if (bounce == 0) dist = idx >= 0 ? t : 0.0f;                             // RK:116-118 (zero-initialised state)
            if (idx < 0) {                                                           // RK:122-126: sampled after the loop
                missed = true;
                alive = false;
            } else {
                const float* s = records + 8u * (size_t)idx;                         // the record of the winning index
                diffuse = V(s[4], s[5], s[6]);
                const v3 pos = add(ro, scale(t, rd));                                // HK:319 == RK:129
                normal = normalize(sub(pos, V(s[0], s[1], s[2])));                   // HK:320
                ro = pos;
                rd = normalize(reflect(rd, normal));                                 // RK:130
                sdir = normalize(sub(ro, sc.lightPos));                              // RK:147
                distance = length(sdir);                                             // RK:148
            }
        }
        search_spheres(records, n_spheres, s_geo, resident, alive, sc.lightPos, sdir, st, sidx);   // RK:153
        if (alive) {
            const float next = affect + sum;                                         // RK:120
            const float intensity = light_term(sc, ro, normal, sdir, distance, sidx >= 0, st);
            const v3 blended = scale(intensity, diffuse);                            // RK:133-135, diffuse.w == 1
            color = divs(add(scale(sum, color), scale(affect, blended)), next);      // RK:136
            affect = affect / 2.0f;                                                  // RK:139
            sum = next;                                                              // RK:140
        }
    }
    if (!live) return;
    shade_finish(A, sc, rays, flags, out, i, color, dist, missed, rd, affect, sum);
}

template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
static void launch_st(const RtFrameArgs& a, const RtTriScene& t, const float4* rays, uint32_t flags, float4* out, uint32_t n, hipStream_t s) {
    const uint32_t blocks = (uint32_t)(((size_t)n + kQueryThreads - 1u) / kQueryThreads);
    hipLaunchKernelGGL((shade_triangles<STK, PACKED, PAIRS, P16, INST>), dim3(blocks), dim3(kQueryThreads), 0, s, a, t, rays, flags, out, n);
}
template <bool INST>
static void launch_st_walk(const RtFrameArgs& a, const RtTriScene& t, const float4* rays, uint32_t flags, float4* out, uint32_t n, hipStream_t s) {
    if (t.n_nodes <= 65536u && t.packed_ok) launch_st<uint16_t, true, false, false, INST>(a, t, rays, flags, out, n, s);
    else if (t.n_nodes <= 65536u)          launch_st<uint16_t, false, false, false, INST>(a, t, rays, flags, out, n, s);
    else                                   launch_st<uint32_t, false, false, false, INST>(a, t, rays, flags, out, n, s);
}

}  // namespace rtk

// the forms of rt_launch_limited_triangles (rt_query.hip: launch_lt_form)
hipError_t rt_launch_shade_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const float4* rays, uint32_t flags, float4* out,
                                     uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const bool pairs = inst && t.pairs && t.n_nodes <= 65536u && t.packed_ok && t.n_blas <= rtk::kWideBlas;
    if (pairs && t.p16_ok) rtk::launch_st<uint16_t, true, true, true, true>(a, t, rays, flags, out, n, s);
    else if (pairs)        rtk::launch_st<uint16_t, true, true, false, true>(a, t, rays, flags, out, n, s);
    else if (inst)         rtk::launch_st_walk<true>(a, t, rays, flags, out, n, s);
    else                   rtk::launch_st_walk<false>(a, t, rays, flags, out, n, s);
    return hipGetLastError();
}

hipError_t rt_launch_shade_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags,
                                   float4* out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((size_t)n + rtk::kQueryThreads - 1u) / rtk::kQueryThreads);
    hipLaunchKernelGGL(rtk::shade_spheres, dim3(blocks), dim3(rtk::kQueryThreads), 0, s, a, records, n_spheres, rays, flags, out, n);
    return hipGetLastError();
}
