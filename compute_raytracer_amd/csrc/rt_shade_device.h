// rt_shade_device.h -- what the kernels of rt_shade.hip (caller rays) and rt_sample.hip (camera samples) share: rayColor's bounce
// loop (RK:101-144) over a triangle scene and over a sphere scene, and the end of a path -- the sky it escaped into (RK:122-125)
// and pixelColor on top of it (RK:91-96).  Every expression in the oracle's order (oracle/rt_oracle.c: ray_color, shade_pixel); the
// including file is compiled with -ffp-contract=off -fno-slp-vectorize.
#pragma once
#include "rt_device.h"
#include "rt_tri_types.h"
#include "rt_tri_device.h"
#include "rt_filter.h"
#include "rt_query_device.h"

namespace rtk {

// a path when its bounce loop ends
struct PathEnd {
    v3 color;                  // RK:103, the running mean
    float dist;                // RK:102: 0 unless the first ray hits (RK:116-118)
    bool missed;               // the loop ended on a miss: the sky along `rd` is still to be mixed in
    v3 rd;
    float affect, sum;         // RK:111-112
};

// RK:122-125 for a path that escaped along e.rd, then RK:91-96 under `compose`, the fog colour being the sky along fog_dir() --
// asked for only when it is needed.  One copy of the cube filter serves both samples.
template <typename DIR>
__device__ __forceinline__ v3 path_colour(const RtFrameArgs& A, const Scene& sc, const PathEnd& e, bool compose, DIR fog_dir) {
    v3 color = e.color;
    v3 fog = V(0.0f, 0.0f, 0.0f);
    v3 dir = e.rd;
#pragma unroll 1
    for (int k = e.missed ? 0 : 1; k < (compose ? 2 : 1); ++k) {
        if (k == 1) dir = fog_dir();
        const v3 sky = scale(sc.minIntensity, cube_sample(A, dir));        // RK:123 / RK:92
        if (k == 0) color = divs(add(scale(e.sum, color), scale(e.affect, sky)), e.affect + e.sum);   // RK:120, 124
        else fog = sky;
    }
    if (compose) color = compose_color_sky(fog, color, e.dist);            // RK:94-96
    return color;
}

// The bounce loop of trace_triangles (rt_triangles.hip) without tiles, work list, ray counters or parking: per bounce trace_tlas
// along the path, the hit's normal, albedo and texture sample, the reflection, trace_tlas from the light, the shadow test, the
// running mean.  Tq: T, or T with the staged node buffer (query_triangles); the stacks are the lane's own, slot-major.  vis: what the
// path rays and the shadow rays alike may see -- RK:147-165 is a nearest-hit search too.
template <typename STK, bool PACKED, bool PAIRS, bool P16, typename BSTK>
__device__ __forceinline__ PathEnd path_triangles(const RtTriScene& T, const RtTriScene& Tq, const TriLds& L, const Scene& sc, v3 ro, v3 rd,
                                                  STK* tstack, BSTK* bstack, const TriVis& vis) {
    float dummy = 0.0f;
    v3 color = V(1.0f, 1.0f, 1.0f);                // RK:103
    float dist = 0.0f;                             // RK:102: 0 unless the first ray hits (RK:116-118)
    float affect = 1.0f, sum = 0.0f;               // RK:111-112
    bool missed = false;
    for (uint32_t bounce = 0; bounce < sc.bounces; ++bounce) {                       // RK:113
        const TriHit h = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, ro, rd, tstack, bstack, kQueryThreads, dummy, 0.0f, 0.0f, &vis);   // RK:114
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
        const TriHit sh = trace_tlas<false, STK, PACKED, PAIRS, P16>(Tq, L, sc.lightPos, sdir, tstack, bstack, kQueryThreads, dummy, 0.0f, 0.0f, &vis);   // RK:153
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
    PathEnd e = {color, dist, missed, rd, affect, sum};
    return e;
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

// The bounce loop over a sphere scene: the literal search for the path ray and the shadow ray.  EVERY lane of the workgroup calls
// it and meets every barrier, lanes without a ray (`live` false: a switched-off path) and lanes whose path has ended included; the
// workgroup leaves the loop when none of its lanes has a path left.
__device__ __forceinline__ PathEnd path_spheres(const float* __restrict__ records, uint32_t n_spheres, float4* s_geo, bool resident,
                                                const Scene& sc, bool live, v3 ro, v3 rd) {
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
    PathEnd e = {color, dist, missed, rd, affect, sum};
    return e;
}

}  // namespace rtk
