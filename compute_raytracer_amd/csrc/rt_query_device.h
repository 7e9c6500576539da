// rt_query_device.h -- what the query kernels of rt_query.hip, rt_shade.hip, rt_gbuffer.hip and rt_ao.hip share: the workgroup shape,
// the size of a staged sphere chunk, the ray record, the pixel of a lane in the frame-shaped queries, and the form a triangle scene's
// kernel runs in.
#pragma once
#include "rt_device.h"
#include "rt_tri_device.h"
#include "rt_query_form.h"

namespace rtk {

constexpr int kQueryWaves = 4;
constexpr uint32_t kQueryThreads = 64u * kQueryWaves;
constexpr uint32_t kSphereChunk = 1024u;       // sphere records {centre, radius^2} staged per round: 16 KB of LDS

__device__ __forceinline__ void load_ray(const float4* __restrict__ rays, size_t i, v3& o, v3& d) {
    const float4 a = rays[2u * i], b = rays[2u * i + 1u];
    o = V(a.x, a.y, a.z);
    d = V(b.x, b.y, b.z);
}

// The frame-shaped queries (rt_gbuffer.hip, rt_ao.hip): one pixel per lane, a wave an 8 x 8 tile, a workgroup kQueryWaves tiles side
// by side, counted from the corner of the rectangle O.{x0, y0, w, h}.
#ifndef RT_GBUFFER_ROWS
constexpr uint32_t kGbufTileW = 8u * kQueryWaves, kGbufTileH = 8u;   // a workgroup's pixels: kQueryWaves 8 x 8 tiles in a row
#else                                                                // development builds (docs/experiments.md): a wave is 64 x 1 pixels
constexpr uint32_t kGbufTileW = kQueryThreads, kGbufTileH = 1u;
#endif

// the pixel of this lane, (x, y) within the rectangle; false: the lane has none
template <typename OUT>
__device__ __forceinline__ bool pixel_of_lane(const OUT& O, uint32_t& x, uint32_t& y) {
    const uint32_t cols = (O.w + kGbufTileW - 1u) / kGbufTileW;
    const uint32_t by = blockIdx.x / cols, bx = blockIdx.x - by * cols;
#ifndef RT_GBUFFER_ROWS
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    x = bx * kGbufTileW + wave * 8u + (lane & 7u);
    y = by * kGbufTileH + (lane >> 3);
#else
    x = bx * kGbufTileW + threadIdx.x;
    y = by;
#endif
    return x < O.w && y < O.h;
}
// the workgroups a launch over O's rectangle has
template <typename OUT>
inline uint64_t frame_blocks(const OUT& o) {
    return (uint64_t)((o.w + kGbufTileW - 1u) / kGbufTileW) * ((o.h + kGbufTileH - 1u) / kGbufTileH);
}

// f(RtQueryForm<STK, PACKED, PAIRS, P16, INST>()) for the form the scene `t` is queried in (rt_query_form.h holds the rule); inst:
// the instance data travels in t.inst
template <typename F>
inline void query_form(const RtTriScene& t, int inst, F&& f) {
    rt_query_form(inst != 0, t.pairs != nullptr, t.n_nodes, t.packed_ok != 0u, t.p16_ok != 0u, t.n_blas, kWideBlas, f);
}

}  // namespace rtk
