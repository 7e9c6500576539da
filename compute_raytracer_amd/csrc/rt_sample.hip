// rt_sample.hip -- supersampled frames on gfx950 (include/rt355.h: rt_render_samples, rt_render_samples_host): s x s camera rays per
// pixel, shaded as the renderer shades them and averaged on the chip, one RGBA8 pixel and / or one float pixel stored.  Sample
// (sx, sy) of pixel (x, y) is pixel (x s + sx, y s + sy) of an (s W) x (s H) target (RK:78-86): the kernels take a frame's
// arguments with W and H already multiplied (RtFrameArgs) and the frame's own size in RtSampleOut.  Compiled like rt_shade.hip with
// -ffp-contract=off -fno-slp-vectorize; the bounce loops and the end of a path are rt_shade.hip's own (rt_shade_device.h), so a
// sample is bit for bit the oracle's float pixel of the larger target (oracle/rt_oracle.c: shade_pixel).
//
// CDNA4 mapping: one sample per lane, wave64, kQueryWaves waves per workgroup.  The s*s samples of a pixel sit in adjacent lanes --
// nearly the same ray, so a wave stays in step -- and a workgroup covers P = 256 / (s*s) whole pixels (256, 64, 28, 16 for s = 1 .. 4;
// s = 3 leaves four lanes without a sample).  A lane builds its ray in registers (primary_dir: there is no ray buffer), runs the
// bounce loop, takes the sky and the compose of pixelColor and leaves its colour in LDS, 4 KB per workgroup; after one barrier the
// first P lanes add their pixel's samples in the order sy outer, sx inner -- acc = c[0]; acc = acc + c[1]; ... -- divide once by
// (float)(s*s) and store: a wave writes 256 B of bytes and / or 1 KB of floats in coalesced rows.  Nothing per sample reaches global
// memory.  Pixel indices are 64-bit: W H s*s may pass 2^32.
//   sample_triangles: path_triangles in the forms and with the LDS of shade_triangles.  Lanes without a sample skip the path and
//     wait at the reduction barrier (the traversal has no barrier of its own).
//   sample_spheres: path_spheres -- the literal loop over every sphere, for rt_query.hip's reason; a lane without a sample carries a
//     switched-off path through every barrier of the searches, as in shade_spheres.
#include <type_traits>

#include "rt_shade_device.h"

namespace rtk {

// the sample of this lane: its pixel (px, py) of the (s W) x (s H) target; false: the lane has none
__device__ __forceinline__ bool sample_of_lane(const RtSampleOut& O, uint32_t& px, uint32_t& py) {
    const uint32_t s2 = O.s * O.s, P = kQueryThreads / s2;
    const uint32_t lp = threadIdx.x / s2, sub = threadIdx.x - lp * s2;
    const uint64_t pix = (uint64_t)blockIdx.x * P + lp;
    if (lp >= P || pix >= (uint64_t)O.W * O.H) return false;
    const uint32_t y = (uint32_t)(pix / O.W), x = (uint32_t)(pix - (uint64_t)y * O.W);
    const uint32_t sy = sub / O.s, sx = sub - sy * O.s;
    px = x * O.s + sx;
    py = y * O.s + sy;
    return true;
}

// after the barrier: lane p < P resolves pixel blockIdx.x * P + p from s_col[p s*s ..] -- sequential adds, one division, RK:98
__device__ __forceinline__ void resolve_samples(const RtSampleOut& O, const float4* s_col) {
    const uint32_t s2 = O.s * O.s, P = kQueryThreads / s2;
    const uint64_t pix = (uint64_t)blockIdx.x * P + threadIdx.x;
    if (threadIdx.x >= P || pix >= (uint64_t)O.W * O.H) return;
    const float4* c = s_col + threadIdx.x * s2;
    v3 acc = V(c[0].x, c[0].y, c[0].z);
    for (uint32_t j = 1; j < s2; ++j) acc = add(acc, V(c[j].x, c[j].y, c[j].z));
    const v3 mean = divs(acc, (float)s2);
    if (O.rgba8) O.rgba8[pix] = unorm8(mean.x) | (unorm8(mean.y) << 8) | (unorm8(mean.z) << 16) | 0xFF000000u;
    if (O.rgbaf) O.rgbaf[pix] = make_float4(mean.x, mean.y, mean.z, 1.0f);
}

// STK / PACKED / PAIRS / P16 / INST as in shade_triangles
template <typename STK, bool PACKED, bool PAIRS, bool P16, bool INST>
__global__ __launch_bounds__(kQueryThreads) void sample_triangles(const RtFrameArgs A, const RtTriScene T, const RtQueryMask M, const RtSampleOut O) {
    typedef typename std::conditional<PACKED && !P16, uint32_t, STK>::type BSTK;
    constexpr uint32_t NODES = INST ? kWideNodes : kLdsNodes, BLAS = INST ? kWideBlas : kLdsBlas;
    __shared__ STK tstacks[kStack * kQueryThreads];
    __shared__ BSTK bstacks[kStack * kQueryThreads];
    __shared__ float4 s_nodes[2 * NODES];
    __shared__ float s_blas[20 * BLAS];
    __shared__ float4 s_col[kQueryThreads];
    const TriLds L = stage_head<kQueryWaves, NODES, BLAS, INST, /*ROOTS=*/false>(T, s_nodes, s_blas, &M);
    uint32_t px = 0, py = 0;
    if (sample_of_lane(O, px, py)) {               // (every lane reaches the barrier below)
        RtTriScene Tq = T;                         // (as in query_triangles: a node buffer wholly inside the staged head)
        if (INST && T.n_nodes <= L.n_nodes) Tq.nodes = s_nodes;
        const Scene sc = unpack_scene(A);
        const TriVis vis = {M.table, M.n, M.nearest};
        const PathEnd e = path_triangles<STK, PACKED, PAIRS, P16>(T, Tq, L, sc, sc.cameraPos, primary_dir(A, sc, px, py),
                                                                  tstacks + threadIdx.x, bstacks + threadIdx.x, vis);
        // (the fog colour: the sky along the primary ray, formed again rather than carried through the bounce loop)
        const v3 color = path_colour(A, sc, e, true, [&]() { return primary_dir(A, sc, px, py); });
        s_col[threadIdx.x] = make_float4(color.x, color.y, color.z, 0.0f);
    }
    __syncthreads();
    resolve_samples(O, s_col);
}

// (six waves per SIMD, shade_spheres' occupancy: left to itself the compiler spends 109 VGPRs here, four waves, and the every-sphere
// loop, which lives on waves to switch between, runs a quarter slower)
__global__ __launch_bounds__(kQueryThreads) __attribute__((amdgpu_waves_per_eu(6))) void sample_spheres(const RtFrameArgs A, const float* __restrict__ records, uint32_t n_spheres,
                                                                const RtSampleOut O) {
    __shared__ float4 s_geo[kSphereChunk];
    __shared__ float4 s_col[kQueryThreads];
    uint32_t px = 0, py = 0;
    const bool live = sample_of_lane(O, px, py);   // every lane stages and meets every barrier: no return before the last one
    const bool resident = n_spheres <= kSphereChunk;
    if (resident) {
        stage_spheres(records, 0u, n_spheres, s_geo);
        __syncthreads();
    }
    const Scene sc = unpack_scene(A);
    v3 rd = V(0.0f, 0.0f, 0.0f);
    if (live) rd = primary_dir(A, sc, px, py);
    const PathEnd e = path_spheres(records, n_spheres, s_geo, resident, sc, live, sc.cameraPos, rd);
    if (live) {
        const v3 color = path_colour(A, sc, e, true, [&]() { return primary_dir(A, sc, px, py); });
        s_col[threadIdx.x] = make_float4(color.x, color.y, color.z, 0.0f);
    }
    __syncthreads();
    resolve_samples(O, s_col);
}

static uint32_t sample_blocks(const RtSampleOut& o) {
    const uint64_t P = kQueryThreads / (o.s * o.s);
    return (uint32_t)(((uint64_t)o.W * o.H + P - 1u) / P);
}

}  // namespace rtk

static bool sample_args_ok(const RtFrameArgs& a, const RtSampleOut& o) {
    return o.s >= 1u && o.s <= RT355_MAX_SUPERSAMPLE && o.W && o.H && a.W == o.s * o.W && a.H == o.s * o.H && (o.rgba8 || o.rgbaf);
}

hipError_t rt_launch_sample_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtSampleOut& o, hipStream_t s) {
    const RtQueryMask& m = rt_query_mask_of(t);
    if (!sample_args_ok(a, o)) return hipErrorInvalidValue;
    rtk::query_form(t, inst, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((rtk::sample_triangles<typename F::STK, F::PACKED, F::PAIRS, F::P16, F::INST>), dim3(rtk::sample_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, t, m, o);
    });
    return hipGetLastError();
}

hipError_t rt_launch_sample_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtSampleOut& o, hipStream_t s) {
    if (!sample_args_ok(a, o)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtk::sample_spheres, dim3(rtk::sample_blocks(o)), dim3(rtk::kQueryThreads), 0, s, a, records, n_spheres, o);
    return hipGetLastError();
}
