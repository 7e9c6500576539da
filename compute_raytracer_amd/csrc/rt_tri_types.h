// rt_tri_types.h -- device view of the reference's triangle scene, byte layouts of RR:169-229.
#pragma once
#include "rt_types.h"

// The frame's instance data (RR:169-192: the head of the node buffer = the top-level tree, the BLAS records, the BLAS lookup) as the
// SMALL forms of the triangle kernel take it: by value, in the kernel's own argument block -- what they stage in LDS, in the
// layout they stage it in (word 19 of record k: entry k of the lookup table; word 17: the root's relinked meta).  A frame of these
// forms reads nothing else of the per-frame buffers: no apply_instances kernel in front of it, no version of those buffers to wait for.
constexpr uint32_t kInstHeadNodes = 32u, kInstBlas = 16u;       // = rt_tri_device.h kWideNodes, kWideBlas: the most a small form stages
struct RtTriInst {
    float head[8u * kInstHeadNodes];
    float blas[20u * kInstBlas];
};

struct RtTriScene {
    const float4* nodes;       // [n_nodes][2]  {min.xyz, leftChildIndex}, {max.xyz, primitiveCount}
    const float* blas;         // [n_blas][20]  inverseModel (column-major), rootNodeIndex, pad
    const float* tri;          // [n_tri][40]   RR:198-209
    const float4* corners;     // [n_tri_lookup][3]  the library's own: cornerA/B/C of triangles[u32(tri_lookup[slot])] (rt_triangles.hip: tri_corners)
    const float* tri_lookup;   // [n_tri_lookup] f32 indices
    const float* blas_lookup;  // [n_blas_lookup] f32 indices
    const uint8_t* tex;        // meshTex, rgba8unorm
    uint32_t n_nodes, n_blas, n_tri, n_tri_lookup, n_blas_lookup, tex_w, tex_h;
    uint32_t packed_ok;        // every node's count, child index and lookup slot fits 16 bits: the BLAS stack may hold (count, left)
    uint32_t tlas_small;       // the host walked this frame's top-level tree (rt_tlas_fit.h): 1 = leaves at most 4 levels down, all nodes among
                               // the first 16; 2 = at most 3 levels, 8 nodes, 4 instances; 3 = at most 8 levels, 24 nodes; 4 = 8 levels, 32 nodes;
                               // 0 = none of these
    uint32_t p16_ok;           // ... and (count << 14 | x) fits 16: leaves of at most 3 triangles, at most 16,384 pair records and lookup slots
    // Work list (rt_triangles.hip: order_hist / order_scatter): tile_order[0] tiles are rendered as four quarters, tile_order[1] as
    // sixteen 2x2 blocks, tile_order[2...] is the order of the tiles (null: every tile whole, in index order); every workgroup
    // leaves the time it took in tile_cost[tile] by atomicMax -- the parts of a split tile: the longest of theirs, scaled (x 3 a
    // sixteenth, x 1.5 a quarter) -- (null: nowhere), from which the list of the next frame on this stream is made.
    // Relinked copy of the BLAS trees (rt_flow_build.h), when the scene fits it (rt_api.hip: flow_ok; null otherwise): the two
    // children of an inner node as one 64-byte record with packed (count << 16 | x) metas, and per instance the root's meta.
    const float4* pairs;
    uint32_t root_meta[16];    // instances the tile kernel stages (rt_tri_device.h: kLdsBlas; kWideBlas in the widest small form)
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    uint32_t form;             // the stack form rt_tri_stack_form chose for this frame (0 / 1 / 2 = SMALL of rt_triangles.hip); forms 1 and 2 read `inst`
    RtTriInst inst;
    uint32_t in_flight;        // the caller keeps frames in flight (rt_api.hip: pipelined_hint): throughput over latency
    unsigned long long* dbg;   // development builds (tools/tri_timeline.py): per workgroup {start, end (100 MHz ticks), tile << 8 | part}; null: off
    uint32_t prio;             // development builds: wave priority of the head of the work list (rt_triangles.hip)
    uint32_t roles;            // the frame's work list splits tiles (the caller knows from the pinned word order_hist leaves): forms 1 and 3 then run as trace_roles (rt_triangles.hip)
    uint32_t cost_mul4, cost_mul16;   // ... whose quarters / sixteenths leave their time x this / 8 in tile_cost
    uint32_t xcd_rows;         // set by the launch (no work list): workgroup b renders row (b % 8) + 8 (b / 8 / tiles per row) -- a row per XCD
};

// Instance visibility of a ray query (include/rt355.h: rt_write_instance_masks, rt_set_query_masks): the query kernels' own small
// argument -- no frame kernel takes it, and RtTriScene / RtTriInst hold none of it.  Instance bi (a BLAS record) is visible to a ray
// iff (mask of bi) & (mask of the ray) != 0.
struct RtQueryMask {
    const uint32_t* table;     // [n] the mask of record i, device memory (null with n == 0); records from n on: 0xFFFFFFFF
    uint32_t n;
    uint32_t nearest;          // the mask of every nearest-hit search of the call
    uint32_t occlusion;        // ... and of its any-hit searches (rt_occluded, the k rays of rt_render_ao)
};
// The scene of a ray query: what a frame's kernel takes, and the masks of the call beside it.  Every rt_launch_*_triangles function
// of the queries below is handed one of these through its `const RtTriScene& t` (rt_api.hip: Query::ts) -- the launch signatures
// are those of the unmasked queries -- and passes the two parts to its kernel as two arguments.
struct RtQueryScene : RtTriScene {
    RtQueryMask mask;
};
inline const RtQueryMask& rt_query_mask_of(const RtTriScene& t) { return static_cast<const RtQueryScene&>(t).mask; }

// Which stack form rt_launch_triangles runs the frame as: 0 twenty TLAS slots, 1 four (five waves per SIMD), 2 three (six waves),
// 3 eight (five waves), 4 eight with sixteen staged instances.  The caller stores the answer in t.form before the launch and, for
// 1 - 4, fills t.inst.
int rt_tri_stack_form(const RtTriScene& t, int heatmap);
hipError_t rt_launch_triangles(const RtFrameArgs& a, const RtTriScene& t, int heatmap, hipStream_t s);
uint32_t rt_order_scan_words(void);      // words of scan space rt_launch_order_tiles needs, zeroed once (it leaves them zero)
hipError_t rt_launch_order_hist(uint32_t* cost, uint32_t* scan, uint32_t* order, uint32_t n_tiles, uint32_t wave_slots,
                                unsigned long long* counters, unsigned long long* host, uint32_t words, unsigned long long* split_out,
                                hipStream_t s);   // (+ the frame's epilogue); split_out: pinned word that receives the number of tiles the list splits, or null
hipError_t rt_launch_order_scatter(uint32_t* cost, uint32_t* scan, uint32_t* order, uint32_t n_tiles, hipStream_t s);
hipError_t rt_launch_tri_corners(float4* out, const float* tri, const float* lookup, uint32_t n_slots, uint32_t n_tri, hipStream_t s);
// Ray queries (rt_query.hip; include/rt355.h: rt_trace_rays): rays [n][2] float4 {origin, -}, {dir, -}, hits [n][2] float4 (rt_hit).
// inst: the instance data travels in t.inst (stage_head<..., true>), as for the small forms; t.pairs only with inst.
// t: an RtQueryScene, in every triangle launch below: the instance masks and the ray masks of the call travel in its `mask` (with
// inst, word 18 of record k of t.inst.blas holds the mask of instance k).
hipError_t rt_launch_query_triangles(const RtTriScene& t, int inst, const float4* rays, float4* hits, uint32_t n, hipStream_t s);
hipError_t rt_launch_query_spheres(const float* records, uint32_t n_spheres, const float4* rays, float4* hits, uint32_t n, hipStream_t s);
// RT_QUERY_LIMITS in `flags`: (tmin, tmax) from ray words 3 and 7.  any: one byte per ray (rt_occluded), else rt_hit records
hipError_t rt_launch_limited_triangles(const RtTriScene& t, int inst, const float4* rays, uint32_t flags, bool any, void* out,
                                       uint32_t n, hipStream_t s);
hipError_t rt_launch_limited_spheres(const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags, bool any, void* out,
                                     uint32_t n, hipStream_t s);
// The k nearest hits (rt_trace_rays_multi), 1 <= k <= RT355_MAX_HITS: hits [n][k] rt_hit, sorted, then miss records
hipError_t rt_launch_multi_triangles(const RtTriScene& t, int inst, const float4* rays, uint32_t flags, uint32_t k, float4* hits,
                                     uint32_t n, hipStream_t s);
hipError_t rt_launch_multi_spheres(const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags, uint32_t k, float4* hits,
                                   uint32_t n, hipStream_t s);
// Shaded ray queries (rt_shade.hip; include/rt355.h: rt_shade_rays): out [n] float4 {r, g, b, dist}.  `a`: parameters, cube faces and
// sky flags as a frame's arguments hold them (nothing else of it is read); flags: RT_SHADE_COMPOSE.  inst as above.
hipError_t rt_launch_shade_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const float4* rays, uint32_t flags, float4* out,
                                     uint32_t n, hipStream_t s);
hipError_t rt_launch_shade_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const float4* rays, uint32_t flags,
                                   float4* out, uint32_t n, hipStream_t s);
// Supersampled frames (rt_sample.hip; include/rt355.h: rt_render_samples): the W x H frame at s x s samples per pixel, resolved in the
// kernel.  `a` as for the shaded queries, with a.W = s W and a.H = s H -- the target whose pixels the samples are -- and the camera
// words of a.p read; either output may be null, not both.  inst as above.
struct RtSampleOut {
    uint32_t W, H, s;
    uint32_t* rgba8;           // [H][W] rgba8unorm, row 0 at the top
    float4* rgbaf;             // [H][W] {r, g, b, 1}
};
hipError_t rt_launch_sample_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtSampleOut& o, hipStream_t s);
hipError_t rt_launch_sample_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtSampleOut& o, hipStream_t s);
// Geometry frames (rt_gbuffer.hip; include/rt355.h: rt_render_gbuffer): the nearest hit of the primary ray of every pixel of o's
// rectangle, as planes.  `a`: the camera words of a.p and a.W = o.W, a.H = o.H (nothing else of it is read).  inst as above.
hipError_t rt_launch_gbuffer_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtGbufferOut& o, hipStream_t s);
hipError_t rt_launch_gbuffer_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtGbufferOut& o, hipStream_t s);
// Ambient-occlusion frames (rt_ao.hip; include/rt355.h: rt_render_ao): per pixel of o's rectangle how many of o.k any-hit rays from
// the primary ray's hit point are occluded.  `a` and inst as for the geometry frames.
hipError_t rt_launch_ao_triangles(const RtFrameArgs& a, const RtTriScene& t, int inst, const RtAoOut& o, hipStream_t s);
hipError_t rt_launch_ao_spheres(const RtFrameArgs& a, const float* records, uint32_t n_spheres, const RtAoOut& o, hipStream_t s);
// Closest-point queries (rt_closest.hip; include/rt355.h: rt_closest_points): points [n] float4 {x, y, z, radius}, out [n][2] float4
// (rt_closest).  cst: 16 words per BLAS record of t, written by a kernel of the launch in front of the search.  inst as above.
hipError_t rt_launch_closest_points(const RtTriScene& t, int inst, float* cst, const float4* points, float4* out, uint32_t n, hipStream_t s);
// rt_api.hip reaches that launch through this pointer, which rt_closest.o sets while the library is loaded (null until then): rt_api.o
// names no symbol of rt_closest.o, so a host-only program that links rt_api.o for the frame path alone (tests/c/enqueue_trace.cpp)
// needs no stand-in for a launch no frame makes.  A null pointer at a call is an error, never a silent miss.
typedef hipError_t (*RtClosestLaunch)(const RtTriScene&, int, float*, const float4*, float4*, uint32_t, hipStream_t);
extern RtClosestLaunch rt_closest_launch;
hipError_t rt_launch_pick_rays(const RtFrameArgs& a, const uint32_t* xy, float4* rays, uint32_t n, hipStream_t s);   // xy: [n][2] u32
