// rt_ctx.h -- the context behind the C ABI, shared by rt_api.hip (single-GPU entry points) and
// rt_comm.hip (the RCCL group entry points).  Private to the library.
#pragma once
#include "../../include/rt355.h"
#include "rt_types.h"
#include "rt_tri_types.h"
#include "rt_flow_build.h"
#include "rt_own.h"

#include <cstdio>
#include <string>
#include <vector>

extern thread_local std::string g_rt_err;      // rt_last_error()

inline int fail(int code, const char* what) {
    g_rt_err = what;
    return code;
}
inline int fail_hip(hipError_t e, const char* where) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
    g_rt_err = buf;
    return RT_ERR_HIP;
}
#define RT_HIP(call)                                                   \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return fail_hip(e_, #call);              \
    } while (0)

// Frames the library itself keeps concurrent (rt_render rotates over this many streams and colour
// buffers).  Why: at the end of a frame every lane of the persistent hierarchy kernel still carries
// a path of up to 2*bounces dependent rays; that tail is latency, not work (0.45 ms of a 2.9 ms C3
// frame, 0.45 of 0.8 ms when 8 ranks share the frame).  Frames in flight each take a share of the
// chip (RtFrameArgs::grid_share), so one frame's tail runs beside the others' bulk.
constexpr int kStreams = 4;
constexpr int kVersions = 4;         // versions of the per-frame instance buffers (>= kStreams)
constexpr uint32_t kHeadNodes = 31u; // TLAS nodes (2 M - 1 for M <= 16 instances) that travel with a frame
constexpr uint32_t kInstMax = 16u;   // instances whose records travel with a frame
constexpr uint32_t kOrderMinTiles = 4096u;   // frames of fewer tiles than the chip has wave slots start all of them at once: no order to choose
constexpr size_t kCounterBytes = (size_t)RT_RAY_COUNTERS * RT_RAY_COUNTER_STRIDE;   // partial ray counters of one frame
constexpr size_t kCtrlBytes = kCounterBytes + 32u;                                   // + the 32-byte control block

struct rt_comm_state;   // rt_comm.hip

// Ownership (rt_own.h): every device buffer, pinned buffer, event and stream below is a DevBuf, PinnedBuf, Event or Stream, and
// `delete c` releases it -- rt_destroy names none of them.  Members are destroyed in reverse order of declaration, so the
// streams are declared first, the events next and the buffers after them: buffers go first, then events, streams last, as
// rt_destroy released them by hand.  A raw hipStream_t / hipEvent_t / pointer member owns nothing: it names one of these.
struct rt_ctx {
    using DevBuf = ::DevBuf;
    int device = 0;
    // ---- streams (destroyed last) ----
    Stream streams[kStreams];            // rt_render rotates: consecutive frames may overlap on the device
    Stream copy_stream;                  // streaming read-back (rt_read_pixels_async)
    Stream query_stream;                 // the host-memory ray queries, made at their first use
    hipStream_t stream = nullptr;        // uploads, read-back, and frames 0, 3, 6 ... of rt_render (= streams[0])
    // ---- events (destroyed before the streams) ----
    Event ev_prep0[RT355_MAX_IN_FLIGHT], ev_k0[RT355_MAX_IN_FLIGHT], ev_k1[RT355_MAX_IN_FLIGHT];
    Event ev_done[RT355_MAX_IN_FLIGHT];  // behind the frame's epilogue kernel: what rt_wait waits for
    Event ev_scene;                      // the scene arrays / hierarchy a frame reads are complete ...
    hipStream_t scene_stream = nullptr;  // ... recorded on this stream
    Event ev_copy[kStreams];             // per colour buffer: the last streaming copy out of it
    Event ev_ver[kVersions];             // behind the apply_instances kernel that last brought the version up to date (made at first use) ...
    hipStream_t ver_stream[kVersions] = {nullptr};   // ... on this stream
    Event ev_query;                      // behind the latest ray query on any stream (made at first use)
    // ---- state and buffers (the buffers are destroyed first) ----
    uint32_t in_flight = 0;              // frames enqueued since the last rt_wait
    hipStream_t slot_stream[RT355_MAX_IN_FLIGHT] = {nullptr};   // the stream each of them was enqueued on
    uint32_t frames_rendered = 0;        // rt_render calls: selects the colour buffer
    uint32_t stream_rot = 0;             // the stream rt_render enqueues on: advances only while frames are in flight
    bool pipelined_hint = false;         // the last rt_wait completed frames on MORE THAN ONE of the library's own streams
                                         // (rt_render / rt_render_gather back to back): the caller keeps frames in flight
    uint32_t W = 0, H = 0;
    uint32_t rank = 0, world = 1;
    float params[24] = {0};
    bool have_params = false;
    bool prep_spheres_valid = false;     // prep_spheres ran since the last rt_write_spheres
    bool prep_params_valid = false;      // ... and since the last rt_write_params (camera / light records)
    DevBuf d_records;                    // n x 32 B as written
    uint32_t n = 0, cap_n = 0;           // cap_n: spheres d_records AND d_scene both hold (0 until both allocations succeeded)
    bool have_spheres = false;
    DevBuf d_scene;                      // 8 float4 arrays of n16: geo lgt cam col geo_f lgt_f cam_f + {geo_w,lgt_w,cam_w,-}
    uint32_t n16 = 0;                    // n rounded up to a multiple of 16
    float scene_bound = 0.0f;            // max over spheres of |center| + radius (host side)
    double scene_min_radius = 0.0;       // smallest non-zero |radius| (rt_plan: the rescaled sign-aware test)
    // bounding-sphere hierarchy (rt_bvh.hip): host copy of the records it is built from, the
    // build result and its device copy
    std::vector<float> h_records;
    std::vector<float> h_bvh_rec;
    std::vector<uint32_t> h_bvh_link;
    DevBuf d_bvh_rec, d_bvh_link;        // float4 and uint32_t per node; allocated together, the link array last: its cap is the capacity of both
    uint32_t bvh_nodes = 0;
    bool bvh_valid = false;              // the device records bound the current spheres
    uint32_t bvh_topo_n = 0;             // sphere count the device topology (links, leaf ids) was built for; 0: none
    struct rt_rebuild* rebuild = nullptr;   // worker thread that rebuilds the topology for moved spheres (rt_api.hip)
    DevBuf d_face[6];
    uint32_t fw[6] = {0, 0, 0, 0, 0, 0}, fh[6] = {0, 0, 0, 0, 0, 0};
    uint32_t face_texel0[6] = {0, 0, 0, 0, 0, 0};   // first texel (rgb) of each face: a one-texel sky of one colour is "flat"
    uint8_t* d_out = nullptr;              // colour buffer of the LATEST rt_render: points into d_outs or into a gather buffer, owns nothing
    DevBuf d_outs[kStreams];
    // streaming read-back (rt_read_pixels_async): copy_stream, per colour buffer ev_copy and the
    // event slot of the frame of the current batch that renders into it (-1: none in flight)
    bool copy_pending[kStreams] = {false};
    int buf_slot[kStreams] = {-1, -1, -1, -1};
    DevBuf d_fin[kStreams];                      // end-of-path records of frames with a textured sky (rt_bvh.hip: sky_resolve), lazily;
                                                 // allocated together, the last one last: its cap is the capacity of each
    size_t out_bytes = 0;                        // bytes of each of d_outs once all are allocated and zeroed (rt_device_pixels reports it)
    // per frame in flight: RT_RAY_COUNTERS partial ray counters (kCtrlBytes - 32 bytes), then a 32-byte
    // control block: unused u64, queue count, queue head, pixel / tile-pair cursor
    DevBuf d_rays;
    DevBuf d_queue;                        // path queue of the two-kernel pipeline
    size_t queue_cap = 0;                  // entries (48 B each): what a frame's arguments carry
    unsigned long long* h_split = nullptr; // behind h_rays (points into it), per stream: the number of tiles the stream's current work list renders in parts (order_hist writes it)
    PinnedBuf h_rays;                      // pinned, device-visible: per frame in flight {rays, fault word}, written by the frame's epilogue kernel
    // the reference's triangle scene (RR:169-229), device copies in the reference's byte layouts
    DevBuf d_tri, d_tri_lookup, d_tex;
    DevBuf d_corners;                            // 48 B per lookup slot: the corners hitTriangle reads, in lookup order (tri_corners)
    bool corners_valid = false;                  // ... built since the last rt_write_triangles / rt_write_tri_lookup
    // Tile order of the triangle kernel (rt_triangles.hip: order_tiles), one set per stream of rt_render: the time every
    // tile of the stream's last frame took, and the longest-first permutation made of it for the stream's next frame.
    DevBuf d_tile_cost[kStreams], d_tile_order[kStreams];   // cap: the bytes of the costs / the list; order_tiles' scan words lie behind them
    uint32_t wave_slots = 4096;                      // waves of the triangle kernel the device holds at once
    uint32_t order_tiles[kStreams] = {0, 0, 0, 0};   // tile count d_tile_order[k] is a permutation of (0: none yet)
    // The buffers the reference rewrites before every frame (RR:169-192: BLAS records, BLAS lookup, the TLAS nodes at
    // the head of the node buffer) exist in kVersions versions: a frame in flight keeps reading the version it was
    // enqueued with while the host already writes the next state (rt_api.hip: apply_instances).
    DevBuf d_nodes[kVersions], d_blas[kVersions], d_blas_lookup[kVersions];
    struct {
        std::vector<float> head, blas, lookup;   // current contents: first head_nodes nodes, BLAS records, BLAS lookup
        uint32_t head_nodes = 0;                 // extent of the node buffer's head that per-frame writes have touched
        bool blas_on = false, lookup_on = false; // the last write of that buffer was a per-frame (small) one
        uint64_t gen = 0;                        // bumped by every per-frame write
    } inst;
    uint64_t inst_gen_carried = 0;               // inst.gen the last frame of a small form took along in its arguments (rt_stats.instance_uploads)
    uint64_t ver_gen[kVersions] = {0, 0, 0, 0};  // inst.gen each device version holds
    size_t nodes_used = 0;                       // bytes of the node buffer written so far (any version)
    uint32_t node_count_max = 0;                 // largest u32(primitiveCount) of any node written so far (packed BLAS stack: <= 65535)
    // The triangle kernel reads the BLAS trees from the library's relinked copy (rt_flow_build.h: pair records) where the scene
    // fits it: built on the host from a mirror of the node buffer, when a frame first needs it or a write has touched what it
    // was built from.
    std::vector<float> h_nodes;                  // mirror of the node buffer (every rt_write_nodes lands here too)
    RtFlow flow;
    bool flow_dirty = true;
    uint32_t flow_frames_since = 0, flow_streak = 0, flow_cooldown = 0;   // frames since the last rebuild; consecutive frames that rebuilt; frames left on the node walk
    DevBuf d_flow;                               // the pair records
    // Deforming meshes (rt_refit_blas; rt_refit_plan.h, rt_refit.hip): the plan of the last refit, kept while nothing it was
    // made from has changed -- the roots asked for, the tree structure in the mirror, the size of the lookup table -- and its
    // device copy, which also names the pair records holding a copy of each planned node (valid for one build of the records).
    uint64_t topo_gen = 1;                       // bumped by every node write that changes a child index, a count or the node count
    uint64_t flow_gen = 0;                       // bumped by every rebuild of the pair records
    struct {
        std::vector<uint32_t> roots, plan;       // sorted unique roots; {node, first_slot, n_slots} per planned node
        uint64_t topo_gen = 0;                   // 0: no plan
        uint32_t n_tri_lookup = 0;
        uint32_t lo = 0, hi = 0;                 // the planned nodes lie in [lo, hi]
        bool on_device = false;                  // d_refit_plan holds this plan ...
        bool with_pairs = false;                 // ... with the pair halves of build `flow_gen` of the records (or without any)
        uint64_t flow_gen = 0;
    } refit;
    DevBuf d_refit_plan;
    DevBuf d_build;                              // scratch of rt_build_blas (rt_build.h: RtBuildArgs), kept between calls
    DevBuf d_deform;                             // staging of rt_deform_triangles_host: vertices, faces, normals; kept between calls
    DevBuf d_tri_dbg;                            // development builds: the triangle kernel's per-workgroup timeline
    // Ray queries (rt_trace_rays_host / rt_pick): query_stream, staging buffers that grow as needed, and ev_query behind the
    // latest query on any stream -- scene writes wait for it as they wait for the frames in flight (rt_drain)
    DevBuf d_qrays, d_qhits, d_qxy;
    DevBuf d_closest;                    // closest-point queries: 16 words per BLAS record, remade by every call on its stream (rt_closest.hip: closest_inst)
    bool query_pending = false;
    bool query_versions = false;         // ... and that query (or one before it since the last drain) read a version of the per-frame buffers
    hipStream_t query_last = nullptr;    // the stream of that query
    // Instance visibility masks (rt_write_instance_masks, rt_set_query_masks): one 32-bit mask per BLAS record, by record index,
    // whatever the record count is or becomes; records beyond the table have 0xFFFFFFFF.  The host copy rides in word 18 of the
    // records a query carries in its arguments (tri_fill_inst); the device copy is what the query kernels read for every other
    // record.  No frame reads either.
    std::vector<uint32_t> h_masks;
    DevBuf d_masks;                      // used: 4 bytes per entry of h_masks
    uint32_t mask_nearest = 0xFFFFFFFFu, mask_occlusion = 0xFFFFFFFFu;   // the ray masks the next query call copies
    uint32_t n_cus = 256;
    uint32_t tex_w = 0, tex_h = 0;
    int scene_kind = 0;                    // 0 spheres, 1 triangles: the primitive type written last
    int mode = RT_MODE_FAST;
    int variant = 0;
    int kernel = RT_KERNEL_RAYTRACER;
    rt_stats stats = {};
    rt_comm_state* comm = nullptr;         // RCCL communicator + gather buffers (rt_comm_init / rt_group_create)
};

// rt_api.hip (defined inside its extern "C" block; not exported through include/rt355.h)
#define RT_INTERNAL __attribute__((visibility("hidden")))
extern "C" {
RT_INTERNAL int rt_enqueue(rt_ctx* c, uint8_t* dst, hipStream_t s);   // prep + ray-trace launches of one frame into `dst` on `s`
RT_INTERNAL int rt_order_colour_buffer(rt_ctx* c, uint32_t k, hipStream_t st);   // before a frame on `st` writes colour buffer k
RT_INTERNAL void rt_default_hw_queues(void);                          // GPU_MAX_HW_QUEUES=8 unless the host set it: before the first HIP call
RT_INTERNAL int rt_drain(rt_ctx* c);                                  // waits for the frames in flight
RT_INTERNAL uint32_t rt_local_tiles(const rt_ctx* c);
RT_INTERNAL void rt_abandon_in_flight(rt_ctx* c);                     // after a communicator abort: forget the frames in flight
}
// rt_comm.hip
RT_INTERNAL void rt_comm_release(rt_ctx* c);                          // called by rt_destroy
RT_INTERNAL int rt_comm_after_wait(rt_ctx* c);                        // called by rt_wait once the frames in flight are complete
RT_INTERNAL int rt_comm_wait_frames(rt_ctx* c);                       // called by rt_wait: polls the frames' events and the communicator


