// rt_api.hip -- host side of librt355.so: the C ABI declared in include/rt355.h.
// One context = one GPU + four streams (frames in flight); see the header for what each entry point replaces in
// the reference's renderer-raytracing.ts.  No CPU fallback: without a gfx950 device
// rt_create fails and nothing else can be called.
#include "rt_ctx.h"

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt_bvh_build.h"
#include "rt_refit.h"
#include "rt_refit_plan.h"
#include "rt_build.h"
#include "rt_tlas_build.h"
#include "rt_tlas_fit.h"
#include "rt_closest.h"
#include "rt_deform.h"

thread_local std::string g_rt_err;
thread_local int g_rt_kernel_id = 0;
thread_local int g_rt_tri_form = 0;

#ifndef RT355_BUILD_ID
#define RT355_BUILD_ID "unknown"
#endif

// children per inner node of the sphere hierarchy (rt_bvh_build.h); development builds read it from the environment
static uint32_t rt_bvh_arity() {
#ifdef RT355_DEV_EXPORTS
    if (const char* e = getenv("RT355_BVH_ARITY")) return (uint32_t)atoi(e);
#endif
    return 4u;
}

// Rebuilds the hierarchy's topology for moved spheres off the caller's thread.  rt_write_spheres with an
// unchanged sphere count posts the new records here; frames meanwhile use the OLD topology with node
// bounds refitted on the device (rt_bvh.hip: bvh_refit) -- always valid, only looser as spheres drift --
// and the next frame that follows a sphere write after the worker has finished takes the new one.
struct rt_rebuild {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool stop = false, pending = false, ready = false;
    std::vector<float> in_records;            // job (latest posted wins)
    uint32_t in_n = 0;
    std::vector<float> out_rec;               // result
    std::vector<uint32_t> out_link;
    uint32_t out_n = 0, out_nodes = 0;

    void run() {
        std::vector<float> records, rec;
        std::vector<uint32_t> link;
        for (;;) {
            uint32_t n;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || pending; });
                if (stop) return;
                records.swap(in_records);
                n = in_n;
                pending = false;
            }
            const uint32_t nodes = rt_bvh_build(records.data(), n, rec, link, rt_bvh_arity());
            std::lock_guard<std::mutex> lk(m);
            out_rec.swap(rec);
            out_link.swap(link);
            out_n = n;
            out_nodes = nodes;
            ready = true;
        }
    }
    void post(const float* records, uint32_t n) {
        {
            std::lock_guard<std::mutex> lk(m);
            in_records.assign(records, records + 8u * (size_t)n);
            in_n = n;
            pending = true;
        }
        if (!th.joinable()) th = std::thread([this] { run(); });
        cv.notify_one();
    }
    ~rt_rebuild() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

namespace {

uint32_t tiles_total(uint32_t H) { return (H + 7u) / 8u; }

// max(scene bound, |camera|, |light|) with a sticky NaN: any NaN operand makes the reach NaN, which
// switches both filter forms off (enqueue)
double rt_reach(double bound, double cam, double lgt) {
    if (bound != bound || cam != cam || lgt != lgt) return NAN;
    return std::max(bound, std::max(cam, lgt));
}

// max over spheres of |center| + |radius|.  A NaN anywhere is sticky -- the bound of a scene with a
// NaN record is NaN whatever the record's position --, an infinite record gives +inf.
double rt_scene_bound(const float* records, uint32_t n) {
    double bound = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = records + 8u * (size_t)i;
        const double len = std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2]) + std::fabs((double)r[7]);
        if (len != len || bound != bound) bound = NAN;
        else if (len > bound) bound = len;
    }
    return bound;
}

// Which filter forms a frame may use.  reach: bound on |ray origin| and on |center| + radius.  The
// sign-aware filter is valid only while the rounding of h.oc (<= 7.3e-7 |oc|, |oc| <= 2*reach) stays
// below half of the 0.001 a valid hit needs (rt_filter.h: filter_one); beyond 2^20 (or NaN / inf) the
// 2^40-scaled filter arithmetic could overflow, and the frame is rendered by the literal kernel.
// smallest non-zero |radius| (+inf if there is none): the sign-aware forms rescale the test by 2^-124, which
// must not push the quantities that decide it into the denormals; with every radius 0 or >= 2^-30 the
// filter's margins (>= 2^-16 r^2) stay 40 binary orders above the smallest normal number
double rt_scene_min_radius(const float* records, uint32_t n) {
    double mn = INFINITY;
    for (uint32_t i = 0; i < n; ++i) {
        const double r = std::fabs((double)records[8u * (size_t)i + 7u]);
        if (r > 0.0 && r < mn) mn = r;
    }
    return mn;
}

void rt_plan(double scene_bound, double min_radius, const float* p, bool& filter_ok, uint32_t& signed_filter) {
    const double cam = std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
    const double lgt = std::sqrt((double)p[16] * p[16] + (double)p[17] * p[17] + (double)p[18] * p[18]);
    // the camera's basis vectors (forwards, right, up: p[4..6], p[8..10], p[12..14]) bound the primary directions the same
    // way: below 2^20 the squared length of fw + hc rt + vc up cannot overflow, so normalize() never returns the zero
    // vector (rt_bvh.hip: flat_sky relies on it); a NaN or absurd basis sends the frame to the literal kernel
    double basis = 0.0;
    for (int k = 4; k < 15; ++k)
        if (k % 4 != 3) { const double a = std::fabs((double)p[k]); basis = (a != a || basis != basis) ? NAN : std::max(basis, a); }
    const double reach = rt_reach(scene_bound, cam, basis != basis ? (double)NAN : std::max(lgt, basis));   // std::max keeps a NaN first operand
    filter_ok = reach == reach && reach < 1048576.0;
    signed_filter = (filter_ok && 2.0 * reach * 7.3e-7 < 5.0e-4 && min_radius >= 9.313225746154785e-10) ? 1u : 0u;   // 2^-30
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT355_ABI_VERSION; }

const char* rt_build_id(void) { return RT355_BUILD_ID; }

const char* rt_kernel_name(int id) {
    switch (id) {
        case RT_KID_LITERAL: return "trace_pixels<literal>";
        case RT_KID_BRUTE_SINGLE: return "trace_pixels<filter>";
        case RT_KID_BRUTE_PIPELINE: return "first_bounce+trace_paths";
        case RT_KID_HIERARCHY_8: return "bvh_pixels<8>";
        case RT_KID_HIERARCHY_12: return "bvh_pixels<12>";
        case RT_KID_HIERARCHY_16: return "bvh_pixels<16>";
        case RT_KID_HIERARCHY_GLOBAL: return "bvh_pixels<global>";
        case RT_KID_TRIANGLES: return "trace_triangles";
        case RT_KID_HEATMAP: return "heatmap_triangles";
        case RT_KID_TRIANGLES_ROLES: return "trace_roles";
        default: return "none";
    }
}

const char* rt_last_error(rt_ctx*) { return g_rt_err.c_str(); }

// A context keeps four frames in flight on four streams, next to its copy stream and RCCL's: with the HIP runtime's default of
// four hardware queues per device several of them share a queue and serialise (C3 through the N > 1 path: 3.67 instead of
// 2.43 ms per frame, round 2).  The runtime reads GPU_MAX_HW_QUEUES once, when it initialises -- at the process's first HIP
// call --, so the library asks for eight before ITS first HIP call, unless the host has set the variable itself
// (RT355_KEEP_HW_QUEUES=1: leave the runtime's default alone).  A host that has initialised HIP before it creates its first
// context keeps what its runtime read then.
void rt_default_hw_queues(void) {
    static bool done = false;
    if (done) return;
    done = true;
    if (!getenv("RT355_KEEP_HW_QUEUES")) (void)setenv("GPU_MAX_HW_QUEUES", "8", 0);
}

int rt_create(int device, rt_ctx** out) {
    if (!out) return fail(RT_ERR_INVALID_ARG, "rt_create: out is NULL");
    *out = nullptr;
    rt_default_hw_queues();
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(RT_ERR_NO_DEVICE, "rt_create: no HIP device visible (this library has no CPU path)");
    }
    if (device < 0 || device >= count) return fail(RT_ERR_NO_DEVICE, "rt_create: device ordinal out of range");
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "rt_create: device %d is %s; librt355 carries gfx950 code only", device,
                      prop.gcnArchName);
        return fail(RT_ERR_NO_DEVICE, buf);
    }
    RT_HIP(hipSetDevice(device));
    rt_ctx* c = new (std::nothrow) rt_ctx();
    if (!c) return fail(RT_ERR_HIP, "rt_create: out of host memory");
    c->device = device;
    c->n_cus = (uint32_t)prop.multiProcessorCount;
    c->wave_slots = (uint32_t)prop.multiProcessorCount * 20u;      // 4 SIMDs x 5 waves: the form of the triangle kernel that awaited frames -- the ones with a work list -- run (rt_launch_triangles)
    hipError_t err;
    err = hipSuccess;
    for (int k = 0; k < kStreams && err == hipSuccess; ++k) err = c->streams[k].ensure(hipStreamNonBlocking);
    c->stream = c->streams[0];
    if (err == hipSuccess) err = c->ev_scene.ensure(hipEventDisableTiming);
    if (err == hipSuccess) err = c->copy_stream.ensure(hipStreamNonBlocking);
    for (int k = 0; k < kStreams && err == hipSuccess; ++k) err = c->ev_copy[k].ensure(hipEventDisableTiming);
    for (int i = 0; i < RT355_MAX_IN_FLIGHT && err == hipSuccess; ++i) {
        if ((err = c->ev_prep0[i].ensure()) != hipSuccess) break;
        if ((err = c->ev_k0[i].ensure()) != hipSuccess) break;
        if ((err = c->ev_k1[i].ensure()) != hipSuccess) break;
        err = c->ev_done[i].ensure(hipEventDisableTiming);
    }
    if (err != hipSuccess ||
        (err = c->d_rays.replace(kCtrlBytes * RT355_MAX_IN_FLIGHT)) != hipSuccess ||
        (err = hipMemset(c->d_rays.p, 0, kCtrlBytes * RT355_MAX_IN_FLIGHT)) != hipSuccess ||
        (err = c->h_rays.replace(16u * RT355_MAX_IN_FLIGHT + 8u * kStreams)) != hipSuccess) {
        rt_destroy(c);
        return fail_hip(err, "rt_create: stream/event/counter setup");
    }
    std::memset(c->h_rays.p, 0, 16u * RT355_MAX_IN_FLIGHT + 8u * kStreams);
    c->h_split = c->h_rays.as<unsigned long long>() + 2u * RT355_MAX_IN_FLIGHT;
    // An event's FIRST record allocates its signal (~10 us each, measured through bench.py's first timed region: 0.25 ms for twelve
    // untouched slots): every event of the ring is recorded once here, so that a host's first frames do not pay for it one by one.
    for (int i = 0; i < RT355_MAX_IN_FLIGHT && err == hipSuccess; ++i) {
        if ((err = hipEventRecord(c->ev_prep0[i], c->stream)) != hipSuccess) break;
        if ((err = hipEventRecord(c->ev_k0[i], c->stream)) != hipSuccess) break;
        if ((err = hipEventRecord(c->ev_k1[i], c->stream)) != hipSuccess) break;
        err = hipEventRecord(c->ev_done[i], c->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) {
        rt_destroy(c);
        return fail_hip(err, "rt_create: event warm-up");
    }
    *out = c;
    return RT_OK;
}

int rt_destroy(rt_ctx* c) {
    if (!c) return RT_OK;
    (void)hipSetDevice(c->device);
    for (uint32_t i = 0; i < c->in_flight; ++i) (void)hipEventSynchronize(c->ev_done[i]);
    for (int k = 0; k < kStreams; ++k)
        if (c->streams[k]) (void)hipStreamSynchronize(c->streams[k]);
    if (c->query_pending) (void)hipEventSynchronize(c->ev_query);
    if (c->query_stream) (void)hipStreamSynchronize(c->query_stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    rt_comm_release(c);
    delete c->rebuild;
    delete c;                 // every buffer, event and stream: released by its owner (rt_own.h), in the order rt_ctx.h declares
    return RT_OK;
}

int rt_wait(rt_ctx* c);
int rt_read_pixels_wait(rt_ctx* c);
uint32_t rt_local_tiles(const rt_ctx* c) { return rt_tiles_of_rank(c->H, c->rank, c->world); }
static uint32_t local_tiles(const rt_ctx* c) { return rt_local_tiles(c); }

uint32_t rt_tiles_of_rank(uint32_t height, uint32_t rank, uint32_t world) {
    if (world == 0 || rank >= world) return 0;
    const uint32_t t = tiles_total(height);
    return t > rank ? (t - rank + world - 1u) / world : 0u;
}

uint32_t rt_padded_tiles(uint32_t height, uint32_t world) {
    if (world == 0) return 0;
    return (tiles_total(height) + world - 1u) / world;
}

// Scene-setup calls change device state that frames in flight may read: they drain first.
int rt_drain(rt_ctx* c) {
    if (c->query_pending) {         // a ray query reads the scene too (rt_trace_rays)
        RT_HIP(hipEventSynchronize(c->ev_query));
        c->query_pending = false;
        c->query_versions = false;
    }
    bool copies = false;
    for (int k = 0; k < kStreams; ++k) copies = copies || c->copy_pending[k];
    if (copies) { int rc = rt_read_pixels_wait(c); if (rc != RT_OK) return rc; }
    return c->in_flight ? rt_wait(c) : RT_OK;
}
static int drain(rt_ctx* c) { return rt_drain(c); }

static int ensure_out(rt_ctx* c) {
    // sized for the padded tile count so that the buffer can be an all-gather operand; one
    // buffer per stream rt_render rotates over (consecutive frames may overlap on the device)
    const size_t need = (size_t)rt_padded_tiles(c->H, c->world) * 8u * c->W * 4u;
    if (need > c->out_bytes || !c->d_outs[0].p) {
        RT_HIP(hipStreamSynchronize(c->stream));
        for (int k = 0; k < kStreams; ++k) c->d_outs[k].reset();
        c->d_out = nullptr;
        c->out_bytes = 0;
        if (need) {
            for (int k = 0; k < kStreams; ++k) {
                RT_HIP(c->d_outs[k].replace(need));
                RT_HIP(hipMemsetAsync(c->d_outs[k].p, 0, need, c->stream));
            }
            RT_HIP(hipStreamSynchronize(c->stream));
            c->d_out = c->d_outs[0].as<uint8_t>();
            c->out_bytes = need;
        }
    }
    return RT_OK;
}

// The path queue of the two-kernel brute-force pipeline (48 B per local pixel in the worst case:
// every primary ray hits) is allocated when a frame first takes that pipeline -- the default
// hierarchy path never reads it (1.6 GB at 8K).
static int ensure_queue(rt_ctx* c) {
    const size_t entries = (size_t)rt_padded_tiles(c->H, c->world) * 8u * c->W;
    if (entries > c->queue_cap) {
        { int rc = drain(c); if (rc != RT_OK) return rc; }
        c->queue_cap = 0;
        RT_HIP(c->d_queue.replace(entries * 3u * sizeof(float4)));
        c->queue_cap = entries;
    }
    return RT_OK;
}

// End-of-path records for the hierarchy kernel under a textured sky (32 B per local pixel slot, one buffer per
// frame that may be in flight on its own stream): allocated when a frame first needs them.
static int ensure_fin(rt_ctx* c) {
    const size_t slots = (size_t)rt_padded_tiles(c->H, c->world) * 8u * c->W;
    if (slots * 2u * sizeof(float4) > c->d_fin[kStreams - 1].cap) {      // the last one allocated: all of them hold as much
        { int rc = drain(c); if (rc != RT_OK) return rc; }
        for (int k = 0; k < kStreams; ++k) c->d_fin[k].reset();
        for (int k = 0; k < kStreams; ++k) RT_HIP(c->d_fin[k].replace(slots * 2u * sizeof(float4)));
    }
    return RT_OK;
}

int rt_resize(rt_ctx* c, uint32_t width, uint32_t height) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_resize: ctx is NULL");
    if (width == 0 || height == 0 || width > 65536u || height > 65536u)
        return fail(RT_ERR_INVALID_ARG, "rt_resize: width/height must be in 1..65536");
    // pixel indices and the padded tile space are 32-bit in the kernels
    if ((uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u >= (1ull << 31))
        return fail(RT_ERR_INVALID_ARG, "rt_resize: more than 2^31 pixel slots (width x height, padded to 8x8 tiles)");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    c->W = width;
    c->H = height;
    return ensure_out(c);
}

int rt_set_partition(rt_ctx* c, uint32_t rank, uint32_t world) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_set_partition: ctx is NULL");
    if (world == 0 || rank >= world) return fail(RT_ERR_INVALID_ARG, "rt_set_partition: need rank < world");
    if (c->comm && (rank != c->rank || world != c->world))
        return fail(RT_ERR_STATE, "rt_set_partition: the partition of a context with a communicator is its rank in the group");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    c->rank = rank;
    c->world = world;
    if (c->W && c->H) return ensure_out(c);
    return RT_OK;
}

int rt_write_params(rt_ctx* c, const float params[24]) {
    if (!c || !params) return fail(RT_ERR_INVALID_ARG, "rt_write_params: NULL argument");
    std::memcpy(c->params, params, sizeof c->params);   // travels in the kernarg segment
    c->have_params = true;
    c->prep_params_valid = false;
    return RT_OK;
}

int rt_write_spheres(rt_ctx* c, const float* records, uint32_t n) {
    if (!c || (n && !records)) return fail(RT_ERR_INVALID_ARG, "rt_write_spheres: NULL argument");
    if (n > (1u << 24)) return fail(RT_ERR_INVALID_ARG, "rt_write_spheres: more than 2^24 spheres");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    if (n > c->cap_n) {
        RT_HIP(hipStreamSynchronize(c->stream));
        c->d_records.reset(); c->d_scene.reset();
        c->cap_n = 0;
        const size_t cap16 = ((size_t)n + 15u) & ~(size_t)15u;
        RT_HIP(c->d_records.replace((size_t)n * 32u));
        RT_HIP(c->d_scene.replace(cap16 * 8u * sizeof(float4)));
        c->cap_n = n;
    }
    if (n) {
        RT_HIP(hipMemcpyAsync(c->d_records.p, records, (size_t)n * 32u, hipMemcpyHostToDevice, c->stream));
        RT_HIP(hipStreamSynchronize(c->stream));   // caller may free `records` now (writeBuffer semantics)
    }
    c->n = n;
    c->scene_kind = 0;
    c->n16 = (n + 15u) & ~15u;
    c->h_records.assign(records, records + 8u * (size_t)n);   // the hierarchy is built lazily from this copy
    c->bvh_valid = false;
    // Moved spheres, same count: the next frame refits the node bounds on the device and keeps the topology;
    // a new topology for these positions is built on the worker thread meanwhile (enqueue takes it when done).
    if (n != 0 && n == c->bvh_topo_n) {
        if (!c->rebuild) c->rebuild = new (std::nothrow) rt_rebuild();
        if (c->rebuild) c->rebuild->post(records, n);
    }
    c->scene_bound = (float)rt_scene_bound(records, n);   // scene extent, for the filter's validity range (enqueue)
    c->scene_min_radius = rt_scene_min_radius(records, n);
    c->have_spheres = true;
    c->prep_spheres_valid = false;
    return RT_OK;
}

int rt_write_cubemap_face(rt_ctx* c, int face, uint32_t w, uint32_t h, const uint8_t* rgba) {
    if (!c || !rgba) return fail(RT_ERR_INVALID_ARG, "rt_write_cubemap_face: NULL argument");
    if (face < 0 || face > 5) return fail(RT_ERR_INVALID_ARG, "rt_write_cubemap_face: face must be 0..5");
    if (w == 0 || h == 0 || w > 16384u || h > 16384u)
        return fail(RT_ERR_INVALID_ARG, "rt_write_cubemap_face: face size must be in 1..16384");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    const size_t bytes = (size_t)w * h * 4u;
    if (c->fw[face] != w || c->fh[face] != h || !c->d_face[face].p) {
        RT_HIP(hipStreamSynchronize(c->stream));
        c->fw[face] = c->fh[face] = 0;
        RT_HIP(c->d_face[face].replace(bytes < 16 ? 16 : bytes));
        c->fw[face] = w;
        c->fh[face] = h;
    }
    RT_HIP(hipMemcpyAsync(c->d_face[face].p, rgba, bytes, hipMemcpyHostToDevice, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    c->face_texel0[face] = (uint32_t)rgba[0] | ((uint32_t)rgba[1] << 8) | ((uint32_t)rgba[2] << 16);
    return RT_OK;
}

// capacity of a device buffer, contents kept; drains when it has to reallocate
static int grow_buf(rt_ctx* c, rt_ctx::DevBuf& b, size_t need) {
    if (need <= b.cap) return RT_OK;
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    RT_HIP(hipStreamSynchronize(c->stream));
    rt_ctx::DevBuf nb;
    const size_t cap = need < 256 ? 256 : need;
    RT_HIP(nb.replace(cap));
    RT_HIP(hipMemsetAsync(nb.p, 0, cap, c->stream));
    if (b.p && b.used) RT_HIP(hipMemcpyAsync(nb.p, b.p, b.used, hipMemcpyDeviceToDevice, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    nb.used = b.used;
    b = std::move(nb);        // frees the old block
    return RT_OK;
}

// writeBuffer(buffer, byte_offset, data): grows the device buffer when needed (keeping what is
// already there), copies, and returns once the caller's memory is no longer needed
static int write_buf(rt_ctx* c, rt_ctx::DevBuf& b, size_t byte_offset, const void* data, size_t bytes, const char* who) {
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    const size_t need = byte_offset + bytes;
    { int rc = grow_buf(c, b, need); if (rc != RT_OK) return rc; }
    if (bytes) {
        if (!data) return fail(RT_ERR_INVALID_ARG, who);
        RT_HIP(hipMemcpyAsync(static_cast<char*>(b.p) + byte_offset, data, bytes, hipMemcpyHostToDevice, c->stream));
        RT_HIP(hipStreamSynchronize(c->stream));
    }
    if (need > b.used) b.used = need;
    return RT_OK;
}

int rt_write_triangles(rt_ctx* c, const float* data, uint32_t n) {                    // RR:198-209
    if (!c || (n && !data)) return fail(RT_ERR_INVALID_ARG, "rt_write_triangles: NULL argument");
    c->d_tri.used = 0;
    c->corners_valid = false;
    int rc = write_buf(c, c->d_tri, 0, data, (size_t)n * 160u, "rt_write_triangles: NULL data");
    if (rc == RT_OK) c->scene_kind = 1;
    return rc;
}
// The same write into every version of a per-frame buffer (the static part of the scene, or an instance set too large
// to travel with a frame): drains, like every scene-setup call.
static int write_versions(rt_ctx* c, rt_ctx::DevBuf (&b)[kVersions], size_t byte_offset, const void* data, size_t bytes, const char* who) {
    for (int v = 0; v < kVersions; ++v) c->ver_gen[v] = 0;      // the next frame on each version re-applies the per-frame state
    for (int v = 0; v < kVersions; ++v) {
        int rc = write_buf(c, b[v], byte_offset, data, bytes, who);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}
// capacity for a per-frame write in every version, contents kept; drains only when something must grow
static int reserve_versions(rt_ctx* c, rt_ctx::DevBuf (&b)[kVersions], size_t bytes) {
    for (int v = 0; v < kVersions; ++v) {
        if (b[v].cap < bytes) c->ver_gen[v] = 0;
        int rc = grow_buf(c, b[v], bytes);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

int rt_write_nodes(rt_ctx* c, size_t byte_offset, const float* data, uint32_t n) {    // RR:184-192, 212-223
    if (!c || (n && !data)) return fail(RT_ERR_INVALID_ARG, "rt_write_nodes: NULL argument");
    if (byte_offset % 32u) return fail(RT_ERR_INVALID_ARG, "rt_write_nodes: byte_offset must be a multiple of the 32-byte node");
    const size_t bytes = (size_t)n * 32u, end = byte_offset + bytes;
    const size_t head_bytes = (size_t)kHeadNodes * 32u;
    for (uint32_t i = 0; i < n; ++i) {              // u32(primitiveCount) as the kernel forms it (NaN and negatives: 0)
        const float f = data[8u * (size_t)i + 7u];
        const uint32_t cnt = !(f > 0.0f) ? 0u : (f >= 4294967040.0f ? 4294967295u : (uint32_t)f);
        c->node_count_max = std::max(c->node_count_max, cnt);
    }
    if (n) {                                        // the mirror the relinked copy of the BLAS trees is built from (rt_flow_build.h)
        // does the write change the STRUCTURE of the trees (a refit plan rests on it, rt_refit_blas)?  The reference's per-frame
        // rewrite of the top-level nodes usually does not.
        bool topo = c->h_nodes.size() < end / 4u;
        for (uint32_t i = 0; i < n && !topo; ++i)
            topo = std::memcmp(&c->h_nodes[byte_offset / 4u + 8u * (size_t)i + 3u], &data[8u * (size_t)i + 3u], 4) != 0 ||
                   std::memcmp(&c->h_nodes[byte_offset / 4u + 8u * (size_t)i + 7u], &data[8u * (size_t)i + 7u], 4) != 0;
        if (topo) ++c->topo_gen;
        if (c->h_nodes.size() < end / 4u) c->h_nodes.resize(end / 4u, 0.0f);
        std::memcpy(reinterpret_cast<char*>(c->h_nodes.data()) + byte_offset, data, bytes);
        if (!c->flow_dirty && end / 32u > c->flow.min_node) c->flow_dirty = true;      // the write reaches nodes the copy was built from
        if (end / 32u > c->flow.n_nodes) c->flow_dirty = true;                          // the buffer grew: the clamp-to-last-node rule moves
    }
    // the part of the write that falls into the head region updates the host's copy of it; frames carry that copy
    if (byte_offset < head_bytes && n) {
        const size_t hi = std::min(end, head_bytes);
        if (c->inst.head.size() < (size_t)kHeadNodes * 8u) c->inst.head.resize((size_t)kHeadNodes * 8u, 0.0f);
        std::memcpy(reinterpret_cast<char*>(c->inst.head.data()) + byte_offset, data, hi - byte_offset);
        c->inst.head_nodes = std::max(c->inst.head_nodes, (uint32_t)(hi / 32u));
        ++c->inst.gen;
    }
    int rc = RT_OK;
    if (end <= head_bytes) {                        // the per-frame TLAS write (RR:184-192): no drain, the next frame carries it
        RT_HIP(hipSetDevice(c->device));
        rc = reserve_versions(c, c->d_nodes, head_bytes);
    } else {
        rc = write_versions(c, c->d_nodes, byte_offset, data, bytes, "rt_write_nodes: NULL data");
    }
    if (rc == RT_OK) { c->scene_kind = 1; c->nodes_used = std::max(c->nodes_used, end); }
    return rc;
}
int rt_write_blas(rt_ctx* c, const float* data, uint32_t n) {                         // RR:169-174
    if (!c || (n && !data)) return fail(RT_ERR_INVALID_ARG, "rt_write_blas: NULL argument");
    if (n <= kInstMax) {
        RT_HIP(hipSetDevice(c->device));
        int rc = reserve_versions(c, c->d_blas, (size_t)kInstMax * 80u);
        if (rc != RT_OK) return rc;
        c->inst.blas.assign(data, data + 20u * (size_t)n);
        c->inst.blas_on = true;
        ++c->inst.gen;
        return RT_OK;
    }
    c->inst.blas_on = false;
    for (int v = 0; v < kVersions; ++v) c->d_blas[v].used = 0;
    return write_versions(c, c->d_blas, 0, data, (size_t)n * 80u, "rt_write_blas: NULL data");
}
int rt_write_tri_lookup(rt_ctx* c, const float* data, uint32_t n) {                   // RR:225-229
    if (!c || (n && !data)) return fail(RT_ERR_INVALID_ARG, "rt_write_tri_lookup: NULL argument");
    c->d_tri_lookup.used = 0;
    c->corners_valid = false;
    return write_buf(c, c->d_tri_lookup, 0, data, (size_t)n * 4u, "rt_write_tri_lookup: NULL data");
}
int rt_write_blas_lookup(rt_ctx* c, const float* data, uint32_t n) {                  // RR:177-181
    if (!c || (n && !data)) return fail(RT_ERR_INVALID_ARG, "rt_write_blas_lookup: NULL argument");
    if (n <= kInstMax) {
        RT_HIP(hipSetDevice(c->device));
        int rc = reserve_versions(c, c->d_blas_lookup, (size_t)kInstMax * 4u);
        if (rc != RT_OK) return rc;
        c->inst.lookup.assign(data, data + (size_t)n);
        c->inst.lookup_on = true;
        ++c->inst.gen;
        return RT_OK;
    }
    c->inst.lookup_on = false;
    for (int v = 0; v < kVersions; ++v) c->d_blas_lookup[v].used = 0;
    return write_versions(c, c->d_blas_lookup, 0, data, (size_t)n * 4u, "rt_write_blas_lookup: NULL data");
}
int rt_write_mesh_texture(rt_ctx* c, uint32_t w, uint32_t h, const uint8_t* rgba) {   // material.ts:61-65
    if (!c || !rgba) return fail(RT_ERR_INVALID_ARG, "rt_write_mesh_texture: NULL argument");
    if (w == 0 || h == 0 || w > 16384u || h > 16384u)
        return fail(RT_ERR_INVALID_ARG, "rt_write_mesh_texture: size must be in 1..16384");
    c->d_tex.used = 0;
    int rc = write_buf(c, c->d_tex, 0, rgba, (size_t)w * h * 4u, "rt_write_mesh_texture: NULL data");
    if (rc == RT_OK) { c->tex_w = w; c->tex_h = h; }
    return rc;
}

int rt_select_kernel(rt_ctx* c, int kernel) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_select_kernel: ctx is NULL");
    if (kernel == RT_KERNEL_RAYTRACER || kernel == RT_KERNEL_HEATMAP) { c->kernel = kernel; return RT_OK; }
    return fail(RT_ERR_INVALID_ARG, "rt_select_kernel: unknown kernel");
}

int rt_set_mode(rt_ctx* c, int mode) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_set_mode: ctx is NULL");
    if (mode != RT_MODE_FAST && mode != RT_MODE_STRICT) return fail(RT_ERR_INVALID_ARG, "rt_set_mode: unknown mode");
    c->mode = mode;
    return RT_OK;
}

int rt_set_variant(rt_ctx* c, int variant) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_set_variant: ctx is NULL");
    if (variant < 0 || variant > 6) return fail(RT_ERR_INVALID_ARG, "rt_set_variant: unknown variant");
    c->variant = variant;
    return RT_OK;
}

// ---- instance visibility masks (ray queries alone: no frame reads them) ----

// The table indexes BLAS records and is no part of any scene buffer: it outlives every write of those.  For queries this is a scene
// write, ordered by ev_query on one side and by completing before it returns on the other: it waits (the host does) for the queries
// enqueued before it, which keep the table they were enqueued with -- in their arguments, or in the device table this call may only
// now touch -- and it returns with the device table written, so a query enqueued afterwards, on any stream, reads the new one with no
// event to wait for.  It copies on the query stream, where no frame runs: no drain, no frame waited for, ev_scene left alone (a frame
// that waits for ev_scene would otherwise wait here).
int rt_write_instance_masks(rt_ctx* c, const uint32_t* masks, uint32_t n) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_write_instance_masks: ctx is NULL");
    if (n && !masks) return fail(RT_ERR_INVALID_ARG, "rt_write_instance_masks: masks is NULL");
    RT_HIP(hipSetDevice(c->device));
    if (c->query_pending) RT_HIP(hipEventSynchronize(c->ev_query));   // (not a drain: the frames in flight go on)
    if (n) {
        const size_t bytes = (size_t)n * 4u;
        if (bytes > c->d_masks.cap) RT_HIP(c->d_masks.replace(std::max(bytes, (size_t)256u)));
        RT_HIP(c->query_stream.ensure(hipStreamNonBlocking));
        RT_HIP(hipMemcpyAsync(c->d_masks.p, masks, bytes, hipMemcpyHostToDevice, c->query_stream));
        RT_HIP(hipStreamSynchronize(c->query_stream));
        c->h_masks.assign(masks, masks + n);
        c->d_masks.used = bytes;
    } else {
        c->h_masks.clear();
        c->d_masks.used = 0;
    }
    return RT_OK;
}

int rt_set_query_masks(rt_ctx* c, uint32_t nearest, uint32_t occlusion) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_set_query_masks: ctx is NULL");
    c->mask_nearest = nearest;
    c->mask_occlusion = occlusion;
    return RT_OK;
}

// ---- the triangle scene a kernel reads: one place for frames (rt_enqueue) and ray queries (rt_trace_rays) ----

// The compact corner array follows the triangles and the lookup table: built on `s` by the first frame or query that needs it
// after rt_write_triangles / rt_write_tri_lookup -- BEFORE a frame takes a slot of the event ring (it may drain the frames in
// flight, which empties the ring).
static int ensure_corners(rt_ctx* c, hipStream_t s) {
    if (c->corners_valid) return RT_OK;
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    const uint32_t n_slots = (uint32_t)(c->d_tri_lookup.used / 4u);
    { int rc = grow_buf(c, c->d_corners, (size_t)n_slots * 48u); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != s) RT_HIP(hipStreamWaitEvent(s, c->ev_scene, 0));
    RT_HIP(rt_launch_tri_corners(static_cast<float4*>(c->d_corners.p), static_cast<const float*>(c->d_tri.p),
                                 static_cast<const float*>(c->d_tri_lookup.p), n_slots, (uint32_t)(c->d_tri.used / 160u), s));
    RT_HIP(hipEventRecord(c->ev_scene, s));          // frames on other streams wait for it (the scene-update event)
    c->scene_stream = s;
    c->corners_valid = true;
    return RT_OK;
}

// The instance roots of a scene whose instance data travels with the frame (up to 16 instances) and whose indices fit the relinked
// pair records (rt_flow_build.h); false when the scene does not fit them.
static bool tri_pair_roots(const rt_ctx* c, uint32_t (&roots)[kInstMax], uint32_t& n_inst) {
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u);
    n_inst = (uint32_t)(c->inst.blas.size() / 20u);
    const bool fits = c->inst.blas_on && c->inst.lookup_on && n_inst >= 1u && n_inst <= kInstMax && !c->inst.lookup.empty() &&
                      c->inst.lookup.size() <= kInstMax && n_nodes >= 1u && n_nodes <= 65536u && c->d_tri_lookup.used / 4u <= 65536u &&
                      c->node_count_max <= 65535u && c->h_nodes.size() / 8u >= n_nodes;
    if (!fits) return false;
    for (uint32_t i = 0; i < n_inst; ++i) roots[i] = rt_flow_u32f(c->inst.blas[20u * i + 16u]);
    return true;
}

// The relinked copy is usable: current (no write has reached it, the same node count) and knowing every root -- and then the
// roots' metas.  Never rebuilds it (a frame does, rt_enqueue).
static bool tri_pairs_current(const rt_ctx* c, const uint32_t* roots, uint32_t n_inst, uint32_t (&root_meta)[kInstMax]) {
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u);
    const bool ok = !c->flow_dirty && c->flow.ok && c->flow.n_pairs != 0u && c->flow.n_nodes == n_nodes && rt_flow_covers(c->flow, roots, n_inst);
    if (ok) {
        const uint32_t last = n_nodes - 1u;
        for (uint32_t i = 0; i < n_inst; ++i)
            root_meta[i] = rt_flow_meta(c->h_nodes.data(), n_nodes, roots[i] < last ? roots[i] : last, c->flow.pair_of);
    }
    return ok;
}

// The scene over version `v` of the per-frame buffers (the static part of the scene is in every version), with the relinked pair
// records where `have_pairs` says they are current.  Work list, debug and form fields are the caller's.
static void tri_scene(const rt_ctx* c, uint32_t v, bool have_pairs, const uint32_t (&root_meta)[kInstMax], RtTriScene& ts) {
    ts.nodes = static_cast<const float4*>(c->d_nodes[v].p);
    ts.blas = static_cast<const float*>(c->d_blas[v].p);
    ts.tri = static_cast<const float*>(c->d_tri.p);
    ts.corners = static_cast<const float4*>(c->d_corners.p);
    ts.tri_lookup = static_cast<const float*>(c->d_tri_lookup.p);
    ts.blas_lookup = static_cast<const float*>(c->d_blas_lookup[v].p);
    ts.tex = static_cast<const uint8_t*>(c->d_tex.p);
    ts.n_nodes = (uint32_t)(c->nodes_used / 32u);
    ts.n_blas = c->inst.blas_on ? (uint32_t)(c->inst.blas.size() / 20u) : (uint32_t)(c->d_blas[v].used / 80u);
    ts.n_tri = (uint32_t)(c->d_tri.used / 160u);
    ts.n_tri_lookup = (uint32_t)(c->d_tri_lookup.used / 4u);
    ts.n_blas_lookup = c->inst.lookup_on ? (uint32_t)c->inst.lookup.size() : (uint32_t)(c->d_blas_lookup[v].used / 4u);
    ts.tex_w = c->tex_w; ts.tex_h = c->tex_h;
    ts.packed_ok = (c->node_count_max <= 65535u && ts.n_nodes <= 65536u && ts.n_tri_lookup <= 65536u) ? 1u : 0u;
    // the top-level tree this frame walks (the mirror holds every node write, per-frame heads included): small enough for the
    // four-slot TLAS stack?  (rt_tlas_fit.h; the same constants as the kernel's: rt_tri_device.h kSmallStack / kSmallNodes)
    ts.tlas_small = 0u;
    if (c->h_nodes.size() / 8u >= ts.n_nodes) {
        if (ts.n_blas <= 4u && rt_tlas_fits(c->h_nodes.data(), ts.n_nodes, 3u, 8u)) ts.tlas_small = 2u;
        else if (rt_tlas_fits(c->h_nodes.data(), ts.n_nodes, 4u, 16u)) ts.tlas_small = 1u;
        else if (rt_tlas_fits(c->h_nodes.data(), ts.n_nodes, 8u, 24u)) ts.tlas_small = 3u;
        else if (rt_tlas_fits(c->h_nodes.data(), ts.n_nodes, 8u, 32u)) ts.tlas_small = 4u;
    }
    // two-byte stack entries (count << 14 | x): every meta of the records and of this frame's roots must fit them
    ts.p16_ok = (have_pairs && c->flow.max_count <= 3u && c->flow.max_x <= 16383u) ? 1u : 0u;
    for (uint32_t i = 0; i < kInstMax && ts.p16_ok; ++i)
        if ((root_meta[i] >> 16) > 3u || (root_meta[i] & 0xFFFFu) > 16383u) ts.p16_ok = 0u;
    // (13-16 instances: only the form that stages sixteen records can walk the pair records -- the others find a root's meta in
    // one of TWELVE staged records --, i.e. only a frame whose tree passed a walk above)
    ts.pairs = (have_pairs && (ts.n_blas <= 12u || ts.tlas_small != 0u)) ? static_cast<const float4*>(c->d_flow.p) : nullptr;
    for (uint32_t i = 0; i < kInstMax; ++i) ts.root_meta[i] = root_meta[i];
}

// The instance data that travels with a frame (inst.blas_on / lookup_on), by value, in the layout the small forms stage it in
// (rt_tri_types.h: RtTriInst): the head of the node buffer from the mirror, the records with the lookup entries, the roots' metas
// (ts.root_meta) and the instances' visibility masks (a ray query reads them; a frame reads none) in their padding words.
static void tri_fill_inst(const rt_ctx* c, RtTriScene& ts) {
    const uint32_t nn = std::min(ts.n_nodes, kInstHeadNodes), nb = std::min(ts.n_blas, kInstBlas);
    std::memcpy(ts.inst.head, c->h_nodes.data(), (size_t)nn * 32u);
    std::memcpy(ts.inst.blas, c->inst.blas.data(), (size_t)nb * 80u);
    const uint32_t nl = std::min(ts.n_blas_lookup, nb);
    for (uint32_t k = 0; k < nb; ++k) {
        if (k < nl) ts.inst.blas[20u * k + 19u] = c->inst.lookup[k];
        std::memcpy(&ts.inst.blas[20u * k + 17u], &ts.root_meta[k], 4);
        const uint32_t mask = k < c->h_masks.size() ? c->h_masks[k] : 0xFFFFFFFFu;
        std::memcpy(&ts.inst.blas[20u * k + 18u], &mask, 4);
    }
}

// Brings version `v` of the per-frame buffers to the host's current instance state (a one-workgroup kernel on `s` whose kernarg
// block holds the values).  Every frame among the first `slot` of the event ring that reads the version must be through first,
// and so must the latest ray query that read a version.
static int apply_version(rt_ctx* c, uint32_t v, uint32_t slot, hipStream_t s) {
    for (uint32_t i = v; i < slot; i += (uint32_t)kVersions) RT_HIP(hipStreamWaitEvent(s, c->ev_k1[i], 0));
    if (c->query_versions && c->ev_query) RT_HIP(hipStreamWaitEvent(s, c->ev_query, 0));
    RtInstanceArgs ia;
    ia.nodes = static_cast<float*>(c->d_nodes[v].p);
    ia.blas = static_cast<float*>(c->d_blas[v].p);
    ia.lookup = static_cast<float*>(c->d_blas_lookup[v].p);
    ia.n_head_f = ia.nodes ? c->inst.head_nodes * 8u : 0u;
    ia.n_blas_f = (c->inst.blas_on && ia.blas) ? (uint32_t)c->inst.blas.size() : 0u;
    ia.n_lookup_f = (c->inst.lookup_on && ia.lookup) ? (uint32_t)c->inst.lookup.size() : 0u;
    if (ia.n_head_f) std::memcpy(ia.data, c->inst.head.data(), ia.n_head_f * sizeof(float));
    if (ia.n_blas_f) std::memcpy(ia.data + 31 * 8, c->inst.blas.data(), ia.n_blas_f * sizeof(float));
    if (ia.n_lookup_f) std::memcpy(ia.data + 31 * 8 + 16 * 20, c->inst.lookup.data(), ia.n_lookup_f * sizeof(float));
    RT_HIP(rt_launch_apply_instances(ia, s));
    RT_HIP(c->ev_ver[v].ensure(hipEventDisableTiming));
    RT_HIP(hipEventRecord(c->ev_ver[v], s));
    c->ver_stream[v] = s;
    c->ver_gen[v] = c->inst.gen;
    return RT_OK;
}

// What a kernel may assume of the sky, for frames (rt_enqueue) and shaded queries (shade_frame_args).  flat: six 1x1 faces of one
// colour.  seamless: six equal squares -- what WebGPU accepts as a cube texture (CM:35-79: 512 x 512 x 6).
static void sky_flags(const rt_ctx* c, uint32_t& flat, uint32_t& seamless) {
    flat = seamless = 1u;
    for (int i = 0; i < 6; ++i) {
        if (c->fw[i] != 1u || c->fh[i] != 1u || c->face_texel0[i] != c->face_texel0[0]) flat = 0u;
        if (c->fw[i] != c->fw[0] || c->fh[i] != c->fw[0]) seamless = 0u;
    }
}

// ---- a frame (rt_enqueue): its preconditions, its plan, what may drain before it takes a slot of the event ring, its steps ----

// Which of the streams rt_render / rt_render_gather rotate over `s` is; -1: a stream of the caller's (rt_render_to)
static int own_stream_index(const rt_ctx* c, hipStream_t s) {
    for (int k = 0; k < kStreams; ++k)
        if (s == c->streams[k]) return k;
    return -1;
}

// The state a frame needs; a triangle scene without a texture gets the default one here.
static int frame_preconditions(rt_ctx* c) {
    if (!c->W || !c->H) return fail(RT_ERR_STATE, "rt_render: rt_resize has not been called");
    if (!c->have_params) return fail(RT_ERR_STATE, "rt_render: rt_write_params has not been called");
    const bool tri = c->scene_kind == 1;
    if (!tri && !c->have_spheres) return fail(RT_ERR_STATE, "rt_render: rt_write_spheres has not been called");
    if (tri) {
        const bool have_blas = c->inst.blas_on ? !c->inst.blas.empty() : c->d_blas[0].used != 0;
        const bool have_lookup = c->inst.lookup_on ? !c->inst.lookup.empty() : c->d_blas_lookup[0].used != 0;
        if (!c->d_tri.used || !c->nodes_used || !have_blas || !c->d_tri_lookup.used || !have_lookup)
            return fail(RT_ERR_STATE, "rt_render: a triangle scene needs rt_write_triangles, _nodes, _blas, _tri_lookup and _blas_lookup");
        if (!c->d_tex.used) {   // meshTex is mandatory in the reference (RR:113-114); default: 1x1 white
            const uint8_t white[4] = {255, 255, 255, 255};
            int rc = rt_write_mesh_texture(c, 1, 1, white);
            if (rc != RT_OK) return rc;
        }
    } else if (c->kernel == RT_KERNEL_HEATMAP) {
        return fail(RT_ERR_UNSUPPORTED, "rt_render: the heatmap kernel counts BVH traversal steps; sphere scenes have no BVH");
    }
    for (int i = 0; i < 6; ++i)
        if (!c->d_face[i].p) return fail(RT_ERR_STATE, "rt_render: all six cube map faces must be written first");
    return RT_OK;
}

// Which kernels render the frame and what they need first.  Made from the context as the caller left it: frame_plan writes nothing
// and calls no HIP, and rt_enqueue makes it BEFORE anything that may drain the frames in flight -- a drain is an rt_wait, which
// changes pipelined_hint and in_flight --, so that a frame is planned the same whether or not it had to wait for a resource.
struct FramePlan {
    bool tri, filter_ok;                       // a triangle scene (else spheres); rt_plan: within the filter's range (else the literal kernel)
    uint32_t signed_filter;
    int own;                                   // own_stream_index of the frame's stream
    bool hint;                                 // ... one of the library's, and the caller keeps frames in flight (rt_wait: pipelined_hint)
    bool use_bvh, queue_pipeline;              // the hierarchy kernel (rt_bvh.hip); the two-kernel brute-force pipeline
    bool need_prep, need_bvh, refit;           // prep_spheres / the hierarchy first; ... by a refit of the device topology, not a host build
    uint32_t sky_flat, sky_seamless;
    bool resolve_pass;                         // rt_bvh.hip: sky_resolve
    RtLaunchCfg cfg;
};
static FramePlan frame_plan(const rt_ctx* c, hipStream_t s) {
    FramePlan p;
    p.tri = c->scene_kind == 1;
    p.filter_ok = false;
    p.signed_filter = 0;
    rt_plan(c->scene_bound, c->scene_min_radius, c->params, p.filter_ok, p.signed_filter);
    // Fast mode renders through the bounding-sphere hierarchy (rt_bvh.hip) from 128 spheres on (default,
    // variant 0) -- from 72 on for a caller that keeps frames in flight, where the hierarchy kernel's
    // end-of-frame tail is hidden: at 3840x2160 / 8 bounces the two forms cross at ~110 spheres one frame at a
    // time and at ~60 in flight (96 spheres: 1.33 vs 1.00 ms and 0.76 vs 0.98 ms; profiles/r02/count_sweep.log) --
    // or whenever variant 4 asks for it; variant 5 is the brute-force default, 1-3 its forms.
    p.own = own_stream_index(c, s);
    p.hint = p.own >= 0 && c->pipelined_hint;
    const uint32_t bvh_from = p.hint ? 72u : 128u;
    p.use_bvh = !p.tri && c->mode == RT_MODE_FAST && p.filter_ok && c->n > 0 &&
                (c->variant == 4 || (c->variant == 0 && c->n >= bvh_from));
    // Frames in flight: the hierarchy kernel and the triangle kernels write nothing but their
    // own control block and `dst`, so consecutive frames may overlap on the device (the next
    // frame's workgroups start while the last paths of this one finish), and so may the
    // single-kernel brute-force and literal forms; the two-kernel brute-force pipeline shares one
    // path queue and is serialised behind the frames in flight.
    p.cfg.mode = p.filter_ok ? c->mode : (int)RT_MODE_STRICT;
    p.cfg.variant = (c->variant == 4 || c->variant == 5) ? 0 : c->variant;   // rt_kernels.hip numbers its default 0
    p.queue_pipeline = !p.tri && !p.use_bvh && c->mode == RT_MODE_FAST && p.filter_ok && rt_trace_wants_queue(c->n, p.cfg);
    p.need_prep = !p.tri && c->n && (!c->prep_spheres_valid || (!p.use_bvh && !c->prep_params_valid));
    p.need_bvh = p.use_bvh && !c->bvh_valid;
    p.refit = p.need_bvh && c->bvh_topo_n == c->n && c->bvh_topo_n != 0u;
    sky_flags(c, p.sky_flat, p.sky_seamless);
    p.resolve_pass = p.use_bvh && !p.sky_flat;
    return p;
}

// A brute-force variant none of whose forms holds the scene (1 above 2,176 spheres, 2 and 3 above 3,264, up to the
// 4,608 from which every variant reads the records from global memory) is refused here: before anything of the frame
// is enqueued, a slot of the event ring is taken or the stats change.
static int frame_refused(const rt_ctx* c, const FramePlan& p) {
    if (p.tri || p.use_bvh || rt_trace_fits(c->n, c->n16, p.cfg, p.queue_pipeline)) return RT_OK;
    char buf[200];
    std::snprintf(buf, sizeof buf, "rt_render: kernel variant %d has no form for %u spheres (its sphere records exceed the "
                  "160 KiB of LDS); variant 0 renders any count", c->variant, c->n);
    return fail(RT_ERR_UNSUPPORTED, buf);
}

// The hierarchy after rt_write_spheres, its host side.  A changed sphere count (or the first frame): host build, here and
// now.  The same count: the topology on the device stays, its node bounds are refitted there (frame_scene_update);
// a topology the worker thread has finished meanwhile is taken first.  Either way the device arrays may be
// rewritten or reallocated: nothing may be in flight (rt_write_spheres has drained already).
static int ensure_hierarchy(rt_ctx* c, const FramePlan& p, bool& upload_topology) {
    upload_topology = false;
    if (!p.need_bvh) return RT_OK;
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    uint32_t nodes = c->bvh_nodes;
    if (!p.refit) {
        nodes = rt_bvh_build(c->h_records.data(), c->n, c->h_bvh_rec, c->h_bvh_link, rt_bvh_arity());
        upload_topology = true;
    } else if (c->rebuild) {
        std::lock_guard<std::mutex> lk(c->rebuild->m);
        if (c->rebuild->ready && c->rebuild->out_n == c->n) {
            c->h_bvh_rec.swap(c->rebuild->out_rec);
            c->h_bvh_link.swap(c->rebuild->out_link);
            nodes = c->rebuild->out_nodes;
            upload_topology = true;
        }
        c->rebuild->ready = false;
    }
    if (((size_t)nodes + 1u) * sizeof(uint32_t) > c->d_bvh_link.cap) {      // the second of the pair: both hold as many nodes
        c->d_bvh_rec.reset(); c->d_bvh_link.reset();
        RT_HIP(c->d_bvh_rec.replace(((size_t)nodes + 1u) * sizeof(float4)));
        RT_HIP(c->d_bvh_link.replace(((size_t)nodes + 1u) * sizeof(uint32_t)));
    }
    c->bvh_nodes = nodes;
    return RT_OK;
}

// The relinked pair records of the BLAS trees (rt_flow_build.h), for scenes whose instance data travels with the frame (up
// to 16 instances) and whose indices fit 16 bits: rebuilt when a write has reached the nodes the copy was made from or a
// frame names a root it does not know -- from the union of the roots it knows and the new ones, so that a host that
// alternates root sets between frames pays for each root once.  have_pairs: the copy is current and covers this frame's roots.
// (The counters move in a frame that fails later, too.)
static int ensure_pairs(rt_ctx* c, uint32_t (&root_meta)[kInstMax], bool& have_pairs) {
    have_pairs = false;
    if (c->kernel == RT_KERNEL_HEATMAP || c->variant == 6) return RT_OK;
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u);
    uint32_t roots[kInstMax], n_inst = 0;
    if (!tri_pair_roots(c, roots, n_inst)) return RT_OK;
    // (the per-frame head of the node buffer lives in inst.head until a frame carries it: the mirror has it already)
    const bool stale = c->flow_dirty || c->flow.n_nodes != n_nodes;
    const bool need = stale || !rt_flow_covers(c->flow, roots, n_inst);
    ++c->flow_frames_since;
    // A host that invalidates the copy with every frame (it rewrites BLAS nodes per frame: nothing says it may not) would
    // pay a drain, a host-side rebuild of every tree and an upload per frame for records that live one frame.  Four frames
    // in a row that each had to rebuild: the node walk (which reads the reference's buffer as written) for the next sixty,
    // then another try.
    if (need && c->flow_cooldown > 0u) {
        --c->flow_cooldown;
    } else if (need) {
        c->flow_streak = c->flow_frames_since <= 1u ? c->flow_streak + 1u : 1u;
        c->flow_frames_since = 0u;
        if (c->flow_streak >= 4u) { c->flow_cooldown = 60u; c->flow_streak = 0u; }
        { int rc = drain(c); if (rc != RT_OK) return rc; }
        std::vector<uint32_t> all(roots, roots + n_inst);
        if (!stale) all.insert(all.end(), c->flow.roots.begin(), c->flow.roots.end());   // roots already known stay known
        rt_flow_build(c->h_nodes.data(), n_nodes, all.data(), (uint32_t)all.size(), c->flow);
        c->flow_dirty = false;
        ++c->flow_gen;
        ++c->stats.pair_rebuilds;
        if (c->flow.ok && c->flow.n_pairs) {
            int rc = write_buf(c, c->d_flow, 0, c->flow.pairs.data(), (size_t)c->flow.n_pairs * 64u, "flow pairs");
            if (rc != RT_OK) return rc;
        }
    }
    have_pairs = tri_pairs_current(c, roots, n_inst, root_meta);
    return RT_OK;
}

// Everything of a frame that may drain the frames in flight -- which empties the event ring --, and so all of it BEFORE the frame
// takes its slot: the refusal, the lazily made buffers, the hierarchy's host side, and what the triangle kernels read beside the
// reference's buffers (the corner array, the pair records).  No other step of a frame calls drain.
static int frame_resources(rt_ctx* c, const FramePlan& p, hipStream_t s, bool& upload_topology, uint32_t (&root_meta)[kInstMax], bool& have_pairs) {
    { int rc = frame_refused(c, p); if (rc != RT_OK) return rc; }
    if (p.queue_pipeline) { int rc = ensure_queue(c); if (rc != RT_OK) return rc; }
    if (p.resolve_pass) { int rc = ensure_fin(c); if (rc != RT_OK) return rc; }
    { int rc = ensure_hierarchy(c, p, upload_topology); if (rc != RT_OK) return rc; }
    have_pairs = false;
    if (p.tri) {
        { int rc = ensure_corners(c, s); if (rc != RT_OK) return rc; }
        { int rc = ensure_pairs(c, root_meta, have_pairs); if (rc != RT_OK) return rc; }
    }
    if (c->in_flight == RT355_MAX_IN_FLIGHT) return rt_wait(c);   // event ring full
    return RT_OK;
}

extern "C++" {
// The sphere arrays in d_scene (rt_ctx.h: eight float4 arrays of n16), with the parameters and the counts, as the frame kernels
// read them (RtFrameArgs) and as prep_spheres writes them (RtPrepArgs)
template <typename ARGS>
static void sphere_arrays(const rt_ctx* c, ARGS& a) {
    std::memcpy(a.p, c->params, sizeof a.p);
    a.N = c->n; a.N16 = c->n16;
    float4* b = c->d_scene.as<float4>();
    const uint32_t m = c->n16;
    a.geo = b; a.lgt = b + m; a.cam = b + 2u * m; a.col = b + 3u * m;
    a.geo_f = b + 4u * m; a.lgt_f = b + 5u * m; a.cam_f = b + 6u * m;
    float* w = reinterpret_cast<float*>(b + 7u * m);
    a.geo_w = w; a.lgt_w = w + m; a.cam_w = w + 2u * m;
}
}

// Ordering against the frames in flight and against the last scene update
static int frame_order(rt_ctx* c, const FramePlan& p, hipStream_t s) {
    if (p.need_prep || p.need_bvh || p.queue_pipeline) {
        for (uint32_t i = 0; i < c->in_flight; ++i) RT_HIP(hipStreamWaitEvent(s, c->ev_k1[i], 0));
    }
    if (c->scene_stream && c->scene_stream != s) RT_HIP(hipStreamWaitEvent(s, c->ev_scene, 0));
    return RT_OK;
}

// What the plan says must run before the frame's kernel: prep_spheres, the hierarchy's upload, refit and fill
static int frame_scene_update(rt_ctx* c, const FramePlan& p, bool upload_topology, const RtFrameArgs& fa, hipStream_t s) {
    if (p.need_prep) {
        RtPrepArgs pa;
        sphere_arrays(c, pa);
        pa.records = c->d_records.as<float>();
        RT_HIP(rt_launch_prep(pa, s));
        c->prep_spheres_valid = true;
        c->prep_params_valid = true;
    }
    if (p.need_bvh) {
        if (upload_topology) {
            const size_t nn = (size_t)c->bvh_nodes + 1u;
            RT_HIP(hipMemcpyAsync(c->d_bvh_rec.p, c->h_bvh_rec.data(), nn * sizeof(float4), hipMemcpyHostToDevice, s));
            RT_HIP(hipMemcpyAsync(c->d_bvh_link.p, c->h_bvh_link.data(), nn * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            RT_HIP(hipStreamSynchronize(s));   // pageable sources: the vectors may be rebuilt later
            c->bvh_topo_n = c->n;
        }
        // bounds of the inner nodes for the current positions (a topology from the worker was built for older ones)
        if (p.refit) RT_HIP(rt_launch_bvh_refit(c->d_bvh_rec.as<float4>(), c->d_bvh_link.as<uint32_t>(), c->bvh_nodes, c->d_records.as<float>(), s));
        RT_HIP(rt_launch_bvh_fill(c->d_bvh_rec.as<float4>(), c->d_bvh_link.as<uint32_t>(), c->bvh_nodes, fa.geo_f, s));
        c->bvh_valid = true;
    }
    if (p.need_prep || p.need_bvh) {
        RT_HIP(hipEventRecord(c->ev_scene, s));
        c->scene_stream = s;
    }
    return RT_OK;
}

// frames in flight on DIFFERENT streams run concurrently and share the chip: this frame's grid is
// 1 / (number of distinct streams among it and the kStreams-1 frames enqueued before it); reads slot_stream[slot]
static uint32_t frame_grid_share(const rt_ctx* c, const FramePlan& p, uint32_t slot) {
    if (p.queue_pipeline) return 1u;
    // a caller that has been enqueuing frames back to back through rt_render / rt_render_gather (the library's
    // own rotation over kStreams streams) gets equal shares from the first frame of a batch on (rt_bvh.hip:
    // launch_bvh_as); one that waits after every frame keeps the whole chip, and frames a host enqueues on its
    // own stream(s) through rt_render_to share the chip by the streams actually in use, whatever the history
    if (p.hint) return (uint32_t)kStreams;
    hipStream_t seen[kStreams] = {c->slot_stream[slot]};
    uint32_t distinct = 1;
    for (uint32_t back = 1; back < (uint32_t)kStreams && back <= slot; ++back) {
        hipStream_t o = c->slot_stream[slot - back];
        bool known = false;
        for (uint32_t j = 0; j < distinct; ++j) known = known || seen[j] == o;
        if (!known) seen[distinct++] = o;
    }
    return distinct;
}

// The frame's arguments but grid_share: no HIP call
static void frame_args(const rt_ctx* c, const FramePlan& p, uint32_t slot, uint8_t* dst, RtFrameArgs& fa) {
    sphere_arrays(c, fa);
    fa.W = c->W; fa.H = c->H;
    fa.tile_first = c->rank; fa.tile_step = c->world; fa.n_local_tiles = local_tiles(c);
    fa.signed_filter = p.signed_filter;
    fa.bvh_rec = p.use_bvh ? c->d_bvh_rec.as<float4>() : nullptr;
    fa.bvh_link = p.use_bvh ? c->d_bvh_link.as<uint32_t>() : nullptr;
    fa.bvh_nodes = p.use_bvh ? c->bvh_nodes : 0u;
    // this frame's partial ray counters and its 32-byte control block: one of RT355_MAX_IN_FLIGHT
    // sets, all zeroed by rt_create and again by every frame's epilogue kernel (no memset or read-back by the host)
    unsigned long long* counters = c->d_rays.as<unsigned long long>() + (kCtrlBytes / 8u) * slot;
    unsigned long long* ctrl = counters + kCounterBytes / 8u;
    for (int i = 0; i < 6; ++i) { fa.face[i] = c->d_face[i].as<uint8_t>(); fa.fw[i] = c->fw[i]; fa.fh[i] = c->fh[i]; }
    fa.sky_flat = p.sky_flat;
    fa.sky_seamless = p.sky_seamless;
    fa.out = dst;
    // one record buffer per frame that may be running (rt_enqueue waits for the frame kStreams slots back)
    fa.fin = p.resolve_pass ? c->d_fin[slot % (uint32_t)kStreams].as<float4>() : nullptr;
    fa.rays = counters;
    fa.queue = p.queue_pipeline ? c->d_queue.as<float4>() : nullptr;   // rt_kernels.hip takes the pipeline only with a queue
    fa.qctrl = reinterpret_cast<uint32_t*>(ctrl) + 2;
    fa.queue_cap = p.queue_pipeline ? (uint32_t)c->queue_cap : 0u;
}

// The triangle scene of the frame in `slot`, the form of the kernel, and the instance data the form reads.
// Per-frame instance data (RR:169-192) travels with the frame: version `v` of the three buffers is brought to the
// host's current state by a one-workgroup kernel whose kernarg block holds the values, in front of the ray-trace
// kernel on the frame's stream.  The frame kVersions slots back read the same version: it must be through.
// Ordering does not lean on which stream a slot happens to use (a host may rotate rt_render_to over any number of its own
// streams): before a version is rewritten, EVERY frame in flight that reads it must be through; and a frame that reads a
// version another stream brought up to date waits for that update.
// (The small forms of the triangle kernel -- the reference's scene, any scene of a few instances -- read none of the three
// buffers: their instance data is in the kernel's own arguments, ts.inst.  No kernel, no event, no wait; the versions
// simply fall behind, and a later frame of another form brings its own up to date.)
static int frame_tri_scene(rt_ctx* c, const FramePlan& p, uint32_t slot, hipStream_t s, bool have_pairs, const uint32_t (&root_meta)[kInstMax], RtTriScene& ts) {
    const uint32_t v = slot % (uint32_t)kVersions;
    tri_scene(c, v, have_pairs, root_meta, ts);
    ts.tile_order = nullptr; ts.tile_cost = nullptr; ts.xcd_rows = 0u; ts.prio = 0u; ts.in_flight = p.hint ? 1u : 0u; ts.dbg = nullptr;
    // which form of the kernel renders the frame (rt_triangles.hip); the small forms take the frame's instance data in their
    // own arguments, in the layout they stage it in
    ts.form = (uint32_t)rt_tri_stack_form(ts, c->kernel == RT_KERNEL_HEATMAP);
    if (ts.form != 0u) {
        tri_fill_inst(c, ts);
        if (c->inst_gen_carried != c->inst.gen) { c->inst_gen_carried = c->inst.gen; ++c->stats.instance_uploads; }
    } else if (c->ver_gen[v] != c->inst.gen) {
        { int rc = apply_version(c, v, slot, s); if (rc != RT_OK) return rc; }
        ++c->stats.instance_uploads;
    } else if (c->ev_ver[v] && c->ver_stream[v] != s) {
        RT_HIP(hipStreamWaitEvent(s, c->ev_ver[v], 0));
    }
    return RT_OK;
}

// Tile order of the triangle kernel, before the launch: which of the library's sets of buffers the frame uses (-1: none), sized
// for its order_n tiles.  Only for frames on the library's own streams (each has its set of buffers) ... and only for a caller
// that waits after each frame (the reference's loop): with frames in flight the tiles of the next frame fill the slots a long
// tile leaves idle anyway, and row-major order keeps neighbours in one L2
static int order_prepare(rt_ctx* c, const FramePlan& p, uint32_t order_n, hipStream_t s, int& order_set) {
    order_set = -1;
    if (!p.tri || c->kernel == RT_KERNEL_HEATMAP || order_n < kOrderMinTiles || p.hint) return RT_OK;
    order_set = p.own;
    if (order_set >= 0 && c->d_tile_cost[order_set].cap < (size_t)order_n * 4u) {
        // only frames on this stream use the set: wait for them, not for the batch (no slot bookkeeping involved)
        RT_HIP(hipStreamSynchronize(s));
        const size_t cap = ((size_t)order_n * 4u + 7u) & ~(size_t)7u, scan_bytes = (size_t)rt_order_scan_words() * 4u;
        for (rt_ctx::DevBuf* b : {&c->d_tile_cost[order_set], &c->d_tile_order[order_set]}) {
            RT_HIP(b->replace(cap + scan_bytes));                      // the list carries two header words; behind the costs: order_tiles' bins
            b->cap = cap;                                              // ... which lie behind `cap`
        }
        RT_HIP(hipMemsetAsync(c->d_tile_cost[order_set].p, 0, cap + scan_bytes, s));   // tiles leave their times by atomicMax
        c->order_tiles[order_set] = 0;
    }
    return RT_OK;
}

// The triangle kernel, with the work list of the frame's set where one has been made for this tile count
static int frame_launch_triangles(rt_ctx* c, const RtFrameArgs& fa, RtTriScene& ts, int order_set, uint32_t order_n, hipStream_t s) {
#ifdef RT355_DEV_EXPORTS
    if (getenv("RT355_TRI_TIMELINE")) {
        const size_t words = 3u * ((size_t)order_n + 3u * 8192u + 15u * 256u + 64u + 8u * ((c->W + 7u) / 8u));
        if (c->d_tri_dbg.cap < words * 8u) RT_HIP(c->d_tri_dbg.replace(words * 8u));
        RT_HIP(hipMemsetAsync(c->d_tri_dbg.p, 0, c->d_tri_dbg.cap, s));
        ts.dbg = static_cast<unsigned long long*>(c->d_tri_dbg.p);
    }
    if (order_set >= 0 && getenv("RT355_KEEP_TILE_COST")) RT_HIP(hipMemsetAsync(c->d_tile_cost[order_set].p, 0, (size_t)order_n * 4u, s));
#endif
    if (order_set >= 0) {
        ts.tile_cost = static_cast<uint32_t*>(c->d_tile_cost[order_set].p);
        if (c->order_tiles[order_set] == order_n) {
            ts.tile_order = static_cast<const uint32_t*>(c->d_tile_order[order_set].p);
            // does that list split tiles?  Then the kernel whose parts' idle lanes trace ahead (the word may be a frame old)
            ts.roles = __atomic_load_n(&c->h_split[order_set], __ATOMIC_RELAXED) != 0ull ? 1u : 0u;
        }
#ifdef RT355_DEV_EXPORTS
        if (getenv("RT355_TRI_NOLIST")) ts.tile_order = nullptr;
#endif
    }
    RT_HIP(rt_launch_triangles(fa, ts, c->kernel == RT_KERNEL_HEATMAP, s));
    return RT_OK;
}

// The list of the set's next frame, made from the times this one leaves.  After the frame's event: rt_wait does not wait for it,
// the stream's next frame does
static int order_next(rt_ctx* c, int order_set, uint32_t order_n, hipStream_t s) {
    uint32_t* const cost = static_cast<uint32_t*>(c->d_tile_cost[order_set].p);
    uint32_t* const scan = reinterpret_cast<uint32_t*>(static_cast<char*>(c->d_tile_cost[order_set].p) + c->d_tile_cost[order_set].cap);
    uint32_t* const list = static_cast<uint32_t*>(c->d_tile_order[order_set].p);
    RT_HIP(rt_launch_order_hist(cost, scan, list, order_n, c->wave_slots, nullptr, nullptr, 0u, c->h_split + order_set, s));
    RT_HIP(rt_launch_order_scatter(cost, scan, list, order_n, s));
    c->order_tiles[order_set] = order_n;
    return RT_OK;
}

int rt_enqueue(rt_ctx* c, uint8_t* dst, hipStream_t s) {
    { int rc = frame_preconditions(c); if (rc != RT_OK) return rc; }
    RT_HIP(hipSetDevice(c->device));
    // the plan first, then everything that may drain: a frame that is refused, or fails, in there has taken no slot
    const FramePlan p = frame_plan(c, s);
    bool upload_topology = false, have_pairs = false;
    uint32_t root_meta[kInstMax] = {0};
    { int rc = frame_resources(c, p, s, upload_topology, root_meta, have_pairs); if (rc != RT_OK) return rc; }

    // ---- the slot of the event ring, and on the frame's stream: waits, scene update, the frame's own data ----
    const uint32_t slot = c->in_flight;
    { int rc = frame_order(c, p, s); if (rc != RT_OK) return rc; }
    RtFrameArgs fa;
    frame_args(c, p, slot, dst, fa);
    RT_HIP(hipEventRecord(c->ev_prep0[slot], s));
    { int rc = frame_scene_update(c, p, upload_topology, fa, s); if (rc != RT_OK) return rc; }
    c->slot_stream[slot] = s;
    fa.grid_share = frame_grid_share(c, p, slot);
    // the frame kStreams slots back must be through with this frame's end-of-path records (frame_args: fa.fin)
    if (p.resolve_pass && slot >= (uint32_t)kStreams) RT_HIP(hipStreamWaitEvent(s, c->ev_k1[slot - (uint32_t)kStreams], 0));
    RtTriScene ts;
    std::memset(&ts, 0, sizeof ts);
    if (p.tri) { int rc = frame_tri_scene(c, p, slot, s, have_pairs, root_meta, ts); if (rc != RT_OK) return rc; }
    int order_set = -1;
    const uint32_t order_n = ((c->W + 7u) / 8u) * fa.n_local_tiles;
    { int rc = order_prepare(c, p, order_n, s, order_set); if (rc != RT_OK) return rc; }

    // ---- the kernel between its two events, the epilogue, the list of the stream's next frame ----
    RT_HIP(hipEventRecord(c->ev_k0[slot], s));
    g_rt_kernel_id = RT_KID_NONE;
    if (p.tri) { int rc = frame_launch_triangles(c, fa, ts, order_set, order_n, s); if (rc != RT_OK) return rc; }
    else if (p.use_bvh) RT_HIP(rt_launch_bvh(fa, s));
    else RT_HIP(rt_launch_trace(fa, p.cfg, s));
    RT_HIP(hipEventRecord(c->ev_k1[slot], s));
#ifdef RT355_DEV_EXPORTS
    if (order_set >= 0 && getenv("RT355_KEEP_TILE_COST")) {      // tools/tile_cost_probe.py reads the times of whole tiles in index order
        c->order_tiles[order_set] = 0;
        order_set = -1;
    }
#endif
    // The end of the frame: its counters summed into host-visible memory and zeroed for the slot's next frame (rt_assemble.hip:
    // frame_epilogue), then the event rt_wait waits for -- as early as can be: an awaited frame's successor is launched by a host
    // that has to wake up first, and its turnaround (15-30 us) is what the work-list kernels behind the event hide in.  (Round 5
    // ran the epilogue inside order_hist's first workgroup to save a link of the chain: the host woke 11 us later and the frame
    // period GREW by as much -- TRI 0.276 -> 0.298 ms; profiles/r05/ref_awaited_trace.log.)
    RT_HIP(rt_launch_frame_epilogue(fa.rays, c->h_rays.as<unsigned long long>() + 2u * slot, (uint32_t)(kCtrlBytes / 8u), s));
    RT_HIP(hipEventRecord(c->ev_done[slot], s));
    if (order_set >= 0) { int rc = order_next(c, order_set, order_n, s); if (rc != RT_OK) return rc; }
    c->stats.kernel_id = (uint32_t)g_rt_kernel_id;
    if (p.tri) c->stats.tri_form = (uint32_t)g_rt_tri_form;
    c->stats.grid_share = fa.grid_share;
    c->in_flight = slot + 1;
    return RT_OK;
}

#ifdef RT355_DEV_EXPORTS
// development builds only (tools/tri_timeline.py): {start, end, tile << 8 | part} of every workgroup of the last triangle frame
__attribute__((visibility("default"))) long long rt_debug_tri_timeline(rt_ctx* c, unsigned long long* dst, size_t cap_words) {
    if (!c || !c->d_tri_dbg.p) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const size_t n = std::min(cap_words, c->d_tri_dbg.cap / 8u);
    if (hipMemcpy(dst, c->d_tri_dbg.p, n * 8u, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long long)n;
}
// development builds only (tools/tile_cost_probe.py): the per-tile times of the last frame rendered on stream `set`
__attribute__((visibility("default"))) int rt_debug_tile_cost(rt_ctx* c, int set, uint32_t* dst, uint32_t cap) {
    if (!c || set < 0 || set >= kStreams || !c->d_tile_cost[set].p) return -1;
    const uint32_t n = std::min(cap, (uint32_t)(c->d_tile_cost[set].cap / 4u));
    if (hipStreamSynchronize(c->streams[set]) != hipSuccess) return -1;
    if (hipMemcpy(dst, c->d_tile_cost[set].p, (size_t)n * 4u, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)n;
}
#endif

// Colour buffer k is about to be written by a frame on stream `st`.  A frame of the current batch that renders into the same
// buffer on ANOTHER stream must be through first (a streaming read-back of it orders itself: ev_copy).  Streams and buffers
// rotate independently since awaited frames stay on one stream: within a run of rt_render calls their offset is constant and
// frame i + 4 follows frame i on its stream anyway, but an awaited frame in between shifts the offset, and rt_render_gather /
// rt_group_render pair stream k with buffer k whatever rt_render did before.
int rt_order_colour_buffer(rt_ctx* c, uint32_t k, hipStream_t st) {
    const int before = c->buf_slot[k];
    if (before >= 0 && (uint32_t)before < c->in_flight && c->slot_stream[before] != st) RT_HIP(hipStreamWaitEvent(st, c->ev_k1[before], 0));
    return RT_OK;
}

int rt_render(rt_ctx* c) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_render: ctx is NULL");
    // consecutive frames rotate over kStreams streams and colour buffers, so that frames enqueued
    // back to back overlap on the device; rt_read_pixels returns the latest one
    const uint32_t k = c->frames_rendered % (uint32_t)kStreams;
    uint8_t* dst = c->d_outs[k].as<uint8_t>();
    // The stream: the next of the four while frames are in flight (they overlap); the SAME one for a frame that follows an
    // awaited frame -- the reference's loop.  The work list of an awaited triangle frame is made from the previous frame of
    // its stream: rotating regardless, that was the frame four steps back, and with the instances turning (the reference's
    // scene spins one of its meshes) a list that old fitted the picture badly: 0.56 ms per frame against 0.38 with nothing
    // moving (profiles/r04/loop_breakdown.log).
    if (c->in_flight != 0u) c->stream_rot = (c->stream_rot + 1u) % (uint32_t)kStreams;
    hipStream_t st = c->streams[c->stream_rot];
    // a streaming read-back (rt_read_pixels_async) may still be copying the frame this buffer holds
    if (c->copy_pending[k]) RT_HIP(hipStreamWaitEvent(st, c->ev_copy[k], 0));
    { int rc = rt_order_colour_buffer(c, k, st); if (rc != RT_OK) return rc; }
    int rc = rt_enqueue(c, dst, st);
#ifdef RT355_DEV_EXPORTS
    // development builds (tools/root_probe.py): what the ROOT of a group of RT355_DEV_ROOT_WORLD ranks runs behind its share of the
    // frame -- the de-interleave of the whole gathered frame, on the frame's own stream, moving its end event as rt_render_gather does
    if (rc == RT_OK)
        if (const char* e = getenv("RT355_DEV_ROOT_WORLD")) {
            // raw on purpose: an owner with static storage duration would release them after the runtime has shut down
            static uint8_t* dev_gather[kStreams] = {nullptr};
            static uint8_t* dev_frame[kStreams] = {nullptr};
            const uint32_t world = (uint32_t)atoi(e);
            const size_t gb = (size_t)world * rt_padded_tiles(c->H, world) * 8u * c->W * 4u, fb = (size_t)c->H * c->W * 4u;
            if (!dev_gather[k]) { RT_HIP(hipMalloc(reinterpret_cast<void**>(&dev_gather[k]), gb)); RT_HIP(hipMalloc(reinterpret_cast<void**>(&dev_frame[k]), fb)); }
            RT_HIP(rt_launch_assemble(dev_gather[k], dev_frame[k], c->W, c->H, world, rt_padded_tiles(c->H, world), st));
            RT_HIP(hipEventRecord(c->ev_k1[c->in_flight - 1u], st));
        }
#endif
    if (rc == RT_OK) { c->d_out = dst; c->buf_slot[k] = (int)c->in_flight - 1; ++c->frames_rendered; }
    return rc;
}

int rt_render_to(rt_ctx* c, void* device_dst, size_t cap, void* hip_stream) {
    if (!c || !device_dst) return fail(RT_ERR_INVALID_ARG, "rt_render_to: NULL argument");
    const size_t need = (size_t)local_tiles(c) * 8u * c->W * 4u;
    if (cap < need) return fail(RT_ERR_CAPACITY, "rt_render_to: destination smaller than local_tiles*8*W*4");
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return rt_enqueue(c, static_cast<uint8_t*>(device_dst), s);
}

// forget the frames in flight (their work has left the device: a communicator was aborted): counters zeroed, ring empty
void rt_abandon_in_flight(rt_ctx* c) {
    for (int k = 0; k < kStreams; ++k)
        if (c->streams[k]) (void)hipStreamSynchronize(c->streams[k]);
    if (c->in_flight) {
        (void)hipMemsetAsync(c->d_rays.p, 0, kCtrlBytes * c->in_flight, c->stream);
        (void)hipStreamSynchronize(c->stream);
    }
    (void)hipGetLastError();
    c->in_flight = 0;
    c->stats.batch_frames = 0;
    for (int v = 0; v < kVersions; ++v) c->ver_gen[v] = 0;
}

int rt_wait(rt_ctx* c) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_wait: ctx is NULL");
    RT_HIP(hipSetDevice(c->device));
    if (c->comm && c->in_flight) {
        // frames that end in an RCCL exchange: a poll that notices a failed peer or a missed deadline (rt_comm.hip)
        int rc = rt_comm_wait_frames(c);
        if (rc != RT_OK) return rc;
    }
    // one synchronisation per frame, on the event behind its epilogue kernel: ray count and fault word are in host memory
    // by then, the counter set is zero again (rt_assemble.hip: frame_epilogue)
    for (uint32_t i = 0; i < c->in_flight; ++i) RT_HIP(hipEventSynchronize(c->ev_done[i]));
    if (c->in_flight) {
        c->stats.frames += c->in_flight;
        const unsigned long long* h_rays = c->h_rays.as<unsigned long long>();
        c->stats.rays = h_rays[2u * (c->in_flight - 1u)];          // of the latest frame
        c->stats.batch_frames = c->in_flight;
        // Frames in flight?  Only the library's own rotation counts: a host that enqueues several frames on ONE stream
        // of its own (rt_render_to) has them serialised by that stream, and must not be given a quarter of the chip.
        {
            bool used[kStreams] = {false};
            for (uint32_t i = 0; i < c->in_flight; ++i)
                if (const int k = own_stream_index(c, c->slot_stream[i]); k >= 0) used[k] = true;
            c->pipelined_hint = std::count(used, used + kStreams, true) > 1;
        }
        c->stats.batch_kernel_ms = 0.0f;
        for (uint32_t i = 0; i < c->in_flight; ++i) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->ev_k0[i], c->ev_k1[i]) == hipSuccess) {
                c->stats.kernel_ms = ms;
                c->stats.batch_kernel_ms += ms;
            }
            if (hipEventElapsedTime(&ms, c->ev_prep0[i], c->ev_k0[i]) == hipSuccess) c->stats.prep_ms = ms;
        }
        (void)hipGetLastError();
        c->in_flight = 0;
        for (int k = 0; k < kStreams; ++k) c->buf_slot[k] = -1;      // every frame of the batch is complete
        // a kernel that could not run as planned says so in the word behind its first ray counter (rt_device.h: report_fault)
        unsigned long long fault = 0ull;
        for (uint32_t i = 0; i < c->stats.batch_frames; ++i) fault = std::max(fault, h_rays[2u * i + 1u]);
        if (fault != 0ull) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "rt_wait: the ray-trace kernel reported fault %llu (1: dynamic LDS not at address 0); the frame is incomplete", fault);
            g_rt_err = buf;
            return RT_ERR_HIP;
        }
        return rt_comm_after_wait(c);
    }
    return RT_OK;
}

int rt_read_pixels(rt_ctx* c, uint8_t* dst, size_t cap) {
    if (!c || !dst) return fail(RT_ERR_INVALID_ARG, "rt_read_pixels: NULL argument");
    if (!c->d_out) return fail(RT_ERR_STATE, "rt_read_pixels: no colour buffer (rt_resize first)");
    int rc = rt_wait(c);
    if (rc != RT_OK) return rc;
    // rows owned by this rank, clipped to the frame (the last tile may be partial)
    const uint32_t lt = local_tiles(c);
    size_t rows = 0;
    for (uint32_t j = 0; j < lt; ++j) {
        const uint32_t y0 = (c->rank + j * c->world) * 8u;
        rows += (c->H - y0 >= 8u) ? 8u : (c->H - y0);
    }
    // the compact buffer keeps 8 rows per tile; only the final tile can be short, so the
    // first `rows` rows are contiguous valid data
    const size_t need = rows * c->W * 4u;
    if (cap < need) return fail(RT_ERR_CAPACITY, "rt_read_pixels: destination smaller than the local rows * W * 4");
    RT_HIP(hipMemcpyAsync(dst, c->d_out, need, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_read_pixels_async(rt_ctx* c, uint32_t frames_back, uint8_t* dst, size_t cap) {
    if (!c || !dst) return fail(RT_ERR_INVALID_ARG, "rt_read_pixels_async: NULL argument");
    if (frames_back >= (uint32_t)kStreams || frames_back >= c->frames_rendered)
        return fail(RT_ERR_INVALID_ARG, "rt_read_pixels_async: frames_back must name one of the last four rt_render calls");
    if (c->world != 1u || c->comm) return fail(RT_ERR_STATE, "rt_read_pixels_async: whole-frame contexts only");
    if (!c->d_outs[0].p) return fail(RT_ERR_STATE, "rt_read_pixels_async: no colour buffer (rt_resize first)");
    const size_t need = (size_t)c->H * c->W * 4u;
    if (cap < need) return fail(RT_ERR_CAPACITY, "rt_read_pixels_async: destination smaller than H * W * 4");
    RT_HIP(hipSetDevice(c->device));
    const uint32_t k = (c->frames_rendered - 1u - frames_back) % (uint32_t)kStreams;
    if (c->buf_slot[k] >= 0) RT_HIP(hipStreamWaitEvent(c->copy_stream, c->ev_k1[c->buf_slot[k]], 0));   // behind that frame's kernels
    RT_HIP(hipMemcpyAsync(dst, c->d_outs[k].p, need, hipMemcpyDeviceToHost, c->copy_stream));
    RT_HIP(hipEventRecord(c->ev_copy[k], c->copy_stream));
    c->copy_pending[k] = true;
    return RT_OK;
}

int rt_read_pixels_wait(rt_ctx* c) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_pixels_wait: ctx is NULL");
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipStreamSynchronize(c->copy_stream));
    for (int k = 0; k < kStreams; ++k) c->copy_pending[k] = false;
    return RT_OK;
}

// raw on purpose: the memory is the caller's from here until rt_host_free
int rt_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(RT_ERR_INVALID_ARG, "rt_host_alloc: NULL / zero size");
    *out = nullptr;
    RT_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return RT_OK;
}

int rt_host_free(void* p) {
    if (p) RT_HIP(hipHostFree(p));
    return RT_OK;
}

int rt_get_stats(rt_ctx* c, rt_stats* out) {
    if (!c || !out) return fail(RT_ERR_INVALID_ARG, "rt_get_stats: NULL argument");
    c->stats.width = c->W;
    c->stats.height = c->H;
    c->stats.local_tiles = local_tiles(c);
    c->stats.spheres = c->n;
    c->stats.mode = c->mode;
    *out = c->stats;
    return RT_OK;
}

int rt_assemble_frame(rt_ctx* c, const void* gathered, void* frame, uint32_t world, void* hip_stream) {
    if (!c || !gathered || !frame) return fail(RT_ERR_INVALID_ARG, "rt_assemble_frame: NULL argument");
    if (world == 0) return fail(RT_ERR_INVALID_ARG, "rt_assemble_frame: world must be >= 1");
    if (!c->W || !c->H) return fail(RT_ERR_STATE, "rt_assemble_frame: rt_resize has not been called");
    RT_HIP(hipSetDevice(c->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    RT_HIP(rt_launch_assemble(static_cast<const uint8_t*>(gathered), static_cast<uint8_t*>(frame), c->W, c->H, world,
                              rt_padded_tiles(c->H, world), s));
    return RT_OK;
}

int rt_build_hierarchy(const float* records, uint32_t n, float* rec4, uint32_t* link, uint32_t cap_nodes,
                       uint32_t* n_nodes) {
    return rt_build_hierarchy_ex(records, n, rec4, link, cap_nodes, n_nodes, RT355_HIERARCHY_PASSES, nullptr);
}

int rt_build_hierarchy_ex(const float* records, uint32_t n, float* rec4, uint32_t* link, uint32_t cap_nodes,
                          uint32_t* n_nodes, uint32_t passes, double* info) {
    if ((n && !records) || !n_nodes) return fail(RT_ERR_INVALID_ARG, "rt_build_hierarchy: NULL argument");
    std::vector<float> r;
    std::vector<uint32_t> l;
    rt_bvh_build_info bi;
    const uint32_t nodes = rt_bvh_build(records, n, r, l, rt_bvh_arity(), passes > 16u ? 16u : passes, &bi);
    *n_nodes = nodes;
    if (info) { info[0] = (double)bi.nodes_topdown; info[1] = (double)bi.moves; info[2] = bi.cost_topdown; info[3] = bi.cost; }
    if (l.empty()) return RT_OK;                       // n == 0: nothing to write
    if (cap_nodes < nodes + 1u || !rec4 || !link) return fail(RT_ERR_CAPACITY, "rt_build_hierarchy: need n_nodes + 1 entries");
    std::memcpy(rec4, r.data(), r.size() * sizeof(float));
    std::memcpy(link, l.data(), l.size() * sizeof(uint32_t));
    return RT_OK;
}

int rt_build_flow(const float* nodes, uint32_t n_nodes, const uint32_t* roots, uint32_t n_roots, float* pairs, uint32_t cap_pairs,
                  uint32_t* n_pairs, uint32_t* root_meta) {
    if (!nodes || (n_roots && !roots) || !n_pairs) return fail(RT_ERR_INVALID_ARG, "rt_build_flow: NULL argument");
    RtFlow f;
    rt_flow_build(nodes, n_nodes, roots, n_roots, f);
    *n_pairs = f.n_pairs;
    if (!f.ok) return fail(RT_ERR_UNSUPPORTED, "rt_build_flow: node buffer beyond 65,536 entries or a count beyond 16 bits");
    if (f.n_pairs && (cap_pairs < f.n_pairs || !pairs)) return fail(RT_ERR_CAPACITY, "rt_build_flow: need room for n_pairs records");
    if (f.n_pairs) std::memcpy(pairs, f.pairs.data(), (size_t)f.n_pairs * 64u);
    if (root_meta)
        for (uint32_t r = 0; r < n_roots; ++r)
            root_meta[r] = rt_flow_meta(nodes, n_nodes, roots[r] < n_nodes - 1u ? roots[r] : n_nodes - 1u, f.pair_of);
    return RT_OK;
}

int rt_order_tiles(rt_ctx* c, const uint32_t* cost, uint32_t n, uint32_t wave_slots, uint32_t* order, size_t cap) {
    if (!c || (n && !cost) || !order) return fail(RT_ERR_INVALID_ARG, "rt_order_tiles: NULL argument");
    if (cap < (size_t)n + 2u) return fail(RT_ERR_CAPACITY, "rt_order_tiles: order needs n + 2 entries");
    if (n > (1u << 26)) return fail(RT_ERR_INVALID_ARG, "rt_order_tiles: more than 2^26 tiles");
    order[0] = order[1] = 0u;
    if (n == 0u) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    const size_t cost_bytes = ((size_t)n * 4u + 7u) & ~(size_t)7u, scan_bytes = (size_t)rt_order_scan_words() * 4u;
    rt_ctx::DevBuf cost_buf, order_buf;                 // temporaries of this call
    hipError_t e = cost_buf.replace(cost_bytes + scan_bytes);
    if (e == hipSuccess) e = order_buf.replace(((size_t)n + 2u) * 4u);
    void *const d_cost = cost_buf.p, *const d_order = order_buf.p;
    if (e == hipSuccess) e = hipMemsetAsync(d_cost, 0, cost_bytes + scan_bytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cost, cost, (size_t)n * 4u, hipMemcpyHostToDevice, c->stream);
    uint32_t* const scan = reinterpret_cast<uint32_t*>(static_cast<char*>(d_cost) + cost_bytes);
    // twice on the same buffers, as consecutive frames of a stream do: the first pass must leave the scan words (and the costs) zero
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
        if (pass) e = hipMemcpyAsync(d_cost, cost, (size_t)n * 4u, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = rt_launch_order_hist(static_cast<uint32_t*>(d_cost), scan, static_cast<uint32_t*>(d_order), n, wave_slots, nullptr, nullptr, 0u, nullptr, c->stream);
        if (e == hipSuccess) e = rt_launch_order_scatter(static_cast<uint32_t*>(d_cost), scan, static_cast<uint32_t*>(d_order), n, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(order, d_order, ((size_t)n + 2u) * 4u, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail_hip(e, "rt_order_tiles");
    return RT_OK;
}

int rt_read_hierarchy(rt_ctx* c, float* rec4, uint32_t* link, uint32_t cap_nodes, uint32_t* n_nodes) {
    if (!c || !n_nodes) return fail(RT_ERR_INVALID_ARG, "rt_read_hierarchy: NULL argument");
    *n_nodes = 0;
    if (c->scene_kind != 0 || c->bvh_nodes == 0u || !c->d_bvh_rec.p || !c->d_bvh_link.p)
        return fail(RT_ERR_STATE, "rt_read_hierarchy: no frame of this sphere scene has walked a hierarchy");
    const uint32_t nodes = c->bvh_nodes;
    *n_nodes = nodes;
    if (cap_nodes < nodes + 1u || !rec4 || !link) return fail(RT_ERR_CAPACITY, "rt_read_hierarchy: need n_nodes + 1 entries");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    const size_t nn = (size_t)nodes + 1u;
    RT_HIP(hipMemcpyAsync(rec4, c->d_bvh_rec.p, nn * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipMemcpyAsync(link, c->d_bvh_link.p, nn * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}

// ---- deforming meshes: partial triangle writes and the BLAS refit (rt_refit_plan.h, rt_refit.hip) ----------------------------

static_assert(kRefitVersions == (uint32_t)kVersions, "rt_refit.hip stores into every version of the node buffer");
static_assert((int)kRefitInvalid == (int)RT_ERR_INVALID_ARG && (int)kRefitUnsupported == (int)RT_ERR_UNSUPPORTED, "rt_refit_plan.h returns rt_status codes");

int rt_refit_plan(const float* nodes, uint32_t n_nodes, uint32_t n_tri_lookup, const uint32_t* roots, uint32_t n_roots,
                  uint32_t* plan, uint32_t cap_nodes, uint32_t* n_plan) {
    if ((n_nodes && !nodes) || (n_roots && !roots) || !n_plan) return fail(RT_ERR_INVALID_ARG, "rt_refit_plan: NULL argument");
    *n_plan = 0;
    std::vector<uint32_t> p;
    const char* why = "";
    const int rc = rt_refit_plan_build(nodes, n_nodes, n_tri_lookup, roots, n_roots, p, &why);
    if (rc != kRefitOk) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_refit_plan: %s", why); return fail(rc, msg); }
    *n_plan = (uint32_t)(p.size() / 3u);
    if (p.empty()) return RT_OK;
    if (cap_nodes < *n_plan || !plan) return fail(RT_ERR_CAPACITY, "rt_refit_plan: need room for n_plan triples");
    std::memcpy(plan, p.data(), p.size() * sizeof(uint32_t));
    return RT_OK;
}

int rt_update_triangles(rt_ctx* c, uint32_t first, uint32_t n, const float* data) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles: ctx is NULL");
    if (c->scene_kind != 1 || !c->d_tri.used) return fail(RT_ERR_STATE, "rt_update_triangles: no triangle scene (rt_write_triangles first)");
    if ((uint64_t)first + n > c->d_tri.used / 160u) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles: first + n is beyond the triangles written");
    if (n == 0u) return RT_OK;
    if (!data) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles: data is NULL");
    // the corner array follows: rebuilt whole by the next refit, frame or query (ensure_corners) -- one pass over 48 bytes per
    // lookup slot, cheaper than keeping the inverse of the lookup table to patch single slots
    c->corners_valid = false;
    return write_buf(c, c->d_tri, (size_t)first * 160u, data, (size_t)n * 160u, "rt_update_triangles: NULL data");
}

// the copy of planned node `i` in the pair records (rt_flow_build.h): as the left child of the pair keyed by i, as the right child
// of the pair keyed by i - 1 -- and of its own pair when i is the last node, where left + 1 clamps
// (three copies -- the last node of a hand-made buffer as the right child of two pairs -- do not fit the plan's two words: false)
static bool refit_pair_halves(const RtFlow& f, uint32_t i, uint32_t (&half)[2]) {
    half[0] = half[1] = 0xFFFFFFFFu;
    if (f.pair_of[i] != 0xFFFFFFFFu) half[0] = 2u * f.pair_of[i];
    const bool after = i > 0u && f.pair_of[i - 1u] != 0xFFFFFFFFu, own = i == f.n_nodes - 1u && f.pair_of[i] != 0xFFFFFFFFu;
    if (after && own) return false;
    if (after) half[1] = 2u * f.pair_of[i - 1u] + 1u;
    if (own) half[1] = 2u * f.pair_of[i] + 1u;
    return true;
}

int rt_refit_blas(rt_ctx* c, const uint32_t* roots, uint32_t n_roots) {
    if (!c || (!roots && n_roots)) return fail(RT_ERR_INVALID_ARG, "rt_refit_blas: NULL argument");
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u), n_slots = (uint32_t)(c->d_tri_lookup.used / 4u);
    if (c->scene_kind != 1 || !c->d_tri.used || !n_nodes || !n_slots || c->h_nodes.size() / 8u < n_nodes)
        return fail(RT_ERR_STATE, "rt_refit_blas: no triangle scene (rt_write_triangles, _nodes and _tri_lookup first)");
    RT_HIP(hipSetDevice(c->device));
    // ---- which roots ----
    std::vector<uint32_t> rs;
    if (roots) {
        rs.assign(roots, roots + n_roots);
    } else if (c->inst.blas_on) {                       // every root the current BLAS records name
        for (size_t i = 0; i + 20u <= c->inst.blas.size(); i += 20u) rs.push_back(rt_flow_u32f(c->inst.blas[i + 16u]));
    } else if (c->d_blas[0].used) {                     // an instance set written to the device only (more than sixteen)
        std::vector<float> rec(c->d_blas[0].used / 4u);
        RT_HIP(hipMemcpy(rec.data(), c->d_blas[0].p, rec.size() * 4u, hipMemcpyDeviceToHost));
        for (size_t i = 0; i + 20u <= rec.size(); i += 20u) rs.push_back(rt_flow_u32f(rec[i + 16u]));
    }
    if (!roots && rs.empty()) return fail(RT_ERR_STATE, "rt_refit_blas: no BLAS records name a root (rt_write_blas first)");
    std::sort(rs.begin(), rs.end());
    rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
    if (rs.empty()) return RT_OK;
    // ---- the plan: validated on the mirror before anything on the device, in the mirror or in the flags changes ----
    if (c->refit.topo_gen != c->topo_gen || c->refit.n_tri_lookup != n_slots || c->refit.roots != rs) {
        std::vector<uint32_t> plan;
        const char* why = "";
        const int rc = rt_refit_plan_build(c->h_nodes.data(), n_nodes, n_slots, rs.data(), (uint32_t)rs.size(), plan, &why);
        if (rc != kRefitOk) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_refit_blas: %s", why); return fail(rc, msg); }
        c->refit.plan.swap(plan);
        c->refit.roots = rs;
        c->refit.topo_gen = c->topo_gen;
        c->refit.n_tri_lookup = n_slots;
        c->refit.on_device = false;
        c->refit.lo = 0xFFFFFFFFu; c->refit.hi = 0u;
        for (size_t e = 0; e < c->refit.plan.size(); e += 3u) {
            c->refit.lo = std::min(c->refit.lo, c->refit.plan[e]);
            c->refit.hi = std::max(c->refit.hi, c->refit.plan[e]);
        }
    }
    const uint32_t n_plan = (uint32_t)(c->refit.plan.size() / 3u);
    if (n_plan == 0u) return RT_OK;
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    for (int v = 0; v < kVersions; ++v) { int rc = grow_buf(c, c->d_nodes[v], c->nodes_used); if (rc != RT_OK) return rc; }
    { int rc = ensure_corners(c, c->stream); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    // the pair records hold copies of the boxes: brought up to date by the same kernel while they are current; records that are
    // stale anyway are rebuilt from the mirror by the frame that needs them
    bool pairs = !c->flow_dirty && c->flow.ok && c->flow.n_pairs != 0u && c->flow.n_nodes == n_nodes &&
                 c->d_flow.p && c->d_flow.used >= (size_t)c->flow.n_pairs * 64u;
    bool pairs_left_behind = false;                     // current records this refit cannot reach: rebuilt by the next frame
    for (uint32_t e = 0; e < n_plan && pairs; ++e) {
        uint32_t half[2];
        if (!refit_pair_halves(c->flow, c->refit.plan[3u * e], half)) { pairs = false; pairs_left_behind = true; }
    }
    if (!c->refit.on_device || c->refit.with_pairs != pairs || (pairs && c->refit.flow_gen != c->flow_gen)) {
        std::vector<uint32_t> dev((size_t)n_plan * kRefitPlanWords);
        for (uint32_t e = 0; e < n_plan; ++e) {
            uint32_t* q = &dev[(size_t)e * kRefitPlanWords];
            q[0] = c->refit.plan[3u * e]; q[1] = c->refit.plan[3u * e + 1u]; q[2] = c->refit.plan[3u * e + 2u];
            uint32_t half[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
            if (pairs) (void)refit_pair_halves(c->flow, q[0], half);
            q[3] = half[0]; q[4] = half[1];
        }
        c->refit.on_device = false;
        { int rc = grow_buf(c, c->d_refit_plan, dev.size() * 4u); if (rc != RT_OK) return rc; }
        RT_HIP(hipMemcpyAsync(c->d_refit_plan.p, dev.data(), dev.size() * 4u, hipMemcpyHostToDevice, c->stream));
        RT_HIP(hipStreamSynchronize(c->stream));        // a pageable source
        c->refit.on_device = true;
        c->refit.with_pairs = pairs;
        c->refit.flow_gen = c->flow_gen;
    }
    RtRefitArgs ra;
    ra.plan = static_cast<const uint32_t*>(c->d_refit_plan.p);
    ra.n_plan = n_plan;
    ra.corners = static_cast<const float4*>(c->d_corners.p);
    ra.n_slots = std::min(n_slots, (uint32_t)(c->d_corners.cap / 48u));
    ra.n_nodes = n_nodes;
    for (int v = 0; v < kVersions; ++v) {
        ra.nodes[v] = static_cast<float*>(c->d_nodes[v].p);
        ra.n_nodes = std::min(ra.n_nodes, (uint32_t)(c->d_nodes[v].cap / 32u));
    }
    ra.pairs = pairs ? static_cast<float*>(c->d_flow.p) : nullptr;
    ra.n_pairs = pairs ? c->flow.n_pairs : 0u;
    RT_HIP(rt_launch_refit_nodes(ra, c->stream));
    RT_HIP(hipEventRecord(c->ev_scene, c->stream));     // frames and queries on other streams wait for it (the scene-update event)
    c->scene_stream = c->stream;
    if (pairs_left_behind) c->flow_dirty = true;
    // ---- the mirror stays what the device holds: the boxes of the planned nodes, read back from version 0 ----
    const uint32_t lo = c->refit.lo, hi = c->refit.hi;
    std::vector<float> back((size_t)(hi - lo + 1u) * 8u);
    RT_HIP(hipMemcpyAsync(back.data(), static_cast<const char*>(c->d_nodes[0].p) + (size_t)lo * 32u, back.size() * 4u, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t e = 0; e < n_plan; ++e) {
        const uint32_t i = c->refit.plan[3u * e];
        const float* b = &back[(size_t)(i - lo) * 8u];
        float* m = &c->h_nodes[(size_t)i * 8u];
        m[0] = b[0]; m[1] = b[1]; m[2] = b[2]; m[4] = b[4]; m[5] = b[5]; m[6] = b[6];
        // a node inside the head of the buffer also lives in the copy that frames carry (apply_version writes it over the
        // versions): the same boxes there.  Not a per-frame write: inst.gen stays, the kernel has updated every version.
        if (i < c->inst.head_nodes && c->inst.head.size() >= (size_t)(i + 1u) * 8u) {
            float* h = &c->inst.head[(size_t)i * 8u];
            h[0] = b[0]; h[1] = b[1]; h[2] = b[2]; h[4] = b[4]; h[5] = b[5]; h[6] = b[6];
        }
    }
    return RT_OK;
}

int rt_read_nodes(rt_ctx* c, uint32_t first_node, uint32_t n, float* dst) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_nodes: ctx is NULL");
    if ((uint64_t)first_node + n > c->nodes_used / 32u) return fail(RT_ERR_INVALID_ARG, "rt_read_nodes: first_node + n is beyond the nodes written");
    if (n == 0u) return RT_OK;
    if (!dst) return fail(RT_ERR_INVALID_ARG, "rt_read_nodes: dst is NULL");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    // version 0: the one the next frame reads (the event ring is empty).  Per-frame writes of the head of the buffer that no
    // frame has carried to it yet are laid over the copy, as a frame or a query sees them.
    { int rc = grow_buf(c, c->d_nodes[0], c->nodes_used); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    RT_HIP(hipMemcpyAsync(dst, static_cast<const char*>(c->d_nodes[0].p) + (size_t)first_node * 32u, (size_t)n * 32u, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    const uint32_t head = std::min(c->inst.head_nodes, (uint32_t)(c->inst.head.size() / 8u));
    if (first_node < head) {
        const uint32_t m = std::min(n, head - first_node);
        std::memcpy(dst, &c->inst.head[(size_t)first_node * 8u], (size_t)m * 32u);
    }
    return RT_OK;
}

// ---- device mesh deformation (rt_deform.h: the arithmetic and the host model; rt_deform.hip: the kernel) -----------------------

extern "C++" { RtDeformLaunch rt_deform_launch = nullptr; }        // set by rt_deform.o (rt_deform.h)

int rt_deform_triangles_model(float* triangles, uint32_t n_triangles, uint32_t first, uint32_t n, const float* vertices, uint32_t V,
                              const uint32_t* faces, const float* normals, uint32_t flags) {
    const char* why = "";
    const int rc = rt_df_model(triangles, n_triangles, first, n, vertices, V, faces, normals, flags, &why);
    if (rc != RT_OK) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_deform_triangles_model: %s", why); return fail(rc, msg); }
    return RT_OK;
}

// A triangle write from device memory produced on `hip_stream`: rt_update_triangles' contract.  Drains, orders the context's
// stream behind the scene-update event and waits (the host does) for the caller's stream.
static int device_source_begin(rt_ctx* c, void* hip_stream) {
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    if (hip_stream) RT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
    return RT_OK;
}
// ... and its end: the scene-update event behind the work, and the work complete, so that the caller's arrays are free
static int device_source_end(rt_ctx* c) {
    RT_HIP(hipEventRecord(c->ev_scene, c->stream));     // frames and queries on other streams wait for it (the scene-update event)
    c->scene_stream = c->stream;
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}

// vertices / faces / normals: device memory the caller's stream `hip_stream` produced (device == true), or host memory
static int deform_triangles(rt_ctx* c, const char* who, uint32_t first, uint32_t n, const float* vertices, uint32_t V,
                            const uint32_t* faces, const float* normals, uint32_t flags, bool device, void* hip_stream) {
    char msg[200];
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (const char* bad = rt_df_check_flags(normals, flags)) { std::snprintf(msg, sizeof msg, "%s: %s", who, bad); return fail(RT_ERR_INVALID_ARG, msg); }
    if (c->scene_kind != 1 || !c->d_tri.used) { std::snprintf(msg, sizeof msg, "%s: no triangle scene (rt_write_triangles first)", who); return fail(RT_ERR_STATE, msg); }
    const uint32_t n_tri = (uint32_t)std::min(c->d_tri.used / 160u, c->d_tri.cap / 160u);
    if (!rt_df_in_range(first, n, n_tri)) { std::snprintf(msg, sizeof msg, "%s: first + n is beyond the triangles written", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (n == 0u) return RT_OK;
    if (const char* bad = rt_df_check_arrays(n, vertices, V, faces)) { std::snprintf(msg, sizeof msg, "%s: %s", who, bad); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && ((reinterpret_cast<uintptr_t>(vertices) | reinterpret_cast<uintptr_t>(faces) | reinterpret_cast<uintptr_t>(normals)) & 3u)) {
        std::snprintf(msg, sizeof msg, "%s: device pointers must be 4-byte aligned", who);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    { int rc = device_source_begin(c, device ? hip_stream : nullptr); if (rc != RT_OK) return rc; }
    RtDeformArgs a;
    a.tri = static_cast<float*>(c->d_tri.p); a.n_tri = n_tri; a.first = first; a.n = n;
    a.vertices = vertices; a.V = V; a.faces = faces; a.normals = normals; a.flags = flags;
    if (!device) {
        // staged: without faces only the first 3 n vertices (and normals) are read
        const size_t v_bytes = (size_t)(faces ? V : 3u * n) * 12u, f_bytes = faces ? (size_t)n * 12u : 0u, n_bytes = normals ? v_bytes : 0u;
        { int rc = grow_buf(c, c->d_deform, v_bytes + f_bytes + n_bytes); if (rc != RT_OK) return rc; }
        char* base = static_cast<char*>(c->d_deform.p);
        RT_HIP(hipMemcpyAsync(base, vertices, v_bytes, hipMemcpyHostToDevice, c->stream));
        if (faces) RT_HIP(hipMemcpyAsync(base + v_bytes, faces, f_bytes, hipMemcpyHostToDevice, c->stream));
        if (normals) RT_HIP(hipMemcpyAsync(base + v_bytes + f_bytes, normals, n_bytes, hipMemcpyHostToDevice, c->stream));
        RT_HIP(hipStreamSynchronize(c->stream));        // pageable sources
        a.vertices = reinterpret_cast<const float*>(base);
        a.faces = faces ? reinterpret_cast<const uint32_t*>(base + v_bytes) : nullptr;
        a.normals = normals ? reinterpret_cast<const float*>(base + v_bytes + f_bytes) : nullptr;
    }
    // the corner array follows: rebuilt whole by the next refit, frame or query (ensure_corners), as after rt_update_triangles
    c->corners_valid = false;
    if (!rt_deform_launch) return fail(RT_ERR_UNSUPPORTED, "rt_deform_triangles: this build holds no deformation kernel (rt_deform.o is not linked)");
    RT_HIP(rt_deform_launch(a, c->stream));
    return device_source_end(c);
}

int rt_deform_triangles(rt_ctx* c, uint32_t first, uint32_t n, const float* vertices, uint32_t V, const uint32_t* faces,
                        const float* normals, uint32_t flags, void* hip_stream) {
    return deform_triangles(c, "rt_deform_triangles", first, n, vertices, V, faces, normals, flags, true, hip_stream);
}
int rt_deform_triangles_host(rt_ctx* c, uint32_t first, uint32_t n, const float* vertices, uint32_t V, const uint32_t* faces,
                             const float* normals, uint32_t flags) {
    return deform_triangles(c, "rt_deform_triangles_host", first, n, vertices, V, faces, normals, flags, false, nullptr);
}

int rt_update_triangles_device(rt_ctx* c, uint32_t first, uint32_t n, const float* records_dev, void* hip_stream) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles_device: ctx is NULL");
    if (c->scene_kind != 1 || !c->d_tri.used) return fail(RT_ERR_STATE, "rt_update_triangles_device: no triangle scene (rt_write_triangles first)");
    if ((uint64_t)first + n > std::min(c->d_tri.used, c->d_tri.cap) / 160u) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles_device: first + n is beyond the triangles written");
    if (n == 0u) return RT_OK;
    if (!records_dev) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles_device: records_dev is NULL");
    if (reinterpret_cast<uintptr_t>(records_dev) & 3u) return fail(RT_ERR_INVALID_ARG, "rt_update_triangles_device: records_dev must be 4-byte aligned");
    { int rc = device_source_begin(c, hip_stream); if (rc != RT_OK) return rc; }
    c->corners_valid = false;                           // as rt_update_triangles
    RT_HIP(hipMemcpyAsync(static_cast<char*>(c->d_tri.p) + (size_t)first * 160u, records_dev, (size_t)n * 160u, hipMemcpyDeviceToDevice, c->stream));
    return device_source_end(c);
}

int rt_read_triangles(rt_ctx* c, uint32_t first, uint32_t n, float* dst) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_triangles: ctx is NULL");
    if ((uint64_t)first + n > c->d_tri.used / 160u) return fail(RT_ERR_INVALID_ARG, "rt_read_triangles: first + n is beyond the triangles written");
    if (n == 0u) return RT_OK;
    if (!dst) return fail(RT_ERR_INVALID_ARG, "rt_read_triangles: dst is NULL");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    RT_HIP(hipMemcpyAsync(dst, static_cast<const char*>(c->d_tri.p) + (size_t)first * 160u, (size_t)n * 160u, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}

// ---- device BLAS builds (rt_blas_build.h: the arithmetic and the host model; rt_build.hip: the kernels) -------------------------

static_assert(kBuildVersions == (uint32_t)kVersions, "rt_build.hip stores into every version of the node buffer");

int rt_build_blas_host(const float* triangles, uint32_t n_triangles, float* tri_lookup, uint32_t n_tri_lookup, float* nodes,
                       uint32_t n_nodes, const rt_blas_range* ranges, uint32_t n, uint32_t* used) {
    const char* why = "";
    const int rc = rt_bb_build_host(triangles, n_triangles, tri_lookup, n_tri_lookup, nodes, n_nodes, ranges, n, used, &why);
    if (rc != RT_OK) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_build_blas_host: %s", why); return fail(rc, msg); }
    return RT_OK;
}

// The levels of a build whose level 0 (`n_roots` nodes) the prep pass has made: price, scan and split per level -- the host learns
// one word per level, the next level's node count -- and then the splits per subtree, last level first.  off / cnt: where each
// level lies among the build nodes; the last entry is the empty level.
static int build_levels(const char* who, const RtBuildArgs& ba, uint32_t n_roots, hipStream_t s, std::vector<uint32_t>& off, std::vector<uint32_t>& cnt) {
    off.assign(1, 0u);
    cnt.assign(1, n_roots);
    while (cnt.back() != 0u) {
        const uint32_t level = (uint32_t)cnt.size() - 1u;
        RT_HIP(rt_launch_build_level(ba, level, off[level], cnt[level], s));
        uint32_t next = 0u;
        RT_HIP(hipMemcpyAsync(&next, ba.next_count, 4u, hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        const uint32_t o = off[level] + cnt[level];
        if (next > ba.node_cap - o) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "%s: a level beyond the build's node capacity (corrupt scratch state)", who);
            return fail(RT_ERR_HIP, msg);
        }
        off.push_back(o);
        cnt.push_back(next);
    }
    for (uint32_t l = (uint32_t)cnt.size() - 1u; l-- > 0u;) RT_HIP(rt_launch_build_count_up(ba, off[l], cnt[l], s));
    return RT_OK;
}

int rt_build_blas(rt_ctx* c, const rt_blas_range* ranges, uint32_t n, uint32_t* used) {
    if (!c || (!ranges && n)) return fail(RT_ERR_INVALID_ARG, "rt_build_blas: NULL argument");
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u), n_slots = (uint32_t)(c->d_tri_lookup.used / 4u);
    const uint32_t n_tri = (uint32_t)(c->d_tri.used / 160u);
    if (c->scene_kind != 1 || !n_tri || !n_nodes || !n_slots || c->h_nodes.size() / 8u < n_nodes)
        return fail(RT_ERR_STATE, "rt_build_blas: no triangle scene (rt_write_triangles, _nodes and _tri_lookup first)");
    if (n == 0u) return RT_OK;
    if (const char* bad = rt_bb_check_ranges(ranges, n, n_nodes, n_slots)) {
        char msg[200]; std::snprintf(msg, sizeof msg, "rt_build_blas: %s", bad); return fail(RT_ERR_INVALID_ARG, msg);
    }
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    for (int v = 0; v < kVersions; ++v) { int rc = grow_buf(c, c->d_nodes[v], c->nodes_used); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    // ---- scratch: 2 n_slots - 1 build nodes per range always suffice (a split leaves both sides non-empty) ----
    uint64_t cap64 = 0;
    for (uint32_t i = 0; i < n; ++i) cap64 += 2u * (uint64_t)ranges[i].n_slots - 1u;
    if (cap64 > 0x7FFFFFFFu) return fail(RT_ERR_CAPACITY, "rt_build_blas: too many lookup slots for one call");
    const uint32_t node_cap = (uint32_t)cap64;
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o = at; at += (bytes + 15u) & ~(size_t)15u; return o; };
    const size_t o_ranges = carve((size_t)n * sizeof(rt_blas_range)), o_prim = carve((size_t)n_slots * sizeof(RtBbPrim));
    const size_t o_ord0 = carve((size_t)n_slots * 4u), o_ord1 = carve((size_t)n_slots * 4u), o_final = carve((size_t)n_slots * 4u);
    const size_t o_node = carve((size_t)node_cap * sizeof(RtBuildNode)), o_dec = carve((size_t)node_cap * sizeof(RtBuildDec));
    const size_t o_sub = carve((size_t)node_cap * 4u), o_rank = carve((size_t)node_cap * 4u), o_index = carve((size_t)node_cap * 4u);
    const size_t o_root = carve((size_t)node_cap * 4u), o_next = carve(4u);
    { int rc = grow_buf(c, c->d_build, at); if (rc != RT_OK) return rc; }
    char* base = static_cast<char*>(c->d_build.p);
    RtBuildArgs ba;
    ba.tri = static_cast<const float*>(c->d_tri.p); ba.n_tri = n_tri;
    ba.lookup = static_cast<float*>(c->d_tri_lookup.p); ba.n_slots = std::min(n_slots, (uint32_t)(c->d_tri_lookup.cap / 4u));
    ba.n_nodes = n_nodes;
    for (int v = 0; v < kVersions; ++v) {
        ba.nodes[v] = static_cast<float*>(c->d_nodes[v].p);
        ba.n_nodes = std::min(ba.n_nodes, (uint32_t)(c->d_nodes[v].cap / 32u));
    }
    ba.ranges = reinterpret_cast<const rt_blas_range*>(base + o_ranges); ba.n_ranges = n;
    ba.prim = reinterpret_cast<RtBbPrim*>(base + o_prim);
    ba.order[0] = reinterpret_cast<uint32_t*>(base + o_ord0); ba.order[1] = reinterpret_cast<uint32_t*>(base + o_ord1);
    ba.final_order = reinterpret_cast<uint32_t*>(base + o_final);
    ba.node = reinterpret_cast<RtBuildNode*>(base + o_node); ba.dec = reinterpret_cast<RtBuildDec*>(base + o_dec);
    ba.sub = reinterpret_cast<uint32_t*>(base + o_sub); ba.rank = reinterpret_cast<uint32_t*>(base + o_rank);
    ba.index = reinterpret_cast<uint32_t*>(base + o_index); ba.root = reinterpret_cast<uint32_t*>(base + o_root);
    ba.node_cap = node_cap;
    ba.next_count = reinterpret_cast<uint32_t*>(base + o_next);
    hipStream_t s = c->stream;
    RT_HIP(hipMemcpyAsync(base + o_ranges, ranges, (size_t)n * sizeof(rt_blas_range), hipMemcpyHostToDevice, s));
    RT_HIP(hipStreamSynchronize(s));                    // a pageable source
    // ---- the levels: the host learns one word per level, the next level's node count ----
    RT_HIP(rt_launch_build_prep(ba, ranges, s));
    std::vector<uint32_t> off, cnt;
    { int rc = build_levels("rt_build_blas", ba, n, s, off, cnt); if (rc != RT_OK) return rc; }
    const uint32_t levels = (uint32_t)cnt.size() - 1u;  // the last entry is the empty level
    // ---- sizing before committing: nothing of the scene has been written so far ----
    std::vector<uint32_t> sub(n);
    RT_HIP(hipMemcpyAsync(sub.data(), ba.sub, (size_t)n * 4u, hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    bool fits = true;
    uint32_t worst = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t u = 1u + 2u * sub[i];
        if (used) used[i] = u;
        if (u > ranges[i].node_cap) { if (fits) worst = i; fits = false; }
    }
    if (!fits) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "rt_build_blas: the tree of range %u needs %u nodes, its node_cap is %u", worst, 1u + 2u * sub[worst], ranges[worst].node_cap);
        return fail(RT_ERR_CAPACITY, msg);
    }
    for (uint32_t l = 0; l < levels; ++l) RT_HIP(rt_launch_build_rank_down(ba, off[l], cnt[l], s));
    for (uint32_t l = 0; l < levels; ++l) RT_HIP(rt_launch_build_emit_nodes(ba, off[l], cnt[l], s));
    RT_HIP(rt_launch_build_emit_lookup(ba, ranges, s));
    RT_HIP(hipEventRecord(c->ev_scene, s));             // frames and queries on other streams wait for it (the scene-update event)
    c->scene_stream = s;
    // ---- the mirror follows: whole records, read back from version 0 ----
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t u = 1u + 2u * sub[i];
        RT_HIP(hipMemcpyAsync(&c->h_nodes[(size_t)ranges[i].root_node * 8u], static_cast<const char*>(c->d_nodes[0].p) + (size_t)ranges[i].root_node * 32u,
                              (size_t)u * 32u, hipMemcpyDeviceToHost, s));
    }
    RT_HIP(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r0 = ranges[i].root_node, u = 1u + 2u * sub[i];
        for (uint32_t k = r0; k < r0 + u; ++k) c->node_count_max = std::max(c->node_count_max, rt_flow_u32f(c->h_nodes[(size_t)k * 8u + 7u]));
        // nodes inside the head of the buffer also live in the copy that frames carry (apply_version writes it over the versions)
        const uint32_t head = std::min(c->inst.head_nodes, (uint32_t)(c->inst.head.size() / 8u));
        if (r0 < head) std::memcpy(&c->inst.head[(size_t)r0 * 8u], &c->h_nodes[(size_t)r0 * 8u], (size_t)std::min(u, head - r0) * 32u);
    }
    ++c->topo_gen;                                      // a refit plan rests on the structure
    c->flow_dirty = true;                               // a node write reached the trees: the next frame rebuilds the pair records
    c->corners_valid = false;                           // the lookup table moved
    return RT_OK;
}

int rt_read_tri_lookup(rt_ctx* c, uint32_t first_slot, uint32_t n, float* dst) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_tri_lookup: ctx is NULL");
    if ((uint64_t)first_slot + n > c->d_tri_lookup.used / 4u) return fail(RT_ERR_INVALID_ARG, "rt_read_tri_lookup: first_slot + n is beyond the slots written");
    if (n == 0u) return RT_OK;
    if (!dst) return fail(RT_ERR_INVALID_ARG, "rt_read_tri_lookup: dst is NULL");
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    RT_HIP(hipMemcpyAsync(dst, static_cast<const char*>(c->d_tri_lookup.p) + (size_t)first_slot * 4u, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}

// ---- device top-level builds (rt_tlas_build.h: the arithmetic and the host model; rt_tlas.hip: the front end of rt_build.hip) ----

int rt_build_tlas_host(const float* models, const uint32_t* roots, uint32_t n, const float* nodes, uint32_t n_nodes,
                       float* tlas_nodes, float* blas, float* blas_lookup, uint32_t node_cap, rt_tlas_info* info) {
    const char* why = "";
    const int rc = rt_tl_build_host(models, roots, n, nodes, n_nodes, tlas_nodes, blas, blas_lookup, node_cap, info, &why);
    if (rc != RT_OK) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_build_tlas_host: %s", why); return fail(rc, msg); }
    return RT_OK;
}

// models: host memory (device == false) or device memory the caller's stream `hip_stream` produced
static int build_tlas(rt_ctx* c, const char* who, const float* models, bool device, void* hip_stream, const uint32_t* roots, uint32_t n,
                      uint32_t node_cap, rt_tlas_info* info) {
    char msg[200];
    if (!c || !models || !roots) { std::snprintf(msg, sizeof msg, "%s: NULL argument", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && (reinterpret_cast<uintptr_t>(models) & 15u)) { std::snprintf(msg, sizeof msg, "%s: models_dev must be 16-byte aligned", who); return fail(RT_ERR_INVALID_ARG, msg); }
    const uint32_t n_nodes = (uint32_t)(c->nodes_used / 32u);
    if (c->scene_kind != 1 || !n_nodes) {
        std::snprintf(msg, sizeof msg, "%s: no triangle scene (rt_write_nodes first: the roots' boxes are read from it)", who);
        return fail(RT_ERR_STATE, msg);
    }
    if (const char* bad = rt_tl_check_args(roots, n, node_cap, n_nodes)) { std::snprintf(msg, sizeof msg, "%s: %s", who, bad); return fail(RT_ERR_INVALID_ARG, msg); }
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    { int rc = grow_buf(c, c->d_nodes[0], c->nodes_used); if (rc != RT_OK) return rc; }
    hipStream_t s = c->stream;
    if (c->scene_stream && c->scene_stream != s) RT_HIP(hipStreamWaitEvent(s, c->ev_scene, 0));
    if (device && hip_stream) RT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
    // a root inside the head of the node buffer may so far live only in the copy that frames carry: version 0 (nothing is in
    // flight) takes the host's current state first, as it does for a query (query_prepare)
    if (c->ver_gen[0] != c->inst.gen && *std::min_element(roots, roots + n) < c->inst.head_nodes) {
        int rc = apply_version(c, 0u, 0u, s);
        if (rc != RT_OK) return rc;
    }
    // ---- scratch: everything is built aside; 2 n - 1 build nodes always suffice ----
    const uint32_t cap = 2u * n - 1u;
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o = at; at += (bytes + 15u) & ~(size_t)15u; return o; };
    const size_t o_range = carve(sizeof(rt_blas_range)), o_models = carve(device ? 0u : (size_t)n * 64u), o_roots = carve((size_t)n * 4u);
    const size_t o_blas = carve((size_t)n * 80u), o_lookup = carve((size_t)n * 4u), o_nodes = carve((size_t)cap * 32u);
    const size_t o_prim = carve((size_t)n * sizeof(RtBbPrim));
    const size_t o_ord0 = carve((size_t)n * 4u), o_ord1 = carve((size_t)n * 4u), o_final = carve((size_t)n * 4u);
    const size_t o_node = carve((size_t)cap * sizeof(RtBuildNode)), o_dec = carve((size_t)cap * sizeof(RtBuildDec));
    const size_t o_sub = carve((size_t)cap * 4u), o_rank = carve((size_t)cap * 4u), o_index = carve((size_t)cap * 4u);
    const size_t o_root = carve((size_t)cap * 4u), o_next = carve(4u);
    { int rc = grow_buf(c, c->d_build, at); if (rc != RT_OK) return rc; }
    char* base = static_cast<char*>(c->d_build.p);
    const rt_blas_range range = {0u, cap, 0u, n};
    RtBuildArgs ba;
    ba.tri = nullptr; ba.n_tri = 0u;
    ba.lookup = reinterpret_cast<float*>(base + o_lookup); ba.n_slots = n;
    for (uint32_t v = 0; v < kBuildVersions; ++v) ba.nodes[v] = nullptr;
    ba.nodes[0] = reinterpret_cast<float*>(base + o_nodes); ba.n_nodes = cap;
    ba.ranges = reinterpret_cast<const rt_blas_range*>(base + o_range); ba.n_ranges = 1u;
    ba.prim = reinterpret_cast<RtBbPrim*>(base + o_prim);
    ba.order[0] = reinterpret_cast<uint32_t*>(base + o_ord0); ba.order[1] = reinterpret_cast<uint32_t*>(base + o_ord1);
    ba.final_order = reinterpret_cast<uint32_t*>(base + o_final);
    ba.node = reinterpret_cast<RtBuildNode*>(base + o_node); ba.dec = reinterpret_cast<RtBuildDec*>(base + o_dec);
    ba.sub = reinterpret_cast<uint32_t*>(base + o_sub); ba.rank = reinterpret_cast<uint32_t*>(base + o_rank);
    ba.index = reinterpret_cast<uint32_t*>(base + o_index); ba.root = reinterpret_cast<uint32_t*>(base + o_root);
    ba.node_cap = cap;
    ba.next_count = reinterpret_cast<uint32_t*>(base + o_next);
    ba.inst.models = device ? models : reinterpret_cast<const float*>(base + o_models);
    ba.inst.roots = reinterpret_cast<const uint32_t*>(base + o_roots);
    ba.inst.nodes = static_cast<const float*>(c->d_nodes[0].p);
    ba.inst.n_nodes = std::min(n_nodes, (uint32_t)(c->d_nodes[0].cap / 32u));
    ba.inst.blas = reinterpret_cast<float*>(base + o_blas);
    RT_HIP(hipMemcpyAsync(base + o_range, &range, sizeof range, hipMemcpyHostToDevice, s));
    if (!device) RT_HIP(hipMemcpyAsync(base + o_models, models, (size_t)n * 64u, hipMemcpyHostToDevice, s));
    RT_HIP(hipMemcpyAsync(base + o_roots, roots, (size_t)n * 4u, hipMemcpyHostToDevice, s));
    RT_HIP(hipStreamSynchronize(s));                    // pageable sources
    // ---- the levels: the host learns one word per level, the next level's node count ----
    RT_HIP(rt_launch_build_prep(ba, &range, s));            // a.inst is set: rt_tlas.hip makes the prims
    std::vector<uint32_t> off, cnt;
    { int rc = build_levels(who, ba, 1u, s, off, cnt); if (rc != RT_OK) return rc; }
    const uint32_t levels = (uint32_t)cnt.size() - 1u, used = off.back();       // every build node becomes one node of the tree
    for (uint32_t l = 0; l < levels; ++l) RT_HIP(rt_launch_build_rank_down(ba, off[l], cnt[l], s));
    for (uint32_t l = 0; l < levels; ++l) RT_HIP(rt_launch_build_emit_nodes(ba, off[l], cnt[l], s));
    RT_HIP(rt_launch_build_emit_lookup(ba, &range, s));
    // ---- read back, judge, and only then commit: as the three writes of the same bytes ----
    std::vector<float> h_nodes((size_t)std::max(used, node_cap) * 8u, 0.0f), h_blas((size_t)n * 20u), h_lookup(n);
    RT_HIP(hipMemcpyAsync(h_nodes.data(), base + o_nodes, (size_t)used * 32u, hipMemcpyDeviceToHost, s));
    RT_HIP(hipMemcpyAsync(h_blas.data(), base + o_blas, (size_t)n * 80u, hipMemcpyDeviceToHost, s));
    RT_HIP(hipMemcpyAsync(h_lookup.data(), base + o_lookup, (size_t)n * 4u, hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    const rt_tlas_info got = rt_tl_info(h_nodes.data(), used);
    if (info) *info = got;
    const char* why = "";
    if (const int rc = rt_tl_verdict(got, node_cap, &why)) {
        std::snprintf(msg, sizeof msg, "%s: %s (%u nodes, depth %u; node_cap %u)", who, why, got.nodes_used, got.depth, node_cap);
        return fail(rc, msg);
    }
    { int rc = rt_write_blas(c, h_blas.data(), n); if (rc != RT_OK) return rc; }
    { int rc = rt_write_blas_lookup(c, h_lookup.data(), n); if (rc != RT_OK) return rc; }
    return rt_write_nodes(c, 0, h_nodes.data(), node_cap);
}

int rt_build_tlas(rt_ctx* c, const float* models, const uint32_t* roots, uint32_t n, uint32_t node_cap, rt_tlas_info* info) {
    return build_tlas(c, "rt_build_tlas", models, false, nullptr, roots, n, node_cap, info);
}
int rt_build_tlas_device(rt_ctx* c, const float* models_dev, const uint32_t* roots, uint32_t n, uint32_t node_cap, rt_tlas_info* info,
                         void* hip_stream) {
    return build_tlas(c, "rt_build_tlas_device", models_dev, true, hip_stream, roots, n, node_cap, info);
}

// the BLAS records / the BLAS lookup words the next frame would read: the host's per-frame copy where frames carry it, else version 0
static int read_instances(rt_ctx* c, const char* who, bool on, const std::vector<float>& carried, const rt_ctx::DevBuf& dev, uint32_t words,
                          uint32_t first, uint32_t n, float* dst) {
    char msg[160];
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    const size_t have = on ? carried.size() / words : dev.used / (4u * (size_t)words);
    if ((uint64_t)first + n > have) { std::snprintf(msg, sizeof msg, "%s: first + n is beyond what was written", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (n == 0u) return RT_OK;
    if (!dst) { std::snprintf(msg, sizeof msg, "%s: dst is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    RT_HIP(hipSetDevice(c->device));
    { int rc = drain(c); if (rc != RT_OK) return rc; }
    if (on) { std::memcpy(dst, &carried[(size_t)first * words], (size_t)n * words * 4u); return RT_OK; }
    if (c->scene_stream && c->scene_stream != c->stream) RT_HIP(hipStreamWaitEvent(c->stream, c->ev_scene, 0));
    RT_HIP(hipMemcpyAsync(dst, static_cast<const char*>(dev.p) + (size_t)first * words * 4u, (size_t)n * words * 4u, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(hipStreamSynchronize(c->stream));
    return RT_OK;
}
int rt_read_blas(rt_ctx* c, uint32_t first, uint32_t n, float* dst) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_blas: ctx is NULL");
    return read_instances(c, "rt_read_blas", c->inst.blas_on, c->inst.blas, c->d_blas[0], 20u, first, n, dst);
}
int rt_read_blas_lookup(rt_ctx* c, uint32_t first, uint32_t n, float* dst) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_read_blas_lookup: ctx is NULL");
    return read_instances(c, "rt_read_blas_lookup", c->inst.lookup_on, c->inst.lookup, c->d_blas_lookup[0], 1u, first, n, dst);
}

int rt_filter_plan(const float* records, uint32_t n, const float params[24], int* filter_ok, int* signed_filter) {
    if ((n && !records) || !params || !filter_ok || !signed_filter) return fail(RT_ERR_INVALID_ARG, "rt_filter_plan: NULL argument");
    bool ok = false;
    uint32_t sgn = 0;
    rt_plan((double)(float)rt_scene_bound(records, n), rt_scene_min_radius(records, n), params, ok, sgn);
    *filter_ok = ok ? 1 : 0;
    *signed_filter = (int)sgn;
    return RT_OK;
}

// ---- ray queries (rt_query.hip) ------------------------------------------------------------------------------------------

// Is there a scene for a query to read?  (query_prepare's first check; rt_render_samples asks before it looks at capacities)
static int query_scene_written(rt_ctx* c, const char* who) {
    char msg[160];
    if (c->scene_kind == 1) {
        const bool have_blas = c->inst.blas_on ? !c->inst.blas.empty() : c->d_blas[0].used != 0;
        const bool have_lookup = c->inst.lookup_on ? !c->inst.lookup.empty() : c->d_blas_lookup[0].used != 0;
        if (!c->d_tri.used || !c->nodes_used || !have_blas || !c->d_tri_lookup.used || !have_lookup) {
            std::snprintf(msg, sizeof msg, "%s: a triangle scene needs rt_write_triangles, _nodes, _blas, _tri_lookup and _blas_lookup", who);
            return fail(RT_ERR_STATE, msg);
        }
    } else if (!c->have_spheres) {
        std::snprintf(msg, sizeof msg, "%s: no scene has been written", who);
        return fail(RT_ERR_STATE, msg);
    }
    return RT_OK;
}
// What a query on `s` reads, and its order behind the last scene update.  Triangle scenes: `ts`, with the instance data in the
// arguments (*inst = 1) when it travels with the frames -- the per-frame buffers then hold an older pose -- and otherwise from a
// version of the per-frame buffers that holds the current state (every version, for instance sets written by write_versions).
static int query_prepare(rt_ctx* c, const char* who, hipStream_t s, bool& tri, RtTriScene& ts, int& inst) {
    { int rc = query_scene_written(c, who); if (rc != RT_OK) return rc; }
    tri = c->scene_kind == 1;
    inst = 0;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(c->ev_query.ensure(hipEventDisableTiming));
    if (tri) { int rc = ensure_corners(c, s); if (rc != RT_OK) return rc; }
    uint32_t v = 0;
    uint32_t root_meta[kInstMax] = {0};
    bool have_pairs = false;
    if (tri) {
        const uint32_t n_inst = (uint32_t)(c->inst.blas.size() / 20u);
        // (a lookup table longer than the instance list names entries that are not staged: the versions then)
        inst = (c->inst.blas_on && c->inst.lookup_on && n_inst >= 1u && c->inst.lookup.size() <= n_inst) ? 1 : 0;
        if (inst) {
            uint32_t roots[kInstMax], n_roots = 0;
            if (tri_pair_roots(c, roots, n_roots)) have_pairs = tri_pairs_current(c, roots, n_roots, root_meta);
        } else {
            int cur = -1;
            for (int k = 0; k < kVersions && cur < 0; ++k)
                if (c->ver_gen[k] == c->inst.gen) cur = k;
            if (cur < 0) {
                // no version holds the current state (a per-frame write since the last frame of the twenty-slot form): bring one
                // up to date -- with nothing in flight, as a frame of this scene after rt_write_blas / _blas_lookup of more than
                // sixteen instances finds it (they drain)
                { int rc = drain(c); if (rc != RT_OK) return rc; }
                cur = 0;
                { int rc = apply_version(c, 0u, 0u, s); if (rc != RT_OK) return rc; }
            } else if (c->ev_ver[cur] && c->ver_stream[cur] != s) {
                RT_HIP(hipStreamWaitEvent(s, c->ev_ver[cur], 0));
            }
            v = (uint32_t)cur;
            c->query_versions = true;
        }
    }
    if (c->scene_stream && c->scene_stream != s) RT_HIP(hipStreamWaitEvent(s, c->ev_scene, 0));
    // queries on different streams run in order: ev_query then stands for all of them (rt_drain)
    if (c->query_pending && c->query_last != s) RT_HIP(hipStreamWaitEvent(s, c->ev_query, 0));
    if (tri) {
        std::memset(&ts, 0, sizeof ts);
        tri_scene(c, v, have_pairs, root_meta, ts);
        if (inst) tri_fill_inst(c, ts);
    }
    return RT_OK;
}

extern "C++" {     // (templates below)

// A query between query_open and query_close: the stream it runs on and what it reads there
struct Query {
    hipStream_t s;
    bool tri;
    int inst;
    RtQueryScene ts;     // ... with the instance masks and the context's two ray masks, copied here: at the call
};

// Opens a query: its stream, and query_prepare on it.  Results in device memory: `hip_stream`, or the context's own when that is
// NULL.  The host-memory forms (host): the context's query stream, made at its first use.
static int query_open(rt_ctx* c, const char* who, bool host, void* hip_stream, Query& q) {
    if (host) {
        RT_HIP(hipSetDevice(c->device));
        RT_HIP(c->query_stream.ensure(hipStreamNonBlocking));
        q.s = c->query_stream;
    } else {
        q.s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    }
    q.ts.mask.table = c->d_masks.as<uint32_t>();
    q.ts.mask.n = (uint32_t)c->h_masks.size();
    q.ts.mask.nearest = c->mask_nearest;
    q.ts.mask.occlusion = c->mask_occlusion;
    return query_prepare(c, who, q.s, q.tri, q.ts, q.inst);
}
// Closes it behind the kernels launched on q.s: what the next query on another stream, and rt_drain, wait for
static int query_close(rt_ctx* c, const Query& q) {
    RT_HIP(hipEventRecord(c->ev_query, q.s));
    c->query_pending = true;
    c->query_last = q.s;
    return RT_OK;
}

// A query with its results in device memory: launch(q) between open and close
template <typename LAUNCH>
static int query_run(rt_ctx* c, const char* who, void* hip_stream, LAUNCH launch) {
    Query q;
    { int rc = query_open(c, who, false, hip_stream, q); if (rc != RT_OK) return rc; }
    { int rc = launch(q); if (rc != RT_OK) return rc; }
    return query_close(c, q);
}

// a staging buffer of the host-memory queries (synchronous: idle between calls): grows, contents not kept
static int grow_staging(rt_ctx::DevBuf& b, size_t need) {
    if (need <= b.cap) return RT_OK;
    RT_HIP(b.replace(std::max(need, (size_t)65536u)));
    return RT_OK;
}

// One result of a host-memory query: `bytes` from the staging buffer `buf` to `host` (NULL: not asked for).  Results that share a
// buffer stand together in the list and lie in the buffer one after the other, in the list's order.  dev: where, once staged.
struct Staged {
    void* host;
    rt_ctx::DevBuf* buf;
    size_t bytes;
    uint8_t* dev;
};

// A query with its results in host memory, synchronous, through the context's staging buffers: grow them, copy `in` (the rays or
// pixels of the call; NULL: none) to in_buf, launch(q) between open and close, copy every result back, wait.
template <size_t N, typename LAUNCH>
static int query_run_host(rt_ctx* c, const char* who, const void* in, rt_ctx::DevBuf* in_buf, size_t in_bytes, Staged (&out)[N], LAUNCH launch) {
    Query q;
    { int rc = query_open(c, who, true, nullptr, q); if (rc != RT_OK) return rc; }
    if (in) { int rc = grow_staging(*in_buf, in_bytes); if (rc != RT_OK) return rc; }
    size_t at[N], end = 0u;
    for (size_t i = 0; i < N; ++i) {
        if (i && out[i].buf != out[i - 1u].buf) end = 0u;
        at[i] = end;
        if (out[i].host) end += out[i].bytes;
        if (i + 1u == N || out[i + 1u].buf != out[i].buf) { int rc = grow_staging(*out[i].buf, end); if (rc != RT_OK) return rc; }
    }
    for (size_t i = 0; i < N; ++i) out[i].dev = out[i].host ? static_cast<uint8_t*>(out[i].buf->p) + at[i] : nullptr;
    if (in) RT_HIP(hipMemcpyAsync(in_buf->p, in, in_bytes, hipMemcpyHostToDevice, q.s));
    { int rc = launch(q); if (rc != RT_OK) return rc; }
    { int rc = query_close(c, q); if (rc != RT_OK) return rc; }
    for (size_t i = 0; i < N; ++i)
        if (out[i].host) RT_HIP(hipMemcpyAsync(out[i].host, out[i].dev, out[i].bytes, hipMemcpyDeviceToHost, q.s));
    RT_HIP(hipStreamSynchronize(q.s));
    return RT_OK;
}

}  // extern "C++"

// The checks every ray-array query starts with, in the header's order: the flags against `allowed` (a pure argument check,
// whatever the context); k, in the call that has one (NULL: none); the context; n == 0 (*done: nothing to do); the pointers; and
// for device memory the alignment `aligned` names in the message -- 16 bytes for `rays`, out_align for `out` (1: a byte per ray).
// aligned NULL: host memory, any address.
static int rays_check(const char* who, rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint32_t allowed, const uint32_t* k,
                      const void* out, const char* aligned, uint32_t out_align, bool& done) {
    char msg[160];
    done = false;
    if (flags & ~allowed) { std::snprintf(msg, sizeof msg, "%s: unknown flag bits 0x%x", who, flags); return fail(RT_ERR_INVALID_ARG, msg); }
    if (k && (*k == 0u || *k > RT355_MAX_HITS)) {
        std::snprintf(msg, sizeof msg, "%s: k = %u is outside 1 .. RT355_MAX_HITS (%u)", who, *k, RT355_MAX_HITS);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (n == 0) { done = true; return RT_OK; }
    if (!rays || !out) { std::snprintf(msg, sizeof msg, "%s: NULL argument", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (aligned && (reinterpret_cast<uintptr_t>(rays) % 16u || reinterpret_cast<uintptr_t>(out) % out_align)) {
        std::snprintf(msg, sizeof msg, "%s: %s must be 16-byte aligned", who, aligned);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    return RT_OK;
}

// The camera of the last rt_write_params in a kernel's arguments, for a frame of W x H; everything else zero
static void camera_frame_args(const rt_ctx* c, uint32_t W, uint32_t H, RtFrameArgs& fa) {
    std::memset(&fa, 0, sizeof fa);
    std::memcpy(fa.p, c->params, sizeof fa.p);
    fa.W = W; fa.H = H;
}

static_assert(sizeof(rt_hit) == 32, "rt_hit is two float4");

// flags (RT_QUERY_LIMITS) or `any` (rt_occluded: `out` is one byte per ray): the limited forms; otherwise rt_trace_rays' own
static int query_launch(rt_ctx* c, const float4* rays, void* out, uint32_t n, const Query& q, uint32_t flags = 0u, bool any = false) {
    if (!flags && !any) {
        float4* hits = static_cast<float4*>(out);
        if (q.tri) RT_HIP(rt_launch_query_triangles(q.ts, q.inst, rays, hits, n, q.s));
        else RT_HIP(rt_launch_query_spheres(c->d_records.as<float>(), c->n, rays, hits, n, q.s));
    } else {
        if (q.tri) RT_HIP(rt_launch_limited_triangles(q.ts, q.inst, rays, flags, any, out, n, q.s));
        else RT_HIP(rt_launch_limited_spheres(c->d_records.as<float>(), c->n, rays, flags, any, out, n, q.s));
    }
    return RT_OK;
}

// rt_trace_rays_ex / rt_occluded: device memory, on `hip_stream`; `out` holds n rt_hit records, or n bytes when `any`
static int query_device(const char* who, rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, bool any, void* out, void* hip_stream) {
    bool done;
    { int rc = rays_check(who, c, rays, n, flags, RT_QUERY_LIMITS, nullptr, out, any ? "rays" : "rays and hits", any ? 1u : 16u, done);
      if (rc != RT_OK || done) return rc; }
    return query_run(c, who, hip_stream, [&](const Query& q) { return query_launch(c, reinterpret_cast<const float4*>(rays), out, n, q, flags, any); });
}

// rt_trace_rays_host_ex / rt_occluded_host: host memory, staged through the context's query buffers, synchronous
static int query_host(const char* who, rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, bool any, void* out) {
    bool done;
    { int rc = rays_check(who, c, rays, n, flags, RT_QUERY_LIMITS, nullptr, out, nullptr, 1u, done); if (rc != RT_OK || done) return rc; }
    Staged r[] = {{out, &c->d_qhits, any ? (size_t)n : (size_t)n * 32u}};
    return query_run_host(c, who, rays, &c->d_qrays, (size_t)n * 32u, r, [&](const Query& q) {
        return query_launch(c, static_cast<const float4*>(c->d_qrays.p), r[0].dev, n, q, flags, any);
    });
}

int rt_trace_rays_ex(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, rt_hit* hits, void* hip_stream) {
    return query_device("rt_trace_rays_ex", c, rays, n, flags, false, hits, hip_stream);
}
int rt_trace_rays_host_ex(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, rt_hit* hits) {
    return query_host("rt_trace_rays_host_ex", c, rays, n, flags, false, hits);
}
int rt_occluded(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint8_t* occluded, void* hip_stream) {
    return query_device("rt_occluded", c, rays, n, flags, true, occluded, hip_stream);
}
int rt_occluded_host(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint8_t* occluded) {
    return query_host("rt_occluded_host", c, rays, n, flags, true, occluded);
}

int rt_trace_rays(rt_ctx* c, const float* rays, uint32_t n, rt_hit* hits, void* hip_stream) {
    return query_device("rt_trace_rays", c, rays, n, 0u, false, hits, hip_stream);
}

int rt_trace_rays_host(rt_ctx* c, const float* rays, uint32_t n, rt_hit* hits) {
    return query_host("rt_trace_rays_host", c, rays, n, 0u, false, hits);
}

// ---- the k nearest hits (rt_query.hip: multi_triangles, multi_spheres) ----

// The argument checks of both forms, in the header's order: flags, k, context, n == 0 (*done), pointers
static int multi_check(const char* who, rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint32_t k, const rt_hit* hits, bool device,
                       bool& done) {
    return rays_check(who, c, rays, n, flags, RT_QUERY_LIMITS, &k, hits, device ? "rays and hits" : nullptr, 16u, done);
}

static int multi_launch(rt_ctx* c, const float4* rays, uint32_t n, uint32_t flags, uint32_t k, float4* hits, const Query& q) {
    if (q.tri) RT_HIP(rt_launch_multi_triangles(q.ts, q.inst, rays, flags, k, hits, n, q.s));
    else RT_HIP(rt_launch_multi_spheres(c->d_records.as<float>(), c->n, rays, flags, k, hits, n, q.s));
    return RT_OK;
}

int rt_trace_rays_multi(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint32_t k, rt_hit* hits, void* hip_stream) {
    bool done;
    { int rc = multi_check("rt_trace_rays_multi", c, rays, n, flags, k, hits, true, done); if (rc != RT_OK || done) return rc; }
    return query_run(c, "rt_trace_rays_multi", hip_stream, [&](const Query& q) {
        return multi_launch(c, reinterpret_cast<const float4*>(rays), n, flags, k, reinterpret_cast<float4*>(hits), q);
    });
}

int rt_trace_rays_multi_host(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, uint32_t k, rt_hit* hits) {
    bool done;
    { int rc = multi_check("rt_trace_rays_multi_host", c, rays, n, flags, k, hits, false, done); if (rc != RT_OK || done) return rc; }
    Staged r[] = {{hits, &c->d_qhits, (size_t)n * 32u * k}};
    return query_run_host(c, "rt_trace_rays_multi_host", rays, &c->d_qrays, (size_t)n * 32u, r, [&](const Query& q) {
        return multi_launch(c, static_cast<const float4*>(c->d_qrays.p), n, flags, k, reinterpret_cast<float4*>(r[0].dev), q);
    });
}

int rt_pick(rt_ctx* c, const uint32_t* xy, uint32_t n, rt_hit* hits) {
    if (!c) return fail(RT_ERR_INVALID_ARG, "rt_pick: ctx is NULL");
    if (n == 0) return RT_OK;
    if (!xy || !hits) return fail(RT_ERR_INVALID_ARG, "rt_pick: NULL argument");
    if (!c->W || !c->H) return fail(RT_ERR_STATE, "rt_pick: rt_resize has not been called");
    if (!c->have_params) return fail(RT_ERR_STATE, "rt_pick: rt_write_params has not been called");
    for (uint32_t i = 0; i < n; ++i)          // full-frame coordinates, whatever the partition
        if (xy[2u * i] >= c->W || xy[2u * i + 1u] >= c->H) return fail(RT_ERR_INVALID_ARG, "rt_pick: pixel outside the frame");
    Staged r[] = {{hits, &c->d_qhits, (size_t)n * 32u}};
    return query_run_host(c, "rt_pick", xy, &c->d_qxy, (size_t)n * 8u, r, [&](const Query& q) {
        // the pixels' primary rays, made on the device into the ray queries' own staging buffer, then rt_trace_rays' kernel
        { int rc = grow_staging(c->d_qrays, (size_t)n * 32u); if (rc != RT_OK) return rc; }
        RtFrameArgs fa;
        camera_frame_args(c, c->W, c->H, fa);
        RT_HIP(rt_launch_pick_rays(fa, static_cast<const uint32_t*>(c->d_qxy.p), static_cast<float4*>(c->d_qrays.p), n, q.s));
        return query_launch(c, static_cast<const float4*>(c->d_qrays.p), r[0].dev, n, q);
    });
}

// ---- closest-point queries (rt_closest.hip) --------------------------------------------------------------------------------------

static_assert(sizeof(rt_closest) == 32, "rt_closest is two float4");

extern "C++" { RtClosestLaunch rt_closest_launch = nullptr; }      // set by rt_closest.o (rt_tri_types.h)

// The checks of both forms, in the header's order: the context, n == 0 (*done), the buffers (device: 16-byte aligned), the scene
// written, a triangle scene
static int closest_check(const char* who, rt_ctx* c, const float* points, uint32_t n, const rt_closest* out, bool device, bool& done) {
    char msg[160];
    done = false;
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (n == 0) { done = true; return RT_OK; }
    if (!points || !out) { std::snprintf(msg, sizeof msg, "%s: NULL argument", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && (reinterpret_cast<uintptr_t>(points) % 16u || reinterpret_cast<uintptr_t>(out) % 16u)) {
        std::snprintf(msg, sizeof msg, "%s: points and out must be 16-byte aligned", who);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    { int rc = query_scene_written(c, who); if (rc != RT_OK) return rc; }
    if (c->scene_kind != 1) {
        std::snprintf(msg, sizeof msg, "%s: sphere scenes have no closest-point query (a sphere's distance needs a square root)", who);
        return fail(RT_ERR_UNSUPPORTED, msg);
    }
    return RT_OK;
}

// the per-instance constants (remade by every call, on its stream: queries run in call order), then the search
static int closest_launch(rt_ctx* c, const float4* points, float4* out, uint32_t n, const Query& q) {
    const size_t need = (size_t)q.ts.n_blas * kCpInstWords * 4u;
    if (need > c->d_closest.cap) {
        if (c->query_pending) RT_HIP(hipEventSynchronize(c->ev_query));      // an earlier call may still read the old one
        RT_HIP(c->d_closest.replace(std::max(need, (size_t)4096u)));
    }
    if (!rt_closest_launch) return fail(RT_ERR_UNSUPPORTED, "rt_closest_points: this build holds no closest-point kernels (rt_closest.o is not linked)");
    RT_HIP(rt_closest_launch(q.ts, q.inst, c->d_closest.as<float>(), points, out, n, q.s));
    return RT_OK;
}

int rt_closest_points(rt_ctx* c, const float* points, uint32_t n, rt_closest* out, void* hip_stream) {
    bool done;
    { int rc = closest_check("rt_closest_points", c, points, n, out, true, done); if (rc != RT_OK || done) return rc; }
    return query_run(c, "rt_closest_points", hip_stream, [&](const Query& q) {
        return closest_launch(c, reinterpret_cast<const float4*>(points), reinterpret_cast<float4*>(out), n, q);
    });
}

int rt_closest_points_host(rt_ctx* c, const float* points, uint32_t n, rt_closest* out) {
    bool done;
    { int rc = closest_check("rt_closest_points_host", c, points, n, out, false, done); if (rc != RT_OK || done) return rc; }
    Staged r[] = {{out, &c->d_qhits, (size_t)n * 32u}};
    return query_run_host(c, "rt_closest_points_host", points, &c->d_qrays, (size_t)n * 16u, r, [&](const Query& q) {
        return closest_launch(c, static_cast<const float4*>(c->d_qrays.p), reinterpret_cast<float4*>(r[0].dev), n, q);
    });
}

int rt_closest_points_model(const float* points, uint32_t n, const float* triangles, uint32_t n_triangles, const float* tri_lookup,
                            uint32_t n_tri_lookup, const float* nodes, uint32_t n_nodes, const float* blas, uint32_t n_blas,
                            const float* blas_lookup, uint32_t n_blas_lookup, const uint32_t* masks, uint32_t n_masks, uint32_t ray_mask,
                            rt_closest* out, uint64_t* tests) {
    const char* why = "";
    const int rc = rt_cp_model(points, n, triangles, n_triangles, tri_lookup, n_tri_lookup, nodes, n_nodes, blas, n_blas, blas_lookup,
                               n_blas_lookup, masks, n_masks, ray_mask, out, tests, &why);
    if (rc != RT_OK) { char msg[200]; std::snprintf(msg, sizeof msg, "rt_closest_points_model: %s", why); return fail(rc, msg); }
    return RT_OK;
}

// ---- shaded ray queries (rt_shade.hip) -----------------------------------------------------------------------------------------

static_assert(sizeof(rt_shade) == 16, "rt_shade is one float4");

// The state a shade query reads beside the scene -- the parameters and the sky -- and the mesh texture a frame would default
static int shade_state(const char* who, rt_ctx* c) {
    char msg[160];
    if (!c->have_params) { std::snprintf(msg, sizeof msg, "%s: rt_write_params has not been called", who); return fail(RT_ERR_STATE, msg); }
    for (int i = 0; i < 6; ++i)
        if (!c->d_face[i].p) { std::snprintf(msg, sizeof msg, "%s: all six cube map faces must be written first", who); return fail(RT_ERR_STATE, msg); }
    if (c->scene_kind == 1 && c->d_tri.used && !c->d_tex.used) {   // meshTex is mandatory in the reference (RR:113-114); default: 1x1 white
        const uint8_t white[4] = {255, 255, 255, 255};
        int rc = rt_write_mesh_texture(c, 1, 1, white);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

// The argument checks of both forms, in query_device's order: flags, context, n == 0 (*done), pointers; then shade_state.
static int shade_check(const char* who, rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, const rt_shade* out, bool device, bool& done) {
    { int rc = rays_check(who, c, rays, n, flags, RT_SHADE_COMPOSE, nullptr, out, device ? "rays and out" : nullptr, 16u, done);
      if (rc != RT_OK || done) return rc; }
    return shade_state(who, c);
}

// A shade kernel's arguments for a target of W x H: parameters, cube faces and sky flags as rt_enqueue assembles them for a frame,
// by value -- no slot of the event ring, no counters, no field of the stats.
static void shade_frame_args(const rt_ctx* c, uint32_t W, uint32_t H, RtFrameArgs& fa) {
    camera_frame_args(c, W, H, fa);
    for (int i = 0; i < 6; ++i) { fa.face[i] = c->d_face[i].as<uint8_t>(); fa.fw[i] = c->fw[i]; fa.fh[i] = c->fh[i]; }
    sky_flags(c, fa.sky_flat, fa.sky_seamless);
}
// The shade kernel on q.s behind query_prepare (rays have no frame: W = H = 0)
static int shade_launch(rt_ctx* c, const float4* rays, uint32_t n, uint32_t flags, float4* out, const Query& q) {
    RtFrameArgs fa;
    shade_frame_args(c, 0u, 0u, fa);
    if (q.tri) RT_HIP(rt_launch_shade_triangles(fa, q.ts, q.inst, rays, flags, out, n, q.s));
    else RT_HIP(rt_launch_shade_spheres(fa, c->d_records.as<float>(), c->n, rays, flags, out, n, q.s));
    return RT_OK;
}

int rt_shade_rays(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, rt_shade* out, void* hip_stream) {
    bool done;
    { int rc = shade_check("rt_shade_rays", c, rays, n, flags, out, true, done); if (rc != RT_OK || done) return rc; }
    return query_run(c, "rt_shade_rays", hip_stream, [&](const Query& q) {
        return shade_launch(c, reinterpret_cast<const float4*>(rays), n, flags, reinterpret_cast<float4*>(out), q);
    });
}

int rt_shade_rays_host(rt_ctx* c, const float* rays, uint32_t n, uint32_t flags, rt_shade* out) {
    bool done;
    { int rc = shade_check("rt_shade_rays_host", c, rays, n, flags, out, false, done); if (rc != RT_OK || done) return rc; }
    Staged r[] = {{out, &c->d_qhits, (size_t)n * sizeof(rt_shade)}};
    return query_run_host(c, "rt_shade_rays_host", rays, &c->d_qrays, (size_t)n * 32u, r, [&](const Query& q) {
        return shade_launch(c, static_cast<const float4*>(c->d_qrays.p), n, flags, reinterpret_cast<float4*>(r[0].dev), q);
    });
}

// ---- supersampled frames (rt_sample.hip) ---------------------------------------------------------------------------------------

// The checks of both forms, in the header's order: s, context, outputs; the state (rt_resize, a scene, shade_state); capacities
static int sample_check(const char* who, rt_ctx* c, uint32_t s, const uint8_t* rgba8, size_t cap8, const float* rgbaf, size_t capf, bool device) {
    char msg[160];
    if (s == 0u || s > RT355_MAX_SUPERSAMPLE) {
        std::snprintf(msg, sizeof msg, "%s: s = %u is outside 1 .. RT355_MAX_SUPERSAMPLE (%u)", who, s, RT355_MAX_SUPERSAMPLE);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!rgba8 && !rgbaf) { std::snprintf(msg, sizeof msg, "%s: both outputs are NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && (reinterpret_cast<uintptr_t>(rgba8) % 4u || reinterpret_cast<uintptr_t>(rgbaf) % 16u)) {
        std::snprintf(msg, sizeof msg, "%s: rgba8 must be 4-byte and rgbaf 16-byte aligned", who);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    if (!c->W || !c->H) { std::snprintf(msg, sizeof msg, "%s: rt_resize has not been called", who); return fail(RT_ERR_STATE, msg); }
    { int rc = query_scene_written(c, who); if (rc != RT_OK) return rc; }
    { int rc = shade_state(who, c); if (rc != RT_OK) return rc; }
    const size_t px = (size_t)c->W * c->H;
    if ((rgba8 && cap8 < px * 4u) || (rgbaf && capf < px * 16u)) {
        std::snprintf(msg, sizeof msg, "%s: a %u x %u frame needs %zu bytes of rgba8 and %zu of rgbaf", who, c->W, c->H, px * 4u, px * 16u);
        return fail(RT_ERR_CAPACITY, msg);
    }
    return RT_OK;
}

// The sample kernel on q.s behind query_prepare: shade_launch's arguments with the camera of the last rt_write_params and the
// target the samples are pixels of, s W x s H -- the whole frame, whatever the partition
static int sample_launch(rt_ctx* c, uint32_t ss, uint8_t* rgba8, float* rgbaf, const Query& q) {
    RtFrameArgs fa;
    shade_frame_args(c, ss * c->W, ss * c->H, fa);
    const RtSampleOut o = {c->W, c->H, ss, reinterpret_cast<uint32_t*>(rgba8), reinterpret_cast<float4*>(rgbaf)};
    if (q.tri) RT_HIP(rt_launch_sample_triangles(fa, q.ts, q.inst, o, q.s));
    else RT_HIP(rt_launch_sample_spheres(fa, c->d_records.as<float>(), c->n, o, q.s));
    return RT_OK;
}

int rt_render_samples(rt_ctx* c, uint32_t ss, uint8_t* rgba8, size_t cap8, float* rgbaf, size_t capf, void* hip_stream) {
    { int rc = sample_check("rt_render_samples", c, ss, rgba8, cap8, rgbaf, capf, true); if (rc != RT_OK) return rc; }
    return query_run(c, "rt_render_samples", hip_stream, [&](const Query& q) { return sample_launch(c, ss, rgba8, rgbaf, q); });
}

int rt_render_samples_host(rt_ctx* c, uint32_t ss, uint8_t* rgba8, size_t cap8, float* rgbaf, size_t capf) {
    { int rc = sample_check("rt_render_samples_host", c, ss, rgba8, cap8, rgbaf, capf, false); if (rc != RT_OK) return rc; }
    // (the staging buffers of the ray queries, idle between calls: the bytes where their rays go, the floats where their results go)
    const size_t px = (size_t)c->W * c->H;
    Staged r[] = {{rgba8, &c->d_qrays, px * 4u}, {rgbaf, &c->d_qhits, px * 16u}};
    return query_run_host(c, "rt_render_samples_host", nullptr, nullptr, 0u, r, [&](const Query& q) {
        return sample_launch(c, ss, r[0].dev, reinterpret_cast<float*>(r[1].dev), q);
    });
}

// ---- the frame-shaped queries: geometry frames (rt_gbuffer.hip) and ambient-occlusion frames (rt_ao.hip) --------------------------

// What both check after their own arguments, in the header's order: the state (rt_resize, a scene, rt_write_params), the rectangle
// (NULL: the whole frame), the capacity.  o.{x0, y0, w, h}: the rectangle the call means; o.{W, H}: the frame it lies in.
extern "C++" {
template <typename OUT>
static int frame_query_check(const char* who, rt_ctx* c, const uint32_t* rect, size_t cap_pixels, OUT& o) {
    char msg[200];
    if (!c->W || !c->H) { std::snprintf(msg, sizeof msg, "%s: rt_resize has not been called", who); return fail(RT_ERR_STATE, msg); }
    { int rc = query_scene_written(c, who); if (rc != RT_OK) return rc; }
    if (!c->have_params) { std::snprintf(msg, sizeof msg, "%s: rt_write_params has not been called", who); return fail(RT_ERR_STATE, msg); }
    const uint32_t x0 = rect ? rect[0] : 0u, y0 = rect ? rect[1] : 0u, w = rect ? rect[2] : c->W, h = rect ? rect[3] : c->H;
    if (!w || !h || (uint64_t)x0 + w > c->W || (uint64_t)y0 + h > c->H) {   // full-frame coordinates, whatever the partition
        std::snprintf(msg, sizeof msg, "%s: the rectangle {%u, %u, %u, %u} is empty or not inside the %u x %u frame", who, x0, y0, w, h, c->W, c->H);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    if (cap_pixels < (size_t)w * h) {
        std::snprintf(msg, sizeof msg, "%s: a %u x %u rectangle needs room for %zu pixels in every plane", who, w, h, (size_t)w * h);
        return fail(RT_ERR_CAPACITY, msg);
    }
    o.x0 = x0; o.y0 = y0; o.w = w; o.h = h;
    o.W = c->W; o.H = c->H;
    return RT_OK;
}
}  // extern "C++"

static_assert(sizeof(rt_gbuffer) == 32, "rt_gbuffer is four pointers");

// The checks of both forms, in the header's order: context, `out`, planes; the state (rt_resize, a scene, rt_write_params); the
// rectangle; the capacity.  o: the planes as given and the rectangle the call means.
static int gbuffer_check(const char* who, rt_ctx* c, const uint32_t* rect, const rt_gbuffer* out, size_t cap_pixels, bool device, RtGbufferOut& o) {
    char msg[200];
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!out) { std::snprintf(msg, sizeof msg, "%s: out is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!out->depth && !out->normal && !out->ids && !out->uv) { std::snprintf(msg, sizeof msg, "%s: all four planes are NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && (reinterpret_cast<uintptr_t>(out->depth) % 4u || reinterpret_cast<uintptr_t>(out->normal) % 16u ||
                   reinterpret_cast<uintptr_t>(out->ids) % 8u || reinterpret_cast<uintptr_t>(out->uv) % 8u)) {
        std::snprintf(msg, sizeof msg, "%s: depth must be 4-byte, ids and uv 8-byte and normal 16-byte aligned", who);
        return fail(RT_ERR_INVALID_ARG, msg);
    }
    o.depth = out->depth;
    o.normal = reinterpret_cast<float4*>(out->normal);
    o.ids = reinterpret_cast<int2*>(out->ids);
    o.uv = reinterpret_cast<float2*>(out->uv);
    return frame_query_check(who, c, rect, cap_pixels, o);
}

// The geometry kernel on q.s behind query_prepare: the camera of the last rt_write_params, by value in the kernel's arguments, and
// the whole frame's size, whatever the partition -- rt_pick's ray, made in the lane
static int gbuffer_launch(rt_ctx* c, const RtGbufferOut& o, const Query& q) {
    RtFrameArgs fa;
    camera_frame_args(c, c->W, c->H, fa);
    if (q.tri) RT_HIP(rt_launch_gbuffer_triangles(fa, q.ts, q.inst, o, q.s));
    else RT_HIP(rt_launch_gbuffer_spheres(fa, c->d_records.as<float>(), c->n, o, q.s));
    return RT_OK;
}

int rt_render_gbuffer(rt_ctx* c, const uint32_t* rect, const rt_gbuffer* out, size_t cap_pixels, void* hip_stream) {
    RtGbufferOut o;
    { int rc = gbuffer_check("rt_render_gbuffer", c, rect, out, cap_pixels, true, o); if (rc != RT_OK) return rc; }
    return query_run(c, "rt_render_gbuffer", hip_stream, [&](const Query& q) { return gbuffer_launch(c, o, q); });
}

int rt_render_gbuffer_host(rt_ctx* c, const uint32_t* rect, const rt_gbuffer* out, size_t cap_pixels) {
    RtGbufferOut o;
    { int rc = gbuffer_check("rt_render_gbuffer_host", c, rect, out, cap_pixels, false, o); if (rc != RT_OK) return rc; }
    // (one staging buffer of the ray queries, idle between calls, holds the planes asked for one after the other, the widest
    // first: every plane then starts on a multiple of its own alignment)
    const size_t px = (size_t)o.w * o.h;
    Staged r[] = {{out->normal, &c->d_qhits, px * 16u}, {out->ids, &c->d_qhits, px * 8u}, {out->uv, &c->d_qhits, px * 8u}, {out->depth, &c->d_qhits, px * 4u}};
    return query_run_host(c, "rt_render_gbuffer_host", nullptr, nullptr, 0u, r, [&](const Query& q) {
        RtGbufferOut d = o;
        d.normal = reinterpret_cast<float4*>(r[0].dev);
        d.ids = reinterpret_cast<int2*>(r[1].dev);
        d.uv = reinterpret_cast<float2*>(r[2].dev);
        d.depth = reinterpret_cast<float*>(r[3].dev);
        return gbuffer_launch(c, d, q);
    });
}

static_assert(sizeof(rt_ao) == 16, "rt_ao is two pointers");

// The checks of both forms, in the header's order: k; context, `dirs`, `out`, planes; the state; the rectangle; the capacity.
// o: the planes as given, the rectangle the call means, and the directions and limits -- copied here, at the call.
static int ao_check(const char* who, rt_ctx* c, const uint32_t* rect, const float* dirs, uint32_t k, float tmin, float radius, const rt_ao* out,
                    size_t cap_pixels, bool device, RtAoOut& o) {
    char msg[200];
    if (k == 0u || k > RT355_MAX_AO_RAYS) { std::snprintf(msg, sizeof msg, "%s: k = %u is not in 1 .. %u", who, k, RT355_MAX_AO_RAYS); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!c) { std::snprintf(msg, sizeof msg, "%s: ctx is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!dirs) { std::snprintf(msg, sizeof msg, "%s: dirs is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!out) { std::snprintf(msg, sizeof msg, "%s: out is NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (!out->count && !out->ao) { std::snprintf(msg, sizeof msg, "%s: both planes are NULL", who); return fail(RT_ERR_INVALID_ARG, msg); }
    if (device && reinterpret_cast<uintptr_t>(out->ao) % 4u) { std::snprintf(msg, sizeof msg, "%s: ao must be 4-byte aligned", who); return fail(RT_ERR_INVALID_ARG, msg); }
    std::memset(&o, 0, sizeof o);
    o.count = out->count;
    o.ao = out->ao;
    o.k = k; o.tmin = tmin; o.radius = radius;
    std::memcpy(o.dirs, dirs, (size_t)k * 3u * sizeof(float));
    return frame_query_check(who, c, rect, cap_pixels, o);
}

// The occlusion kernel on q.s behind query_prepare, with gbuffer_launch's camera
static int ao_launch(rt_ctx* c, const RtAoOut& o, const Query& q) {
    RtFrameArgs fa;
    camera_frame_args(c, c->W, c->H, fa);
    if (q.tri) RT_HIP(rt_launch_ao_triangles(fa, q.ts, q.inst, o, q.s));
    else RT_HIP(rt_launch_ao_spheres(fa, c->d_records.as<float>(), c->n, o, q.s));
    return RT_OK;
}

int rt_render_ao(rt_ctx* c, const uint32_t* rect, const float* dirs, uint32_t k, float tmin, float radius, const rt_ao* out, size_t cap_pixels, void* hip_stream) {
    RtAoOut o;
    { int rc = ao_check("rt_render_ao", c, rect, dirs, k, tmin, radius, out, cap_pixels, true, o); if (rc != RT_OK) return rc; }
    return query_run(c, "rt_render_ao", hip_stream, [&](const Query& q) { return ao_launch(c, o, q); });
}

int rt_render_ao_host(rt_ctx* c, const uint32_t* rect, const float* dirs, uint32_t k, float tmin, float radius, const rt_ao* out, size_t cap_pixels) {
    RtAoOut o;
    { int rc = ao_check("rt_render_ao_host", c, rect, dirs, k, tmin, radius, out, cap_pixels, false, o); if (rc != RT_OK) return rc; }
    // (one staging buffer of the ray queries, idle between calls: the float plane first, so that it starts aligned)
    const size_t px = (size_t)o.w * o.h;
    Staged r[] = {{out->ao, &c->d_qhits, px * 4u}, {out->count, &c->d_qhits, px}};
    return query_run_host(c, "rt_render_ao_host", nullptr, nullptr, 0u, r, [&](const Query& q) {
        RtAoOut d = o;
        d.ao = reinterpret_cast<float*>(r[0].dev);
        d.count = r[1].dev;
        return ao_launch(c, d, q);
    });
}

int rt_device_pixels(rt_ctx* c, void** out_ptr, size_t* out_bytes) {
    if (!c || !out_ptr || !out_bytes) return fail(RT_ERR_INVALID_ARG, "rt_device_pixels: NULL argument");
    if (!c->d_out) return fail(RT_ERR_STATE, "rt_device_pixels: no colour buffer (rt_resize first)");
    *out_ptr = c->d_out;
    *out_bytes = c->out_bytes;
    return RT_OK;
}

}  // extern "C"
