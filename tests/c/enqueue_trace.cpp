// enqueue_trace.cpp -- the sequence of HIP calls and kernel launches that rt_api.hip makes for a frame, without a GPU.
// rt_api.hip holds no device code: compiled --cuda-host-only it links against this file alone, which defines every HIP entry
// point and every rt_launch_* function the object leaves undefined (a launch added later fails the link) and prints one line
// per call.  Memory is calloc's, copies and memsets happen; streams, events and allocations are named by creation order
// (s3, e17, b9), a device pointer prints as bK+offset, a host pointer as `host`.  main() drives the C ABI through every branch of
// rt_enqueue, rt_render, rt_render_to and rt_wait (DESIGN.md 4.7g has the table) and prints a `#` line after every call: the
// call, its status, the message of a failure, and the state the step is about.  tests/test_enqueue_trace_cpu.py holds the output
// against tests/golden/enqueue_trace.txt.gz, recorded from the sources before rt_enqueue was taken apart.
// usage: enqueue_trace <dir with triangles.bin nodes.bin blas.bin tri_lookup.bin blas_lookup.bin (float32, tri_buffers' arrays)>
#include "../../compute_raytracer_amd/csrc/rt_ctx.h"
#include "../../compute_raytracer_amd/csrc/rt_build.h"
#include "../../compute_raytracer_amd/csrc/rt_refit.h"

#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// ---- names ---------------------------------------------------------------------------------------------------------------
namespace {

struct Handle { int id; };
int g_streams = 0, g_events = 0, g_bufs = 0;
std::map<const char*, std::pair<int, size_t>> g_live;       // base -> (name, bytes) of the live allocations

std::string S(hipStream_t s) { return s ? "s" + std::to_string(reinterpret_cast<Handle*>(s)->id) : std::string("s-"); }
std::string E(hipEvent_t e) { return e ? "e" + std::to_string(reinterpret_cast<Handle*>(e)->id) : std::string("e-"); }
std::string P(const void* p) {
    if (!p) return "null";
    const char* q = static_cast<const char*>(p);
    auto it = g_live.upper_bound(q);
    if (it != g_live.begin()) {
        --it;
        if (q < it->first + it->second.second) return "b" + std::to_string(it->second.first) + "+" + std::to_string(q - it->first);
    }
    return "host";
}
hipError_t alloc(const char* what, void** ptr, size_t bytes, unsigned flags) {
    char* p = static_cast<char*>(calloc(bytes ? bytes : 1, 1));
    if (!p) abort();
    g_live[p] = {g_bufs, bytes};
    std::printf("%s b%d %zu flags=%u\n", what, g_bufs++, bytes, flags);
    *ptr = p;
    return hipSuccess;
}
hipError_t release(const char* what, void* ptr) {
    std::printf("%s %s\n", what, P(ptr).c_str());
    if (ptr) { g_live.erase(static_cast<const char*>(ptr)); free(ptr); }
    return hipSuccess;
}

// what the driver sets for the functions that are not launches
bool g_fits = true;
int g_form = 1;

}  // namespace

// ---- the HIP entry points rt_api.hip calls ---------------------------------------------------------------------------------
extern "C" {
hipError_t hipSetDevice(int d) { std::printf("hipSetDevice %d\n", d); return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; std::printf("hipGetDeviceCount\n"); return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int d) {        // (the header maps the name to the entry point of this ABI)
    std::memset(p, 0, sizeof *p);
    std::strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = 256;
    std::printf("hipGetDeviceProperties %d\n", d);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stand-in"; }
hipError_t hipGetLastError(void) { std::printf("hipGetLastError\n"); return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) { return alloc("hipMalloc", p, bytes, 0u); }
hipError_t hipFree(void* p) { return release("hipFree", p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) { return alloc("hipHostMalloc", p, bytes, flags); }
hipError_t hipHostFree(void* p) { return release("hipHostFree", p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    *e = reinterpret_cast<hipEvent_t>(new Handle{g_events});
    std::printf("hipEventCreateWithFlags e%d flags=%u\n", g_events++, flags);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { std::printf("hipEventDestroy %s\n", E(e).c_str()); delete reinterpret_cast<Handle*>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { std::printf("hipEventRecord %s %s\n", E(e).c_str(), S(s).c_str()); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { std::printf("hipEventSynchronize %s\n", E(e).c_str()); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { *ms = 0.0f; std::printf("hipEventElapsedTime %s %s\n", E(a).c_str(), E(b).c_str()); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    *s = reinterpret_cast<hipStream_t>(new Handle{g_streams});
    std::printf("hipStreamCreateWithFlags s%d flags=%u\n", g_streams++, flags);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { std::printf("hipStreamDestroy %s\n", S(s).c_str()); delete reinterpret_cast<Handle*>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { std::printf("hipStreamSynchronize %s\n", S(s).c_str()); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) { std::printf("hipStreamWaitEvent %s %s flags=%u\n", S(s).c_str(), E(e).c_str(), flags); return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    std::printf("hipMemcpy %s <- %s %zu kind=%d\n", P(dst).c_str(), P(src).c_str(), bytes, (int)kind);
    std::memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    std::printf("hipMemcpyAsync %s <- %s %zu kind=%d %s\n", P(dst).c_str(), P(src).c_str(), bytes, (int)kind, S(s).c_str());
    std::memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t bytes) {
    std::printf("hipMemset %s %d %zu\n", P(dst).c_str(), v, bytes);
    std::memset(dst, v, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t s) {
    std::printf("hipMemsetAsync %s %d %zu %s\n", P(dst).c_str(), v, bytes, S(s).c_str());
    std::memset(dst, v, bytes);
    return hipSuccess;
}
}  // extern "C"

// ---- the launches: one line each, with the fields that show the plan --------------------------------------------------------
static void frame_fields(const RtFrameArgs& a) {
    std::printf(" N=%u N16=%u W=%u H=%u share=%u bvh_nodes=%u bvh_rec=%s queue=%s queue_cap=%u fin=%s sky_flat=%u sky_seamless=%u signed=%u"
                " tiles=%u/%u/%u out=%s rays=%s",
                a.N, a.N16, a.W, a.H, a.grid_share, a.bvh_nodes, P(a.bvh_rec).c_str(), P(a.queue).c_str(), a.queue_cap, P(a.fin).c_str(),
                a.sky_flat, a.sky_seamless, a.signed_filter, a.tile_first, a.tile_step, a.n_local_tiles, P(a.out).c_str(), P(a.rays).c_str());
}
hipError_t rt_launch_trace(const RtFrameArgs& a, const RtLaunchCfg& cfg, hipStream_t s) {
    std::printf("launch trace %s", S(s).c_str());
    frame_fields(a);
    std::printf(" cfg=%d/%d geo=%s cam_w=%s\n", cfg.mode, cfg.variant, P(a.geo).c_str(), P(a.cam_w).c_str());
    g_rt_kernel_id = cfg.mode == 1 ? RT_KID_LITERAL : (a.queue ? RT_KID_BRUTE_PIPELINE : RT_KID_BRUTE_SINGLE);
    return hipSuccess;
}
hipError_t rt_launch_bvh(const RtFrameArgs& a, hipStream_t s) {
    std::printf("launch bvh %s", S(s).c_str());
    frame_fields(a);
    std::printf(" geo_f=%s\n", P(a.geo_f).c_str());
    g_rt_kernel_id = RT_KID_HIERARCHY_8;
    return hipSuccess;
}
hipError_t rt_launch_triangles(const RtFrameArgs& a, const RtTriScene& t, int heatmap, hipStream_t s) {
    std::printf("launch triangles %s heatmap=%d", S(s).c_str(), heatmap);
    frame_fields(a);
    std::printf(" form=%u nodes=%s pairs=%s tile_order=%s tile_cost=%s dbg=%s roles=%u in_flight=%u p16_ok=%u packed_ok=%u tlas_small=%u n_blas=%u root_meta=",
                t.form, P(t.nodes).c_str(), P(t.pairs).c_str(), P(t.tile_order).c_str(), P(t.tile_cost).c_str(), P(t.dbg).c_str(), t.roles,
                t.in_flight, t.p16_ok, t.packed_ok, t.tlas_small, t.n_blas);
    for (uint32_t i = 0; i < t.n_blas && i < 16u; ++i) std::printf("%s%08x", i ? "," : "", t.root_meta[i]);
    std::printf("\n");
    g_rt_kernel_id = heatmap ? RT_KID_HEATMAP : ((t.tile_order && t.roles) ? RT_KID_TRIANGLES_ROLES : RT_KID_TRIANGLES);
    g_rt_tri_form = (int)t.form;
    return hipSuccess;
}
hipError_t rt_launch_prep(const RtPrepArgs& a, hipStream_t s) {
    std::printf("launch prep %s N=%u N16=%u records=%s geo=%s lgt=%s cam=%s col=%s geo_f=%s lgt_f=%s cam_f=%s geo_w=%s lgt_w=%s cam_w=%s\n", S(s).c_str(), a.N, a.N16,
                P(a.records).c_str(), P(a.geo).c_str(), P(a.lgt).c_str(), P(a.cam).c_str(), P(a.col).c_str(), P(a.geo_f).c_str(), P(a.lgt_f).c_str(),
                P(a.cam_f).c_str(), P(a.geo_w).c_str(), P(a.lgt_w).c_str(), P(a.cam_w).c_str());
    return hipSuccess;
}
hipError_t rt_launch_apply_instances(const RtInstanceArgs& a, hipStream_t s) {
    std::printf("launch apply_instances %s nodes=%s head_f=%u blas_f=%u lookup_f=%u\n", S(s).c_str(), P(a.nodes).c_str(), a.n_head_f, a.n_blas_f, a.n_lookup_f);
    return hipSuccess;
}
hipError_t rt_launch_frame_epilogue(unsigned long long* counters, unsigned long long* host, uint32_t words, hipStream_t s) {
    std::printf("launch frame_epilogue %s counters=%s host=%s words=%u\n", S(s).c_str(), P(counters).c_str(), P(host).c_str(), words);
    return hipSuccess;
}
hipError_t rt_launch_bvh_refit(float4* rec, const uint32_t* link, uint32_t n_nodes, const float* records, hipStream_t s) {
    std::printf("launch bvh_refit %s rec=%s link=%s nodes=%u records=%s\n", S(s).c_str(), P(rec).c_str(), P(link).c_str(), n_nodes, P(records).c_str());
    return hipSuccess;
}
hipError_t rt_launch_bvh_fill(float4* rec, const uint32_t* link, uint32_t n_nodes, const float4* geo_f, hipStream_t s) {
    std::printf("launch bvh_fill %s rec=%s link=%s nodes=%u geo_f=%s\n", S(s).c_str(), P(rec).c_str(), P(link).c_str(), n_nodes, P(geo_f).c_str());
    return hipSuccess;
}
hipError_t rt_launch_tri_corners(float4* out, const float* tri, const float* lookup, uint32_t n_slots, uint32_t n_tri, hipStream_t s) {
    std::printf("launch tri_corners %s out=%s tri=%s lookup=%s slots=%u tris=%u\n", S(s).c_str(), P(out).c_str(), P(tri).c_str(), P(lookup).c_str(), n_slots, n_tri);
    return hipSuccess;
}
hipError_t rt_launch_order_hist(uint32_t* cost, uint32_t* scan, uint32_t* order, uint32_t n_tiles, uint32_t wave_slots, unsigned long long* counters,
                                unsigned long long* host, uint32_t words, unsigned long long* split_out, hipStream_t s) {
    std::printf("launch order_hist %s cost=%s scan=%s order=%s tiles=%u wave_slots=%u counters=%s host=%s words=%u split=%s\n", S(s).c_str(), P(cost).c_str(),
                P(scan).c_str(), P(order).c_str(), n_tiles, wave_slots, P(counters).c_str(), P(host).c_str(), words, P(split_out).c_str());
    return hipSuccess;
}
hipError_t rt_launch_order_scatter(uint32_t* cost, uint32_t* scan, uint32_t* order, uint32_t n_tiles, hipStream_t s) {
    std::printf("launch order_scatter %s cost=%s scan=%s order=%s tiles=%u\n", S(s).c_str(), P(cost).c_str(), P(scan).c_str(), P(order).c_str(), n_tiles);
    return hipSuccess;
}
hipError_t rt_launch_query_triangles(const RtTriScene& t, int inst, const float4* rays, float4* hits, uint32_t n, hipStream_t s) {
    std::printf("launch query_triangles %s inst=%d nodes=%s pairs=%s rays=%s hits=%s n=%u\n", S(s).c_str(), inst, P(t.nodes).c_str(), P(t.pairs).c_str(),
                P(rays).c_str(), P(hits).c_str(), n);
    return hipSuccess;
}
// the launches of the entry points this program does not drive: referenced by the object, so defined; one line all the same
static hipError_t other(const char* name, hipStream_t s) { std::printf("launch %s %s\n", name, S(s).c_str()); return hipSuccess; }
hipError_t rt_launch_assemble(const uint8_t*, uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t s) { return other("assemble", s); }
hipError_t rt_launch_pick_rays(const RtFrameArgs&, const uint32_t*, float4*, uint32_t, hipStream_t s) { return other("pick_rays", s); }
hipError_t rt_launch_query_spheres(const float*, uint32_t, const float4*, float4*, uint32_t, hipStream_t s) { return other("query_spheres", s); }
hipError_t rt_launch_limited_triangles(const RtTriScene&, int, const float4*, uint32_t, bool, void*, uint32_t, hipStream_t s) { return other("limited_triangles", s); }
hipError_t rt_launch_limited_spheres(const float*, uint32_t, const float4*, uint32_t, bool, void*, uint32_t, hipStream_t s) { return other("limited_spheres", s); }
hipError_t rt_launch_multi_triangles(const RtTriScene&, int, const float4*, uint32_t, uint32_t, float4*, uint32_t, hipStream_t s) { return other("multi_triangles", s); }
hipError_t rt_launch_multi_spheres(const float*, uint32_t, const float4*, uint32_t, uint32_t, float4*, uint32_t, hipStream_t s) { return other("multi_spheres", s); }
hipError_t rt_launch_shade_triangles(const RtFrameArgs&, const RtTriScene&, int, const float4*, uint32_t, float4*, uint32_t, hipStream_t s) { return other("shade_triangles", s); }
hipError_t rt_launch_shade_spheres(const RtFrameArgs&, const float*, uint32_t, const float4*, uint32_t, float4*, uint32_t, hipStream_t s) { return other("shade_spheres", s); }
hipError_t rt_launch_sample_triangles(const RtFrameArgs&, const RtTriScene&, int, const RtSampleOut&, hipStream_t s) { return other("sample_triangles", s); }
hipError_t rt_launch_sample_spheres(const RtFrameArgs&, const float*, uint32_t, const RtSampleOut&, hipStream_t s) { return other("sample_spheres", s); }
hipError_t rt_launch_gbuffer_triangles(const RtFrameArgs&, const RtTriScene&, int, const RtGbufferOut&, hipStream_t s) { return other("gbuffer_triangles", s); }
hipError_t rt_launch_gbuffer_spheres(const RtFrameArgs&, const float*, uint32_t, const RtGbufferOut&, hipStream_t s) { return other("gbuffer_spheres", s); }
hipError_t rt_launch_ao_triangles(const RtFrameArgs&, const RtTriScene&, int, const RtAoOut&, hipStream_t s) { return other("ao_triangles", s); }
hipError_t rt_launch_ao_spheres(const RtFrameArgs&, const float*, uint32_t, const RtAoOut&, hipStream_t s) { return other("ao_spheres", s); }
hipError_t rt_launch_refit_nodes(const RtRefitArgs&, hipStream_t s) { return other("refit_nodes", s); }
hipError_t rt_launch_build_prep(const RtBuildArgs&, const rt_blas_range*, hipStream_t s) { return other("build_prep", s); }
hipError_t rt_launch_build_level(const RtBuildArgs&, uint32_t, uint32_t, uint32_t, hipStream_t s) { return other("build_level", s); }
hipError_t rt_launch_build_count_up(const RtBuildArgs&, uint32_t, uint32_t, hipStream_t s) { return other("build_count_up", s); }
hipError_t rt_launch_build_rank_down(const RtBuildArgs&, uint32_t, uint32_t, hipStream_t s) { return other("build_rank_down", s); }
hipError_t rt_launch_build_emit_nodes(const RtBuildArgs&, uint32_t, uint32_t, hipStream_t s) { return other("build_emit_nodes", s); }
hipError_t rt_launch_build_emit_lookup(const RtBuildArgs&, const rt_blas_range*, hipStream_t s) { return other("build_emit_lookup", s); }

// not launches: the driver sets their answers
bool rt_trace_fits(uint32_t, uint32_t, const RtLaunchCfg&, bool) { return g_fits; }
bool rt_trace_wants_queue(uint32_t n, const RtLaunchCfg& cfg) { return cfg.variant == 2 || cfg.variant == 3 || (cfg.variant == 0 && n >= 320u); }   // rt_kernels.hip's rule
int rt_tri_stack_form(const RtTriScene&, int) { return g_form; }
uint32_t rt_order_scan_words(void) { return 1024u; }
void rt_comm_release(rt_ctx*) {}
int rt_comm_after_wait(rt_ctx*) { return RT_OK; }
int rt_comm_wait_frames(rt_ctx*) { return RT_OK; }

// ---- the driver --------------------------------------------------------------------------------------------------------------
namespace {

rt_ctx* c = nullptr;

// the state a step is about, by group: r ring, f pair-record counters, v instance versions, o work lists, s stats
void state(const char* groups) {
    for (const char* g = groups; *g; ++g) {
        switch (*g) {
            case 'r': std::printf(" in_flight=%u stream_rot=%u hint=%d", c->in_flight, c->stream_rot, (int)c->pipelined_hint); break;
            case 'f': std::printf(" flow_streak=%u cooldown=%u since=%u flow_gen=%llu flow_ok=%d dirty=%d", c->flow_streak, c->flow_cooldown, c->flow_frames_since,
                                  (unsigned long long)c->flow_gen, (int)c->flow.ok, (int)c->flow_dirty); break;
            case 'v': std::printf(" inst_gen=%llu ver_gen=%llu,%llu,%llu,%llu carried=%llu", (unsigned long long)c->inst.gen, (unsigned long long)c->ver_gen[0],
                                  (unsigned long long)c->ver_gen[1], (unsigned long long)c->ver_gen[2], (unsigned long long)c->ver_gen[3],
                                  (unsigned long long)c->inst_gen_carried); break;
            case 'o': std::printf(" order_tiles=%u,%u,%u,%u", c->order_tiles[0], c->order_tiles[1], c->order_tiles[2], c->order_tiles[3]); break;
            case 's': std::printf(" kernel_id=%u tri_form=%u grid_share=%u instance_uploads=%u pair_rebuilds=%u frames=%u batch_frames=%u", c->stats.kernel_id,
                                  c->stats.tri_form, c->stats.grid_share, c->stats.instance_uploads, c->stats.pair_rebuilds, c->stats.frames, c->stats.batch_frames); break;
        }
    }
}
int said(const char* call, int rc, const char* groups) {
    std::printf("# %s -> %d", call, rc);
    if (rc != RT_OK) std::printf(" \"%s\"", rt_last_error(c));
    if (c) state(groups);
    std::printf("\n");
    return rc;
}
#define CALL(groups, expr) said(#expr, (expr), groups)
#define OK(groups, expr) do { if (CALL(groups, expr) != RT_OK) { std::printf("# unexpected failure\n"); return 1; } } while (0)
void step(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::printf("## ");
    std::vprintf(fmt, ap);
    std::printf("\n");
    va_end(ap);
}

std::vector<float> read_floats(const std::string& path) {
    std::vector<float> v;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        v.resize((size_t)n / 4u);
        if (std::fread(v.data(), 4, v.size(), f) != v.size()) v.clear();
        std::fclose(f);
    }
    return v;
}

// n spheres on a lattice inside [-8, 8]^3, radii 0.1 .. 0.4; `far`: the first one 2^21 away (beyond the filter's range)
std::vector<float> spheres(uint32_t n, bool far = false) {
    std::vector<float> r(8u * (size_t)n, 0.0f);
    uint32_t x = 12345u;
    for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 8; ++k) {
            x = x * 1664525u + 1013904223u;
            r[8u * i + k] = (float)(x >> 8) / 16777216.0f;
        }
        for (int k = 0; k < 3; ++k) r[8u * i + k] = r[8u * i + k] * 16.0f - 8.0f;
        r[8u * i + 7] = 0.1f + 0.3f * r[8u * i + 7];
    }
    if (far && n) r[0] = 2097152.0f;
    return r;
}
int write_spheres(uint32_t n, bool far = false) {
    // the same count as the device topology's would start the worker thread, whose finish races the next frame: not in this trace
    if (n == c->bvh_topo_n) { std::printf("# driver error: %u spheres twice\n", n); std::exit(1); }
    const std::vector<float> r = spheres(n, far);
    return rt_write_spheres(c, r.data(), n);
}
void params(float* p, float cam_x) {
    std::memset(p, 0, 24 * sizeof(float));
    p[0] = cam_x; p[1] = 2.0f; p[2] = 12.0f;
    p[4] = 0.0f; p[5] = 0.0f; p[6] = -1.0f;
    p[8] = 1.0f; p[13] = 1.0f;
    p[16] = 0.0f; p[17] = 5.0f; p[18] = 6.0f;
    p[20] = 4.0f;
}
int write_params(float cam_x) {
    float p[24];
    params(p, cam_x);
    return rt_write_params(c, p);
}
int write_sky(uint32_t w, int faces = 6) {
    std::vector<uint8_t> px((size_t)w * w * 4u, 200);
    int rc = RT_OK;
    for (int f = 0; f < faces && rc == RT_OK; ++f) rc = rt_write_cubemap_face(c, f, w, w, px.data());
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: enqueue_trace <scene dir>\n"); return 2; }
    const std::string dir = argv[1];
    const std::vector<float> tris = read_floats(dir + "/triangles.bin"), nodes = read_floats(dir + "/nodes.bin"), blas = read_floats(dir + "/blas.bin"),
                             tri_lookup = read_floats(dir + "/tri_lookup.bin"), blas_lookup = read_floats(dir + "/blas_lookup.bin");
    if (tris.empty() || nodes.empty() || blas.empty() || tri_lookup.empty() || blas_lookup.empty()) { std::fprintf(stderr, "scene files missing\n"); return 2; }
    const uint32_t n_tris = (uint32_t)(tris.size() / 40u), n_nodes = (uint32_t)(nodes.size() / 8u), n_blas = (uint32_t)(blas.size() / 20u);

    step("create");
    OK("", rt_create(0, &c));

    step("1. state errors, in the order rt_enqueue checks them");
    CALL("", rt_render(nullptr)); CALL("", rt_wait(nullptr)); CALL("rs", rt_wait(c));                    // nothing in flight
    CALL("rs", rt_render(c)); OK("", rt_resize(c, 64, 40)); CALL("rs", rt_render(c)); OK("", write_params(0.0f)); CALL("rs", rt_render(c));
    OK("", write_spheres(8)); OK("", write_sky(1, 5)); OK("", rt_select_kernel(c, RT_KERNEL_HEATMAP));
    CALL("rs", rt_render(c));                 // the heatmap over spheres is refused before the faces are looked at
    OK("", rt_select_kernel(c, RT_KERNEL_RAYTRACER)); CALL("rs", rt_render(c)); OK("", write_sky(1));
    step("1. a triangle scene missing each of its five buffers, then without a texture");
    const uint32_t n_tri_lookup = (uint32_t)tri_lookup.size(), n_blas_lookup = (uint32_t)blas_lookup.size();
    OK("", rt_write_triangles(c, tris.data(), n_tris)); OK("", rt_write_blas(c, blas.data(), n_blas));
    OK("", rt_write_tri_lookup(c, tri_lookup.data(), n_tri_lookup)); OK("", rt_write_blas_lookup(c, blas_lookup.data(), n_blas_lookup));
    CALL("rs", rt_render(c)); OK("", rt_write_nodes(c, 0, nodes.data(), n_nodes)); OK("", rt_write_triangles(c, tris.data(), 0));
    CALL("rs", rt_render(c)); OK("", rt_write_triangles(c, tris.data(), n_tris)); OK("", rt_write_blas(c, blas.data(), 0)); CALL("rs", rt_render(c));
    OK("", rt_write_blas(c, blas.data(), n_blas)); OK("", rt_write_tri_lookup(c, tri_lookup.data(), 0)); CALL("rs", rt_render(c));
    OK("", rt_write_tri_lookup(c, tri_lookup.data(), n_tri_lookup)); OK("", rt_write_blas_lookup(c, blas_lookup.data(), 0)); CALL("rs", rt_render(c));
    OK("", rt_write_blas_lookup(c, blas_lookup.data(), n_blas_lookup));
    g_form = 1;
    OK("rsfv", rt_render(c));                 // writes the 1x1 white texture, then renders
    OK("rs", rt_wait(c));

    step("2. spheres, 64x40, n = 8, variant 0: awaited frames");
    OK("", write_spheres(8));
    for (int i = 0; i < 2; ++i) { OK("rs", rt_render(c)); OK("rs", rt_wait(c)); }
    step("2. three in flight, rt_wait sets the hint; three in flight again");
    for (int i = 0; i < 3; ++i) OK("rs", rt_render(c));
    OK("rs", rt_wait(c));
    for (int i = 0; i < 3; ++i) OK("rs", rt_render(c));
    c->h_rays.as<unsigned long long>()[2u * 1u + 1u] = 1ull;
    std::printf("# driver: the fault word of the frame in slot 1 = 1\n");
    CALL("rs", rt_wait(c));                   // the batch is complete all the same; the status and the message say what happened
    c->h_rays.as<unsigned long long>()[2u * 1u + 1u] = 0ull;
    step("2. an awaited frame after it, and one more (the hint is gone); rt_write_params between frames");
    for (int i = 0; i < 2; ++i) { OK("rs", rt_render(c)); OK("rs", rt_wait(c)); }
    OK("", write_params(1.0f)); OK("rs", rt_render(c)); OK("", write_params(2.0f)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));

    step("3. n = 200: host build, both uploads, fill; frames in flight (the hint is set: from 72 on)");
    OK("", write_spheres(200)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    OK("", write_params(3.0f));               // the hierarchy kernel needs no prep for new parameters
    for (int i = 0; i < 3; ++i) OK("rs", rt_render(c));
    OK("rs", rt_wait(c));
    step("3. 100 spheres with and without the hint: hierarchy from 72 on, brute force below 128");
    OK("", write_spheres(100)); OK("rs", rt_render(c)); OK("rs", rt_wait(c)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    OK("", write_spheres(200));
    step("3. variant 5 (brute force, single kernel; prep for the parameters written above)");
    OK("", rt_set_variant(c, 5)); OK("rs", rt_render(c)); OK("rs", rt_render(c));
    step("3. n = 400: two hierarchy frames in flight, then variant 5: the queue's allocation drains; then the pipeline behind frames in flight");
    OK("", write_spheres(400)); OK("", rt_set_variant(c, 0)); OK("rs", rt_render(c)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 5));
    OK("rs", rt_render(c)); OK("rs", rt_render(c)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    step("3. n = 300, a brute-force frame in flight, then variant 0: the first build of the hierarchy drains; the plan is the one made before");
    OK("", write_spheres(300)); OK("", rt_set_variant(c, 5)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 0)); OK("rs", rt_render(c));
    OK("rs", rt_wait(c));
    step("3. variants 2, 3 and 4 at n = 8");
    OK("", write_spheres(8)); OK("", rt_set_variant(c, 2)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 3)); OK("rs", rt_render(c));
    OK("", rt_set_variant(c, 1)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 4)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    step("3. a variant without a form for the scene: refused before anything is enqueued, with a frame in flight");
    OK("", rt_set_variant(c, 1)); OK("rs", rt_render(c));
    g_fits = false;
    CALL("rs", rt_render(c)); OK("", rt_set_variant(c, 4)); OK("rs", rt_render(c));                   // the hierarchy kernel is not asked
    OK("", rt_set_variant(c, 1));
    g_fits = true;
    // the refused call has moved rt_render's stream on, not its colour buffer: the fourth frame from here writes the buffer of the first
    // frame of the batch on another stream, and waits for it
    for (int i = 0; i < 3; ++i) OK("rs", rt_render(c));
    OK("rs", rt_wait(c));
    step("3. RT_MODE_STRICT, under variants 1 and 4; then a scene whose bound defeats the filter, in fast mode");
    OK("", rt_set_mode(c, RT_MODE_STRICT)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 4)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    OK("", rt_set_mode(c, RT_MODE_FAST)); OK("", write_spheres(9, true)); OK("rs", rt_render(c)); OK("", rt_set_variant(c, 2));
    OK("rs", rt_render(c)); OK("", rt_set_variant(c, 0)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    step("3. no spheres at all");
    OK("", write_spheres(0)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));

    step("4. a textured sky (2x2 faces) over n = 200: the end-of-path records, rotating; six frames in flight");
    OK("", write_sky(2)); OK("", write_spheres(200)); OK("", rt_set_variant(c, 5));
    OK("rs", rt_render(c));                   // brute force reads no such records: in flight when the next frame allocates them
    OK("", rt_set_variant(c, 0)); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    for (int i = 0; i < 6; ++i) OK("rs", rt_render(c));
    OK("rs", rt_wait(c));
    step("4. not seamless: one face 1x1 among 2x2 faces");
    {
        const uint8_t px[4] = {1, 2, 3, 4};
        OK("", rt_write_cubemap_face(c, 3, 1, 1, px));
    }
    OK("rs", rt_render(c)); OK("rs", rt_wait(c)); OK("", write_sky(1));

    step("5. rt_render_to on the caller's streams: three frames on one stream");
    hipStream_t mine[5];
    void* dst = nullptr;
    for (int k = 0; k < 5; ++k) if (hipStreamCreateWithFlags(&mine[k], hipStreamNonBlocking) != hipSuccess) return 1;
    const size_t dst_bytes = 64u * 40u * 4u;
    if (hipMalloc(&dst, dst_bytes) != hipSuccess) return 1;
    CALL("rs", rt_render_to(c, nullptr, dst_bytes, mine[0])); CALL("rs", rt_render_to(c, dst, dst_bytes - 1u, mine[0]));
    for (int i = 0; i < 3; ++i) OK("rs", rt_render_to(c, dst, dst_bytes, mine[0]));
    OK("rs", rt_wait(c));
    step("5. alternating over two streams, then over five; then the library's own stream (NULL), then rt_render");
    for (int i = 0; i < 4; ++i) OK("rs", rt_render_to(c, dst, dst_bytes, mine[i % 2]));
    OK("rs", rt_wait(c));
    for (int i = 0; i < 6; ++i) OK("rs", rt_render_to(c, dst, dst_bytes, mine[i % 5]));
    OK("rs", rt_wait(c)); OK("rs", rt_render_to(c, dst, dst_bytes, nullptr)); OK("rs", rt_render_to(c, dst, dst_bytes, nullptr));
    OK("rs", rt_wait(c)); OK("rs", rt_render(c)); OK("rs", rt_render_to(c, dst, dst_bytes, mine[1])); OK("rs", rt_render(c)); OK("rs", rt_wait(c));
    step("5. a streaming read-back pending on the colour buffer the next frame takes");
    {
        std::vector<uint8_t> host(dst_bytes);
        OK("rs", rt_render(c)); OK("", rt_read_pixels_async(c, 0, host.data(), host.size()));
        for (int i = 0; i < 4; ++i) OK("rs", rt_render(c));
        OK("", rt_read_pixels_wait(c)); OK("rs", rt_read_pixels(c, host.data(), host.size()));
    }

    step("6. the ring full: RT355_MAX_IN_FLIGHT + 2 frames without a wait; the plan of the 65th is made before it waits inside");
    OK("", write_spheres(100)); OK("rs", rt_render(c));
    OK("rs", rt_wait(c));                     // one awaited frame: the hint is off, 100 spheres render by brute force
    for (int i = 0; i < RT355_MAX_IN_FLIGHT + 2; ++i) OK(i >= RT355_MAX_IN_FLIGHT - 1 ? "rs" : "", rt_render(c));
    OK("rs", rt_wait(c)); OK("rs", rt_render(c));                   // ... and the next batch has the hint
    OK("rs", rt_wait(c));

    step("7. triangles: a small form (the instance data in the arguments), instance_uploads follows inst.gen");
    OK("", rt_write_triangles(c, tris.data(), n_tris));
    g_form = 1;
    OK("rsfv", rt_render(c)); OK("rsfv", rt_render(c)); OK("rs", rt_wait(c)); OK("", rt_write_blas(c, blas.data(), n_blas)); OK("rsfv", rt_render(c));
    OK("rsfv", rt_render(c)); OK("rs", rt_wait(c));
    step("7. form 0: apply_instances, the version's event, the waits for the frames that read the version");
    g_form = 0;
    for (int i = 0; i < 6; ++i) OK("rsv", rt_render(c));
    OK("rs", rt_wait(c));
    step("7. per-frame instance writes between frames: awaited, then in flight");
    for (int i = 0; i < 2; ++i) {
        OK("", rt_write_blas(c, blas.data(), n_blas)); OK("rsv", rt_render(c)); OK("rs", rt_wait(c));
    }
    for (int i = 0; i < 6; ++i) {
        if (i != 3) OK("", rt_write_nodes(c, 0, nodes.data(), 1));
        OK("rsv", rt_render(c));
    }
    OK("rs", rt_wait(c));
    step("7. ... on three caller streams: a version another stream brought up to date is waited for");
    OK("", rt_write_blas_lookup(c, blas_lookup.data(), n_blas_lookup));
    for (int i = 0; i < 9; ++i) OK("rsv", rt_render_to(c, dst, dst_bytes, mine[i % 3]));
    OK("rs", rt_wait(c));
    for (int i = 0; i < 5; ++i) OK("rsv", rt_render(c));
    OK("rs", rt_wait(c));
    step("7. a device ray query that reads a version (two lookup entries over one instance), then a form-0 frame that rewrites one");
    {
        void* rays = nullptr;
        void* hits = nullptr;
        if (hipMalloc(&rays, 4u * 32u) != hipSuccess || hipMalloc(&hits, 4u * 32u) != hipSuccess) return 1;
        const float two[2] = {blas_lookup[0], blas_lookup[0]};
        OK("", rt_write_blas_lookup(c, two, 2)); OK("rv", rt_trace_rays(c, static_cast<const float*>(rays), 4, static_cast<rt_hit*>(hits), mine[2]));
        OK("rsv", rt_render(c)); OK("", rt_write_blas(c, blas.data(), n_blas));
        OK("rv", rt_trace_rays(c, static_cast<const float*>(rays), 4, static_cast<rt_hit*>(hits), mine[2]));
        OK("", rt_write_blas(c, blas.data(), n_blas)); OK("rsv", rt_render(c)); OK("rsv", rt_render(c)); OK("rs", rt_wait(c));
        OK("", rt_write_blas_lookup(c, blas_lookup.data(), n_blas_lookup));
        if (hipFree(rays) != hipSuccess || hipFree(hits) != hipSuccess) return 1;
    }
    step("7. a write that invalidates the corners while frames are in flight");
    g_form = 1;
    OK("rsv", rt_render(c)); OK("rsv", rt_render(c)); OK("", rt_write_tri_lookup(c, tri_lookup.data(), n_tri_lookup));
    OK("rsv", rt_render_to(c, dst, dst_bytes, mine[3])); OK("rsv", rt_render(c)); OK("rs", rt_wait(c));
    step("7. pair records: a node write that dirties them on four consecutive frames (in flight): the cooldown, the node walk, the retry");
    for (int i = 0; i < 6; ++i) {
        OK("", rt_write_nodes(c, (size_t)(n_nodes - 1u) * 32u, nodes.data() + 8u * (size_t)(n_nodes - 1u), 1)); OK("rsf", rt_render(c));
        if (i == 1) OK("rsf", rt_render(c));          // a frame that need not rebuild: the streak survives only frames back to back
    }
    OK("rs", rt_wait(c));
    for (int i = 0; i < 5; ++i) {
        OK("", rt_write_nodes(c, (size_t)(n_nodes - 1u) * 32u, nodes.data() + 8u * (size_t)(n_nodes - 1u), 1)); OK("rsf", rt_render(c));
    }
    std::printf("# driver: flow_cooldown %u -> 1 (59 more frames on the node walk would look the same)\n", c->flow_cooldown);
    c->flow_cooldown = 1u;
    OK("rsf", rt_render(c)); OK("rsf", rt_render(c)); OK("rsf", rt_render(c)); OK("rs", rt_wait(c));
    step("7. a new root set: the union of the roots; back to the first set: nothing to build");
    {
        std::vector<float> other_root(blas);
        other_root[16] = blas[16] + 2.0f;
        OK("", rt_write_blas(c, other_root.data(), n_blas)); OK("rsf", rt_render(c)); OK("", rt_write_blas(c, blas.data(), n_blas));
        OK("rsf", rt_render(c)); OK("rs", rt_wait(c));
    }
    step("7. a stale copy and a root that is a leaf: a build without pair records, nothing to upload; rt_trace_fits is not asked");
    {
        std::vector<float> leaf_root(blas);
        leaf_root[16] = blas[16] + 1.0f;
        OK("", rt_write_nodes(c, (size_t)(n_nodes - 1u) * 32u, nodes.data() + 8u * (size_t)(n_nodes - 1u), 1));
        OK("", rt_write_blas(c, leaf_root.data(), n_blas));
        g_fits = false;
        OK("rsf", rt_render(c));
        g_fits = true;
        OK("", rt_write_blas(c, blas.data(), n_blas)); OK("rsf", rt_render(c)); OK("rs", rt_wait(c));
    }
    step("7. variant 6 and the heatmap kernel: no pair records, no list");
    OK("", rt_set_variant(c, 6)); OK("rsf", rt_render(c)); OK("", rt_set_variant(c, 0)); OK("", rt_select_kernel(c, RT_KERNEL_HEATMAP));
    OK("rsf", rt_render(c)); OK("", rt_select_kernel(c, RT_KERNEL_RAYTRACER)); OK("rs", rt_wait(c));
    step("7. seventeen instances: the records do not travel with the frame (write_versions), no pair records");
    {
        std::vector<float> many, many_lookup;
        for (int i = 0; i < 17; ++i) { many.insert(many.end(), blas.begin(), blas.begin() + 20); many_lookup.push_back((float)i); }
        OK("", rt_write_blas(c, many.data(), 17)); OK("", rt_write_blas_lookup(c, many_lookup.data(), 17));
        g_form = 0;
        OK("rsfv", rt_render(c)); OK("rsfv", rt_render(c)); OK("rs", rt_wait(c)); OK("", rt_write_blas(c, blas.data(), n_blas));
        OK("", rt_write_blas_lookup(c, blas_lookup.data(), n_blas_lookup));
        g_form = 1;
    }

    step("8. the work list, 512x512 (4,096 tiles): the first awaited frame allocates, the second has the list");
    OK("", rt_resize(c, 512, 512)); OK("rso", rt_render(c));                  // the hint of the last batch: no list
    OK("rso", rt_wait(c)); OK("rso", rt_render(c)); OK("rso", rt_wait(c)); OK("rso", rt_render(c)); OK("rso", rt_wait(c));
    step("8. the list splits tiles (the pinned word order_hist leaves): roles");
    c->h_split[c->stream_rot] = 3ull;
    std::printf("# driver: h_split[%u] = 3\n", c->stream_rot);
    OK("rso", rt_render(c)); OK("rso", rt_wait(c));
    c->h_split[c->stream_rot] = 0ull;
    step("8. 520x512: both grow; a heatmap frame (no list); a first batch in flight (a set per stream), a second (the hint: none); a caller's stream (none), the NULL stream (the library's)");
    OK("", rt_resize(c, 520, 512)); OK("rso", rt_render(c)); OK("rso", rt_wait(c)); OK("", rt_select_kernel(c, RT_KERNEL_HEATMAP));
    OK("rso", rt_render(c)); OK("rso", rt_wait(c)); OK("", rt_select_kernel(c, RT_KERNEL_RAYTRACER));
    for (int i = 0; i < 3; ++i) OK("rso", rt_render(c));
    OK("rso", rt_wait(c));
    for (int i = 0; i < 2; ++i) OK("rso", rt_render(c));
    OK("rso", rt_wait(c)); OK("rso", rt_render(c));                  // the hint: no list
    OK("rso", rt_wait(c)); OK("rso", rt_render(c));                  // awaited again: the list, from the frame two back on this stream
    OK("rso", rt_wait(c));
    {
        void* big = nullptr;
        const size_t big_bytes = 520u * 512u * 4u;
        if (hipMalloc(&big, big_bytes) != hipSuccess) return 1;
        OK("rso", rt_render_to(c, big, big_bytes, mine[4])); OK("rso", rt_wait(c)); OK("rso", rt_render_to(c, big, big_bytes, nullptr));
        OK("rso", rt_wait(c));
        if (hipFree(big) != hipSuccess) return 1;
    }
    step("8. 504x512 (63 x 64 = 4,032 tiles, below kOrderMinTiles): none; rank 1 of 2 over 512x1024: the LOCAL tiles count (64 x 64)");
    OK("", rt_resize(c, 504, 512)); OK("rso", rt_render(c)); OK("rso", rt_wait(c)); OK("", rt_resize(c, 512, 1024));
    OK("", rt_set_partition(c, 1, 2)); OK("rso", rt_render(c)); OK("rso", rt_wait(c)); OK("rso", rt_render(c)); OK("rso", rt_wait(c));
    OK("", rt_set_partition(c, 0, 1));

    step("destroy, with a frame in flight");
    OK("", rt_resize(c, 64, 40)); OK("rs", rt_render(c));
    if (hipFree(dst) != hipSuccess) return 1;
    {
        rt_ctx* last = c;
        c = nullptr;
        OK("", rt_destroy(last));
    }
    for (int k = 0; k < 5; ++k) if (hipStreamDestroy(mine[k]) != hipSuccess) return 1;
    std::printf("# live allocations: %zu\n", g_live.size());
    return 0;
}
