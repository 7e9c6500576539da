/*
 * rt355.h -- C ABI of librt355.so, the MI355X (gfx950) stand-in for the WebGPU
 * calls the reference's RendererRaytracing makes.
 *
 * Every entry point names the reference interface it replaces; citations are
 * relative to the reference repository:
 *   RR = src/rendering-raycast/renderer-raytracing.ts
 *   RK = src/rendering-raycast/shaders/raytracer-kernel.wgsl
 *   CM = src/material/cubemap-material.ts
 *   MT = src/material/material.ts
 *
 * Conventions
 *   - plain C: pointers and sizes only; no C++/torch/HIP types in any signature
 *     (a HIP stream crosses as void*).
 *   - every function returns int: RT_OK (0) or a negative rt_status.  The message
 *     for the most recent failure on the calling thread is rt_last_error().
 *   - every rt_write_* copies out of caller memory before it returns, as
 *     GPUQueue.writeBuffer does (RR:165); the caller may reuse/free at once.
 *   - byte layouts are exactly the ones RR writes (f32 indices and counts,
 *     vec3 padded to 16 B), so buffers captured from a browser run replay unchanged.
 *   - a context is bound to ONE device and is not thread-safe (single JS thread in
 *     the reference).  Multi-GPU: the frame is split into 8-row tiles (one WGSL
 *     workgroup row, RK:73), tile t is rendered by rank t % world, and the LIBRARY
 *     moves the compact per-rank tile buffers over RCCL (xGMI) and de-interleaves
 *     them: rt_comm_init + rt_render_gather (one process per GPU) or rt_group_create +
 *     rt_group_render (one process, all GPUs).  rt_set_partition / rt_render_to /
 *     rt_assemble_frame remain for hosts that bring their own transport.
 *   - there is no CPU fallback anywhere in this library.
 */
#ifndef RT355_H
#define RT355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT355_ABI_VERSION 4

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,  /* null pointer, bad size, bad enum                      */
    RT_ERR_NO_DEVICE = -2,    /* no gfx950 device / ordinal out of range                */
    RT_ERR_HIP = -3,          /* a HIP runtime call failed (message has the hipError)   */
    RT_ERR_UNSUPPORTED = -4,  /* combination not supported (e.g. heatmap of a sphere scene) */
    RT_ERR_STATE = -5,        /* call order: e.g. render before resize / write_params   */
    RT_ERR_CAPACITY = -6,     /* destination buffer too small                           */
    RT_ERR_COMM = -7          /* an RCCL call failed, a peer reported an asynchronous error, or the
                                 exchange did not complete within rt_set_comm_timeout: the communicator was
                                 aborted and stays unusable until rt_comm_destroy / rt_group_destroy        */
} rt_status;

/* Which kernel form rendered a frame (rt_stats.kernel_id): the library chooses by scene type, sphere
 * count, LDS footprint and mode; callers that price a frame (bench.py) read it from here. */
typedef enum rt_kernel_id {
    RT_KID_NONE = 0,
    RT_KID_LITERAL = 1,          /* trace_pixels, the reference's loop as written (strict mode, or a scene outside the filter's range) */
    RT_KID_BRUTE_SINGLE = 2,     /* trace_pixels with the FMA filter: one kernel, every sphere tested */
    RT_KID_BRUTE_PIPELINE = 3,   /* first_bounce + trace_paths over a path queue */
    RT_KID_HIERARCHY_8 = 4,      /* bvh_pixels, 8-wave workgroups, three per CU, nodes in LDS */
    RT_KID_HIERARCHY_12 = 5,     /* 12-wave workgroups, two per CU */
    RT_KID_HIERARCHY_16 = 6,     /* 16-wave workgroups, one per CU */
    RT_KID_HIERARCHY_GLOBAL = 7, /* nodes read from global memory (scenes beyond a CU's LDS) */
    RT_KID_TRIANGLES = 8,        /* trace_triangles (TLAS / BLAS traversal) */
    RT_KID_HEATMAP = 9,          /* heatmap_triangles */
    RT_KID_TRIANGLES_ROLES = 10  /* trace_roles: an awaited frame whose work list splits tiles -- the idle lanes of a part walk the next reflection ray while its pixels' lanes walk the shadow ray */
    /* (10, 11: the persistent triangle kernels of ABI 3 -- measured slower on every configuration, removed in ABI 4;
       docs/experiments.md keeps the account) */
} rt_kernel_id;

typedef enum rt_kernel {
    RT_KERNEL_RAYTRACER = 0,  /* RR:70-72 showRaytracer()  */
    RT_KERNEL_HEATMAP = 1     /* RR:74-76 showHeatmap(): traversal-cost visualiser, triangle scenes only */
} rt_kernel;

/* Arithmetic mode of the ray-trace kernel.
 * RT_MODE_STRICT: no FMA contraction, IEEE div/sqrt, the oracle's operation order ->
 *                 expected bit-identical to oracle/rt_oracle.c.
 * RT_MODE_FAST  : FMA contraction allowed (default); parity within the tolerance stated
 *                 in tests/test_parity_gpu.py. */
typedef enum rt_mode { RT_MODE_FAST = 0, RT_MODE_STRICT = 1 } rt_mode;

typedef struct rt_ctx rt_ctx;

typedef struct rt_stats {
    uint32_t width, height;       /* current target                                        */
    uint32_t local_tiles;         /* 8-row tiles this context renders                      */
    uint32_t spheres;             /* primitives in the scene                               */
    uint64_t rays;                /* scene traversals of the last completed render:
                                     primary/reflection (RK:114) + shadow (RK:153) rays    */
    float kernel_ms;              /* hipEvent time of the last ray-trace kernel launch     */
    float prep_ms;                /* hipEvent time of the last per-frame scene preparation  */
    uint32_t frames;              /* completed renders since rt_create                     */
    int mode;                     /* rt_mode in effect                                     */
    uint32_t batch_frames;        /* renders completed by the last rt_wait                  */
    float batch_kernel_ms;        /* sum of their ray-trace kernel times (hipEvents on the
                                     stream each kernel was launched on)                    */
    float gather_ms;              /* rt_render_gather / rt_group_render: RCCL exchange + de-interleave of the
                                     last frame (hipEvents, same stream); kernel_ms then is the render alone */
    float batch_gather_ms;        /* ... summed over the frames the last rt_wait completed   */
    uint32_t kernel_id;           /* rt_kernel_id of the latest frame enqueued                */
    uint32_t grid_share;          /* that frame's share of the chip: 1 = all resident slots, k = 1/k of them
                                     (frames on k distinct streams in flight)                 */
    uint32_t instance_uploads;    /* frames whose per-frame instance data (rt_write_blas / _blas_lookup /
                                     _nodes at offset 0) travelled with the frame, without a drain */
    uint32_t tri_form;            /* triangle scenes: the stack form of the latest frame's kernel -- 0: twenty top-level slots,
                                     1: four (a top-level tree of depth <= 4 within 16 nodes), five waves per SIMD, 2: three
                                     (depth <= 3, 8 nodes, <= 4 instances), six waves per SIMD, 3: eight (depth <= 8, 24 nodes),
                                     five waves, 4: eight with sixteen staged instances (13-16 instances or 32 nodes), five waves
                                      */
    uint32_t pair_rebuilds;       /* times the library rebuilt its relinked copy of the BLAS trees (a drain + an upload:
                                     a node write reached the trees, or a frame named a root the copy did not know) */
} rt_stats;

/* ---- lifetime ---------------------------------------------------------------------- */

/* Replaces navigator.gpu.requestAdapter()/requestDevice() (RR:82-86).  `device` is the HIP
 * ordinal; its streams are created on it.  Fails (RT_ERR_NO_DEVICE) when no GPU is present. */
int rt_create(int device, rt_ctx** out);
int rt_destroy(rt_ctx* ctx);

/* Thread-local message of the last failure ("" if none).  `ctx` may be NULL. */
const char* rt_last_error(rt_ctx* ctx);

int rt_abi_version(void);

/* sha256 (hex, first 16 digits) of the library's sources at build time: profiles taken with one build are
 * not evidence for another (bench.py matches it against profiles/traffic.json). */
const char* rt_build_id(void);
/* Name of a kernel form, e.g. "bvh_pixels<8>" (static storage). */
const char* rt_kernel_name(int kernel_id);

/* ---- resources ----------------------------------------------------------------------- */

/* Replaces createTexture({size:{width,height}, format:'rgba8unorm'}) (RR:102-109): the
 * W x H x 4 B colour buffer, row-major, row 0 = top.  Re-callable.  1 <= W, H <= 65536 and
 * fewer than 2^31 pixels (padded to 8x8 tiles). */
int rt_resize(rt_ctx* ctx, uint32_t width, uint32_t height);

/* Replaces queue.writeBuffer(sceneParameters, 0, Float32Array(24)) (RR:157-165).
 * p[0..2] cameraPos, [4..6] forwards, [8..10] right, [12..14] up, [16..18] lightPosition,
 * [19] lightIntensity, [20] minIntensity, [21] maxBounces (f32, truncated by u32(), RK:110). */
int rt_write_params(rt_ctx* ctx, const float params[24]);

/* Sphere primitives: `n` records of 8 f32 {cx,cy,cz,_, r,g,b, radius} = the WGSL layout of
 * the reference's commented `struct Sphere` (RK:13-17; model/sphere.ts:1-10).  Takes the
 * place of the triangle/BVH uploads (RR:198-229) for sphere scenes.  n may be 0. */
int rt_write_spheres(rt_ctx* ctx, const float* records, uint32_t n);

/* Replaces copyExternalImageToTexture(face i) (CM:73-77).  face order as CM:40-47:
 * 0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z; rgba8unorm, w*h*4 bytes, row 0 = top.  Six equal squares
 * are a WebGPU cube texture and filter seamlessly across edges; other image sets clamp per image.
 * Memory: a sphere scene rendered through the hierarchy kernel under a sky that is not one colour
 * keeps 32 bytes per local pixel of end-of-path records in each of four frame slots (the sky is
 * sampled by a second kernel): 1.06 GB per slot at 7680x4320, allocated when a
 * frame first needs them. */
int rt_write_cubemap_face(rt_ctx* ctx, int face, uint32_t w, uint32_t h, const uint8_t* rgba);

/* The reference's live scene type: triangles behind a two-level BVH (RK:168-410).  Same byte
 * layouts as RR writes: 160-B triangles (RR:198-209), 32-B nodes {min.xyz, leftChildIndex,
 * max.xyz, primitiveCount} (indices and counts as f32), 80-B BLAS records {inverseModel
 * column-major, rootNodeIndex, pad}, f32 lookup tables.  rt_write_nodes takes a byte offset like
 * queue.writeBuffer(nodeBuffer, offset, ...): the TLAS nodes are rewritten every frame at offset
 * 0 (RR:184-192), the BLAS nodes once at 32*tlasNodesMax (RR:212-223).  Writing triangles or
 * nodes switches the context to the triangle scene; rt_write_spheres switches back. */
/* Per-frame instance data.  The reference rewrites the BLAS records, the BLAS lookup and the TLAS nodes
 * before EVERY frame (RR:169-192; scene-raytracing.ts:138-143).  Those three writes -- rt_write_blas and
 * rt_write_blas_lookup of up to 16 instances, rt_write_nodes inside the first 31 nodes -- do not wait for
 * the frames in flight: the library keeps their current contents on the host, and the next frame carries
 * them to the device itself (in the kernarg block of a one-workgroup kernel, in front of the ray-trace
 * kernel on the frame's stream, into one of four versions of the three buffers -- a frame in flight keeps
 * reading the version it was enqueued with).  Larger instance sets, and every other rt_write_*, drain. */
int rt_write_triangles(rt_ctx* ctx, const float* data, uint32_t n_triangles);        /* RR:198-209 */
int rt_write_nodes(rt_ctx* ctx, size_t byte_offset, const float* data, uint32_t n);  /* RR:184-192, 212-223 */
int rt_write_blas(rt_ctx* ctx, const float* data, uint32_t n_blas);                  /* RR:169-174 */
int rt_write_tri_lookup(rt_ctx* ctx, const float* data, uint32_t n);                 /* RR:225-229 */
int rt_write_blas_lookup(rt_ctx* ctx, const float* data, uint32_t n);                /* RR:177-181 */
int rt_write_mesh_texture(rt_ctx* ctx, uint32_t w, uint32_t h, const uint8_t* rgba); /* MT:61-65 */

/* Replaces selecting one of the two compute pipelines (RR:70-76, RR:356-374). */
int rt_select_kernel(rt_ctx* ctx, int kernel);

/* Arithmetic mode (no reference counterpart: WGSL leaves fp contraction to the driver). */
int rt_set_mode(rt_ctx* ctx, int mode);

/* Kernel variant for A/B measurements (0 = library default).  Fast-mode sphere scenes:
 * 0 = bounding-sphere hierarchy from 128 spheres on (from 72 on once the caller keeps frames in flight), single
 * brute-force kernel below;
 * 4 = hierarchy for any sphere count; 5 = brute force (two-kernel pipeline from 320 spheres on);
 * 1, 2, 3 = individual brute-force forms; a frame none of whose forms holds the scene (variant 1 above 2,176 spheres, 2 and 3
 * above 3,264, up to 4,608 -- beyond that each reads the records from global memory) fails rt_render with RT_ERR_UNSUPPORTED
 * before anything of it is enqueued.  Triangle scenes: 0 = one workgroup per tile (rt_triangles.hip), reading the BLAS
 * trees from the library's relinked pair records where the scene fits them (up to 12 instances, node buffer and lookup table
 * within 16-bit indices); 6 = the same kernel on the reference's node buffer only.  Every variant produces the same pixels.
 * See DESIGN.md. */
int rt_set_variant(rt_ctx* ctx, int variant);

/* ---- multi-GPU partition --------------------------------------------------------------- */

/* This context renders the 8-row tiles t with t % world == rank, into a compact buffer of
 * rt_local_tiles() * 8 rows.  Default rank 0, world 1 = the whole frame. */
int rt_set_partition(rt_ctx* ctx, uint32_t rank, uint32_t world);

/* Tiles owned by `rank`, and the padded per-rank tile count (max over ranks) that sizes the
 * all-gather message: bytes = rt_padded_tiles * 8 * width * 4. */
uint32_t rt_tiles_of_rank(uint32_t height, uint32_t rank, uint32_t world);
uint32_t rt_padded_tiles(uint32_t height, uint32_t world);

/* ---- frame ------------------------------------------------------------------------------- */

/* Replaces beginComputePass/setPipeline/setBindGroup/dispatchWorkgroups(ceil(W/8),
 * ceil(H/8),1)/submit (RR:442-446, RR:465): enqueues scene preparation + the ray-trace
 * kernel and returns without waiting.  The reference keeps one frame in flight (RR:467) --
 * rt_render + rt_wait per frame does the same.  A caller that enqueues frames back to back
 * gets up to four of them running concurrently (the library rotates over four streams
 * and four colour buffers, each concurrent frame taking a share of the chip): the
 * dependent-ray tail of one frame then runs beside the bulk of the next.  Every frame uses
 * the parameters and scene written before its rt_render call; rt_read_pixels returns the
 * frame of the latest rt_render.  Up to RT355_MAX_IN_FLIGHT frames may be enqueued between
 * two rt_wait; beyond that the library drains by itself.  Scene-setup calls (rt_write_spheres,
 * rt_write_cubemap_face, rt_write_triangles ..., rt_resize, rt_set_partition) wait for the
 * frames in flight first; rt_write_params does not need to. */
#define RT355_MAX_IN_FLIGHT 64
int rt_render(rt_ctx* ctx);

/* Replaces `await queue.onSubmittedWorkDone()` (RR:467). */
int rt_wait(rt_ctx* ctx);

/* Copies this context's tiles (world 1: the W*H*4 frame) to host memory.
 * Needs cap >= local_tiles*8*W*4 clipped to the frame. */
int rt_read_pixels(rt_ctx* ctx, uint8_t* dst, size_t cap);

/* Streaming read-back: frames kept in flight AND copied out.  rt_read_pixels returns the latest frame only and waits;
 * a host that wants every frame of a pipelined sequence begins an asynchronous copy per frame instead: the frame
 * `frames_back` rt_render calls ago (0 = the latest, at most 3 -- the library rotates over four colour buffers) is copied
 * to `dst` on a copy stream of the library's own, behind that frame's kernels and beside the rendering of the frames
 * after it; a later frame that would overwrite the colour buffer waits for the copy, nothing else does.  `dst` should be
 * pinned memory (rt_host_alloc) -- with pageable memory the copy is staged and the call may block.  rt_read_pixels_wait
 * returns when every copy begun so far has landed.  Whole-frame contexts only (no partition, no rt_render_gather). */
int rt_read_pixels_async(rt_ctx* ctx, uint32_t frames_back, uint8_t* dst, size_t cap);
int rt_read_pixels_wait(rt_ctx* ctx);
int rt_host_alloc(size_t bytes, void** out);   /* pinned host memory (hipHostMalloc) */
int rt_host_free(void* p);

int rt_get_stats(rt_ctx* ctx, rt_stats* out);

/* ---- device-pointer interop (process-per-GPU hosts: torch.distributed / RCCL) --------- */

/* As rt_render, but the kernel runs on `hip_stream` (a hipStream_t; NULL = the context's
 * stream) and writes the compact tile buffer to `device_dst` (device memory of this
 * context's GPU, >= rt_padded_tiles*8*W*4 bytes).  Nothing is copied to the host.  Frames
 * enqueued on different streams (into different buffers) may run concurrently, as with
 * rt_render; frames on one stream execute in order. */
int rt_render_to(rt_ctx* ctx, void* device_dst, size_t cap, void* hip_stream);

/* De-interleaves an all-gathered buffer [world][padded_tiles][8][W][4] into the row-major
 * frame [H][W][4] (both device memory) on `hip_stream`. */
int rt_assemble_frame(rt_ctx* ctx, const void* gathered, void* frame, uint32_t world,
                      void* hip_stream);

/* Device address of the colour buffer of the latest rt_render (valid until the next
 * rt_render / rt_resize / rt_destroy). */
int rt_device_pixels(rt_ctx* ctx, void** out_ptr, size_t* out_bytes);

/* ---- ray queries: the nearest hit of rays the host supplies (RK:168-244 / RK:311-322 without the shading) ------------------ */

/* One ray: 8 f32 = {origin.xyz, tmin, dir.xyz, tmax}.  Words 3 and 7 are read only under RT_QUERY_LIMITS (rt_trace_rays_ex,
 * rt_occluded); everywhere else they are ignored.
 * dir need not be unit length; t is in units of |dir|, as in the reference's arithmetic. */
typedef struct rt_hit {
    float t;          /* nearest hit, RK:168-244 traceTLAS / RK:311-322 over spheres: tMin 0.001, search starts at 9999; -1 on a miss */
    float u, v;       /* triangle barycentrics of RK:378-379 (object space); 0 for spheres and misses                        */
    int32_t prim;     /* triangle: u32(triangleLookup[slot]) (index into rt_write_triangles' records); sphere: record index; -1 miss */
    int32_t instance; /* triangle: BLAS record index bi of RK:223 (= order of rt_write_blas = scene.instances); -1 spheres / miss */
    float normal[3];  /* the renderer's shading normal: RK:334-338 (transpose(inverseModel) * n, normalised) / HK:320; 0 on a miss */
} rt_hit;             /* 32 bytes */

/* rt_trace_rays: `rays` ([n][8] f32) and `hits` ([n] rt_hit) in device memory of this context's GPU, 16-byte aligned; enqueued on
 * `hip_stream` (NULL = the context's stream), returns at once, like rt_render_to.  rt_trace_rays_host: host memory, synchronous
 * (staged through device buffers the context owns, which grow as needed).  rt_pick: the primary ray of each pixel (x, y) --
 * xy = [n][2] u32 -- under the current rt_write_params and rt_resize, exactly the ray that pixel of the next frame starts with;
 * host memory, synchronous.  Coordinates are full-frame even under rt_set_partition; one outside W x H: RT_ERR_INVALID_ARG.
 *
 * Contract.
 *   - A query sees the scene the next rt_render would render: every rt_write_* made before it, on any stream, per-frame
 *     instance writes that no frame has carried yet included.  Results are bit for bit the reference's arithmetic (the
 *     oracle's rt_oracle_trace_tri_rays / hit_sphere); sphere scenes are searched with the literal loop, every sphere in
 *     index order (the lowest index wins a tie).
 *   - n == 0: RT_OK, nothing done.  A NULL pointer: RT_ERR_INVALID_ARG.  No scene written: RT_ERR_STATE.
 *   - Queries are not frames: they take no slot of the event ring, change no field of rt_stats, have no rt_kernel_id, and are
 *     unaffected by rt_select_kernel, rt_set_mode and rt_set_variant.
 *   - Frames in flight are never disturbed.  A query waits for the last scene update, not for frames; it drains only where a
 *     frame would: the first query or frame after rt_write_triangles / _tri_lookup builds the library's corner array, and a
 *     scene whose instance data does not travel with frames (more than sixteen instances) may need its per-frame buffers
 *     brought up to date.  Queries run in call order, whatever their streams; scene writes after a query wait for it. */
int rt_trace_rays(rt_ctx* ctx, const float* rays, uint32_t n, rt_hit* hits, void* hip_stream);  /* device memory, async     */
int rt_trace_rays_host(rt_ctx* ctx, const float* rays, uint32_t n, rt_hit* hits);               /* host memory, synchronous */
int rt_pick(rt_ctx* ctx, const uint32_t* xy, uint32_t n, rt_hit* hits);                         /* host memory, synchronous */

/* ---- bounded and occlusion queries ---------------------------------------------------------------------------------------- */

/* flags of rt_trace_rays_ex / rt_occluded */
#define RT_QUERY_LIMITS 1u   /* ray word 3 is tmin, word 7 is tmax */

/* rt_trace_rays_ex / rt_trace_rays_host_ex: rt_trace_rays / rt_trace_rays_host with flags.  rt_occluded / rt_occluded_host: whether
 * anything blocks each ray: occluded[i] = 1 or 0, one byte per ray.  Memory, streams and the contract of rt_trace_rays above apply
 * word for word (`rays` 16-byte aligned, `hits` too; `occluded` needs no alignment).  Unknown flag bits: RT_ERR_INVALID_ARG.
 *
 * Limits.
 *   - flags = 0: the search is today's (tmin 0.001, search starts at 9999); words 3 and 7 are ignored, whatever they hold.
 *   - RT_QUERY_LIMITS: word 3 is tmin and replaces the 0.001 of the acceptance tests (triangles RK:380 `t > tmin && t < tMax`,
 *     spheres HK:318); word 7 is tmax and replaces the 9999 the running nearest hit starts from (RK:172).  Box pruning stays the
 *     reference's (`d1 > nearest`, `d2 < nearest`).  (0.001, 9999) gives exactly rt_trace_rays.
 *   - A NaN limit, or tmin >= tmax: a miss (the strict inequalities).
 *   - A negative tmin is allowed: triangles behind the origin can then be hit.  Spheres still use only the near root (HK:317).
 *   - A tmax of 99999 or more is honoured, but it disables the pruning of boxes the ray misses (hit_aabb's 99999, RK:405-407):
 *     results stay correct, the walk gets slower.
 *
 * Occlusion.  occluded[i] = 1 if and only if rt_trace_rays_ex with the same flags reports a hit for ray i.  The walk stops at the
 * first accepted triangle or sphere; until then it takes the limited nearest search's steps under the same bound, so both accept
 * their first primitive at the same step or not at all. */
int rt_trace_rays_ex(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, rt_hit* hits, void* hip_stream);  /* device, async */
int rt_trace_rays_host_ex(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, rt_hit* hits);               /* host, sync   */
int rt_occluded(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, uint8_t* occluded, void* hip_stream);  /* device, async */
int rt_occluded_host(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, uint8_t* occluded);               /* host, sync   */

/* ---- multi-hit queries: the k nearest hits along each ray -------------------------------------------------------------------- */

#define RT355_MAX_HITS 8u    /* the largest k of rt_trace_rays_multi */

/* rt_trace_rays_multi / rt_trace_rays_multi_host: the first k surfaces each ray crosses, in order.  `rays` are the 8-float records
 * above; `flags` is 0 or RT_QUERY_LIMITS with exactly rt_trace_rays_ex's meaning (words 3 and 7 are tmin and tmax, otherwise 0.001
 * and 9999).  `hits` is [n][k] rt_hit: ray i's records are hits[i*k .. i*k+k), the filled ones first in the order below, the rest the
 * miss record of rt_trace_rays (t = -1, prim = instance = -1, everything else 0).  There is no count array: count prim >= 0.
 * Device form: `rays` and `hits` in device memory of this context's GPU, 16-byte aligned, enqueued on `hip_stream` (NULL = the
 * context's stream), returns at once.  Host form: host memory, synchronous, staged through the context's query buffers (which grow
 * to n*k*32 bytes for the hits).
 *
 * Which hits.
 *   - Triangle scenes: a hit is a pair of an instance and a triangle-lookup slot under that instance's BLAS root that passes
 *     hitTriangle's tests (RK:344-379, back faces culled) with tmin < t < tmax, both strict.  t, u, v and the normal are exactly
 *     rt_trace_rays' for that triangle and instance; t is the world ray parameter, so hits of different instances compare.
 *   - Sphere scenes: a hit is a sphere whose near root (HK:316-317, disc > 0) lies in (tmin, tmax): at most one hit per sphere,
 *     and a ray that starts inside a sphere does not see it, as in the reference.
 *   - Reported are the k smallest under the total order ascending t, then ascending instance, then ascending prim (spheres: t, then
 *     index), sorted by it.  The result does not depend on the order the walk visits things: surfaces at exactly equal t
 *     (coincident instances, duplicated spheres) are all kept, which calling rt_trace_rays_ex again with tmin = t cannot do.
 *
 * Pruning.  The bound is tmax while a ray holds fewer than k hits and the t of its k-th hit afterwards.  A box is skipped only
 * when its entry distance is strictly greater than the bound, and the far child is visited when its distance is <= the bound (the
 * reference's nearest search has <): a surface at exactly the k-th t that sorts before the k-th entry replaces it.  The note on
 * tmax >= 99999 of rt_trace_rays_ex applies unchanged.
 *
 * Relation to the other queries.  On a scene whose trees the reference's walk searches exhaustively (every tree the library's and
 * the reference's builders make), hit 0's t is bit for bit rt_trace_rays_ex's t, the miss sets agree, and rt_occluded is 1 exactly
 * where hit 0 exists.  On an exact tie hit 0 may name a different triangle than rt_trace_rays_ex, whose winner depends on the
 * order of its walk; for spheres it names the same one, the lowest index.
 * On hand-made trees the walk does not search exhaustively (a spine deeper than the twenty stack slots, boxes that do not nest)
 * the walk clamps its stacks as the nearest search does and is memory-safe; its records are still true hits, distinct, sorted and
 * within the limits, and it promises no more than that.
 *
 * Checks, in this order: unknown flag bits, then k == 0 or k > RT355_MAX_HITS, then a NULL context: RT_ERR_INVALID_ARG;
 * n == 0: RT_OK; a NULL buffer: RT_ERR_INVALID_ARG; no scene written: RT_ERR_STATE.  Otherwise the contract of rt_trace_rays
 * above applies word for word: a query sees every write made before it, takes no slot of the event ring, changes no field of
 * rt_stats, has no rt_kernel_id, is unaffected by mode and variant, never disturbs frames in flight, and queries run in call order. */
int rt_trace_rays_multi(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, uint32_t k, rt_hit* hits, void* hip_stream);  /* device, async */
int rt_trace_rays_multi_host(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, uint32_t k, rt_hit* hits);               /* host, sync   */

/* ---- shaded ray queries: the renderer's colour along rays the host supplies (RK:101-144, optionally RK:91-96) -------------- */

typedef struct rt_shade { float r, g, b, dist; } rt_shade;      /* 16 bytes */

/* flags of rt_shade_rays */
#define RT_SHADE_COMPOSE 1u   /* r, g, b is pixelColor (RK:91-96) instead of rayColor */

/* rt_shade_rays / rt_shade_rays_host: what the renderer would show along each ray.  Rays are the 8-float records above
 * {origin.xyz, -, dir.xyz, -}; words 3 and 7 are ignored.  Device form: `rays` and `out` ([n] rt_shade) in device memory of this
 * context's GPU, 16-byte aligned, enqueued on `hip_stream` (NULL = the context's stream), returns at once.  Host form: host memory,
 * synchronous, staged through the context's query buffers.
 *
 * flags = 0: out[i] is the vec4 rayColor(origin, dir) returns (RK:143).
 *   - r, g, b: the running-mean colour after up to u32(maxBounces) bounces; every hit casts a shadow ray from the light
 *     (RK:146-166); on a miss the sky is sampled along the path's last direction (RK:122-125).
 *   - dist: the first segment's t (RK:116-118), or 0 when the first ray misses or maxBounces is 0.
 *   - dir is used as given, nothing normalises it: dist is in units of |dir|.  From the first reflection on, directions are the
 *     shader's own normalised ones.
 * RT_SHADE_COMPOSE: r, g, b is instead pixelColor of RK:91-96 before the rgba8 store -- k = clamp((30 - dist) / 30, 0, 1),
 * k * rayColor + (1 - k) * minIntensity * sky(dir as given); dist stays in word 3.  Shading pixel (x, y)'s primary ray (rt_pick's
 * ray: RK:76-86) with this flag and quantising each channel by RK:98's rule (floor(clamp(c, 0, 1) * 255 + 0.5), NaN -> 0) gives
 * exactly that pixel of the next frame.
 *
 * State read.  Light position, intensities and maxBounces are those of the last rt_write_params, copied at the call as a frame
 * copies them: a later rt_write_params does not reach a query already enqueued.  The camera words are not read.  The sky and the mesh
 * texture are what the next frame would sample (no mesh texture written: 1x1 white, as for a frame).
 *
 * Contract.  The contract of rt_trace_rays above applies word for word: a query sees every write made before it, per-frame instance
 * writes that no frame has carried yet included; takes no slot of the event ring, changes no field of rt_stats, has no rt_kernel_id;
 * is unaffected by rt_select_kernel, rt_set_mode and rt_set_variant; never disturbs frames in flight; queries run in call order, and
 * scene writes after one wait for it.  Results are bit for bit the reference's arithmetic (the oracle's rt_oracle_ray_color for sphere
 * scenes, its float frame for triangle scenes); sphere scenes are searched with the literal loop, every sphere in index order, for the
 * path ray and the shadow ray alike.
 *   - Unknown flag bits: RT_ERR_INVALID_ARG (checked first, whatever the context).  A NULL pointer: RT_ERR_INVALID_ARG.
 *   - n == 0: RT_OK, nothing done.
 *   - No scene written, no rt_write_params yet, or a cube map face missing: RT_ERR_STATE. */
int rt_shade_rays(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, rt_shade* out, void* hip_stream);   /* device, async */
int rt_shade_rays_host(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t flags, rt_shade* out);                /* host, sync   */

/* ---- supersampled frames: s x s camera rays per pixel, resolved on the device ------------------------------------------------ */

#define RT355_MAX_SUPERSAMPLE 4u   /* the largest s of rt_render_samples */

/* rt_render_samples / rt_render_samples_host: the whole width x height frame of the last rt_resize, anti-aliased -- a frame-shaped
 * shaded query that makes its own rays, whatever rt_set_partition says (as for rt_pick).  Device form: the outputs in device
 * memory of this context's GPU, enqueued on `hip_stream` (NULL = the context's stream), returns at once.  Host form: host memory,
 * synchronous, staged through buffers the context owns.
 *
 * Outputs.  rgba8 is [height][width][4] bytes, row 0 at the top, with a frame's alpha byte (255); in the device form 4-byte aligned.
 * rgbaf is [height][width][4] float {r, g, b, 1.0f}; in the device form 16-byte aligned.  Either may be NULL, not both.  cap8 and
 * capf are the sizes of the two buffers in bytes (ignored for a NULL output).
 *
 * A pixel.  For sy = 0 .. s-1 (outer) and sx = 0 .. s-1 (inner), c[sy s + sx] is pixelColor (RK:91-96, float) along the primary ray
 * of pixel (x s + sx, y s + sy) of an (s width) x (s height) target: the ray rt_pick would cast were the target that size
 * (RK:76-86), under the camera of the last rt_write_params, copied at the call.  Per channel acc = c[0]; acc = acc + c[1]; ... in
 * that order, mean = acc / (float)(s s) -- float32 throughout, one IEEE division, no fused multiply-add.  rgbaf holds mean; rgba8
 * holds RK:98's rule applied to it (floor(clamp(mean, 0, 1) * 255 + 0.5), NaN -> 0).  s = 1 is byte for byte the frame rt_render
 * would produce.  No sample is stored anywhere: the s s colours of a pixel are added on the chip.
 *
 * Contract.  That of rt_shade_rays, word for word: sees every write made before it, per-frame instance writes that no frame has
 * carried yet included; takes no slot of the event ring, changes no field of rt_stats, has no rt_kernel_id; is unaffected by
 * rt_select_kernel, rt_set_mode and rt_set_variant; never disturbs frames in flight; queries run in call order, and scene writes
 * after one wait for it.  Sphere scenes are searched with the literal loop.
 *
 * Checks, in this order: s == 0 or s > RT355_MAX_SUPERSAMPLE, then a NULL context, then both outputs NULL (or, in the device form,
 * a misaligned one): RT_ERR_INVALID_ARG.  Then RT_ERR_STATE, as for rt_shade_rays: no rt_resize, no scene written, no
 * rt_write_params, or a cube map face missing.  Then cap8 < width * height * 4 or capf < width * height * 16 for a non-NULL output:
 * RT_ERR_CAPACITY. */
int rt_render_samples(rt_ctx* ctx, uint32_t s, uint8_t* rgba8, size_t cap8, float* rgbaf, size_t capf, void* hip_stream);   /* device, async */
int rt_render_samples_host(rt_ctx* ctx, uint32_t s, uint8_t* rgba8, size_t cap8, float* rgbaf, size_t capf);                /* host, sync    */

/* ---- geometry frames: per pixel the depth, normal, ids and barycentrics of what the camera sees ------------------------------- */

typedef struct rt_gbuffer {
    float*   depth;   /* [h][w]    f32: rt_hit.t of the pixel's primary ray, -1 on a miss       */
    float*   normal;  /* [h][w][4] f32: rt_hit.normal, word 3 = 0; all 0 on a miss              */
    int32_t* ids;     /* [h][w][2] i32: {rt_hit.prim, rt_hit.instance}; -1, -1 on a miss        */
    float*   uv;      /* [h][w][2] f32: {rt_hit.u, rt_hit.v}; 0, 0 for spheres and misses       */
} rt_gbuffer;         /* any plane may be NULL, not all four */

/* rt_render_gbuffer / rt_render_gbuffer_host: a frame-shaped nearest-hit query that makes its own rays -- rt_pick over a rectangle
 * of the frame, each field of the hits as a dense plane of its own, and only the planes asked for.  Device form: the planes in device
 * memory of this context's GPU (depth 4-byte, ids and uv 8-byte, normal 16-byte aligned), enqueued on `hip_stream` (NULL = the
 * context's stream), returns at once.  Host form: host memory, synchronous, staged through query buffers the context owns, which
 * grow as needed.
 *
 * rect is {x0, y0, w, h} in full-frame pixel coordinates of the last rt_resize, whatever rt_set_partition says (as for rt_pick and
 * rt_render_samples); NULL is the whole frame.  It is read on the host at the call, in both forms.  The planes are [h][w] of the
 * rectangle, row 0 at the top; a 1 x 1 rectangle is the device form of rt_pick.  cap_pixels is the number of pixels every non-NULL
 * plane has room for.
 *
 * A pixel.  Pixel (x, y) of the rectangle holds the rt_hit that rt_pick returns for frame pixel (x0 + x, y0 + y), field for field
 * and bit for bit: the ray of RK:76-86 under the camera of the last rt_write_params, copied at the call, searched as rt_trace_rays
 * searches (tMin 0.001, the running nearest hit starting at 9999; sphere scenes with the literal loop, every sphere in index order).
 * No ray and no coordinate is stored anywhere: a lane makes its ray in registers, and a plane that is NULL costs no store.  No sky,
 * mesh texture, light or maxBounces is read: a missing cube map face is not an error here.
 *
 * Contract.  That of rt_trace_rays, word for word: sees every write made before it, per-frame instance writes that no frame has
 * carried yet included; takes no slot of the event ring, changes no field of rt_stats, has no rt_kernel_id; is unaffected by
 * rt_select_kernel, rt_set_mode and rt_set_variant; never disturbs frames in flight; queries run in call order, and scene writes
 * after one wait for it.
 *
 * Checks, in this order: a NULL context, a NULL `out`, all four planes NULL, or in the device form a misaligned plane:
 * RT_ERR_INVALID_ARG.  Then RT_ERR_STATE: no rt_resize, no scene written, or no rt_write_params.  Then a rectangle with w == 0 or
 * h == 0, or with x0 + w > width or y0 + h > height (the sums taken in 64 bits): RT_ERR_INVALID_ARG.  Then cap_pixels < w * h:
 * RT_ERR_CAPACITY. */
int rt_render_gbuffer(rt_ctx* ctx, const uint32_t* rect, const rt_gbuffer* out, size_t cap_pixels, void* hip_stream); /* device, async */
int rt_render_gbuffer_host(rt_ctx* ctx, const uint32_t* rect, const rt_gbuffer* out, size_t cap_pixels);             /* host, sync   */

/* ---- ambient-occlusion frames: per pixel, how many of k rays over the hemisphere of what the camera sees are blocked ----------- */

#define RT355_MAX_AO_RAYS 64u

typedef struct rt_ao {
    uint8_t* count;   /* [h][w]    u8 : how many of the k rays are occluded; 0 on a miss        */
    float*   ao;      /* [h][w]    f32: (float)(k - count) / (float)k; 1.0f on a miss            */
} rt_ao;              /* either may be NULL, not both */

/* rt_render_ao / rt_render_ao_host: rt_render_gbuffer's depth and normal planes, k rays per pixel made from them and rt_occluded over
 * those rays, in one kernel that keeps a pixel's hit point and tangent frame in registers -- no plane, no ray and no per-ray answer
 * in memory.  Device form: the planes in device memory of this context's GPU (ao 4-byte aligned), enqueued on `hip_stream` (NULL =
 * the context's stream), returns at once.  Host form: host memory, synchronous, staged through query buffers the context owns.
 *
 * rect and cap_pixels are rt_render_gbuffer's: {x0, y0, w, h} in full-frame pixels of the last rt_resize whatever the partition, NULL
 * the whole frame, read at the call; the planes are [h][w] of the rectangle, row 0 at the top, and cap_pixels is the room of every
 * non-NULL plane in pixels.  dirs is HOST memory in both forms: k directions, [k][3] f32, in the tangent space of the shading
 * normal (z along the normal).  It is copied at the call -- a later change to the array does not reach an enqueued call.  Nothing
 * normalises or checks the directions.  (tmin, radius) are the limits of every ray, exactly as under RT_QUERY_LIMITS; NaN limits or
 * tmin >= radius are not errors: every ray is then a miss and every count 0.
 *
 * A pixel, in float32 without fused multiply-add, one operation per line, in this order:
 *   h = the rt_hit that rt_pick returns for the pixel; on a miss count = 0, ao = 1.0f and nothing else is done;
 *   p = o + h.t * d per component (one multiply, one add: HK:319), o the camera origin and d the pixel's primary direction;
 *   n = h.normal;  s = (n.z >= 0) ? 1 : -1  (so -0 gives +1 and NaN gives -1);  a = -1 / (s + n.z);  b = (n.x * n.y) * a;
 *   T = (1 + ((s * n.x) * n.x) * a,  s * b,  (-s) * n.x);   B = (b,  s + (n.y * n.y) * a,  -n.y);
 *   ray j: origin p, direction (dirs[j].x * T + dirs[j].y * B) + dirs[j].z * n per component, limits (tmin, radius);
 *   count = the number of j for which rt_occluded (RT_QUERY_LIMITS) reports 1 for that ray -- the same walk taking the same steps,
 *   back faces culled as there; sphere scenes use the literal loop for the primary ray and the k rays, the normal from HK:320.
 * No sky, mesh texture, light or maxBounces is read.
 *
 * Contract.  That of rt_render_gbuffer, word for word: sees every write made before it; takes no slot of the event ring, changes no
 * field of rt_stats, has no rt_kernel_id; is unaffected by rt_select_kernel, rt_set_mode and rt_set_variant; never disturbs frames
 * in flight; queries run in call order, and scene writes after one wait for it.
 *
 * Checks, in this order: k == 0 or k > RT355_MAX_AO_RAYS: RT_ERR_INVALID_ARG.  Then a NULL context, NULL `dirs`, NULL `out`, both
 * planes NULL, or in the device form an `ao` plane that is not 4-byte aligned: RT_ERR_INVALID_ARG.  Then RT_ERR_STATE: no rt_resize,
 * no scene written, or no rt_write_params.  Then the rectangle, as for rt_render_gbuffer: RT_ERR_INVALID_ARG.  Then
 * cap_pixels < w * h: RT_ERR_CAPACITY. */
int rt_render_ao(rt_ctx* ctx, const uint32_t* rect, const float* dirs, uint32_t k, float tmin, float radius, const rt_ao* out, size_t cap_pixels, void* hip_stream); /* device, async */
int rt_render_ao_host(rt_ctx* ctx, const uint32_t* rect, const float* dirs, uint32_t k, float tmin, float radius, const rt_ao* out, size_t cap_pixels);             /* host, sync   */

/* ---- instance visibility masks: which instances the rays of a query may see --------------------------------------------------- */

/* rt_write_instance_masks / rt_set_query_masks: every instance has a 32-bit mask, every ray a query casts carries one, and an
 * instance is visible to a ray if and only if (instance mask & ray mask) != 0.  An instance is a BLAS record: its index bi is the
 * value of RK:223 after the library's clamp to n_blas - 1, the number rt_hit.instance reports.  A ray never enters the BLAS of an
 * instance it cannot see -- no ray transform, no box test and no triangle test there.  The top-level walk does not change: its box
 * tests, its order, its stack, the guard of RK:212 and the running nearest hit are what they are without masks.  With every mask at
 * its default, 0xFFFFFFFF, every query returns the bits it returns without this section.  Sphere scenes have no instances: the masks
 * are kept and ignored, and every sphere stays visible.
 *
 * rt_write_instance_masks: `masks` is HOST memory, n words, copied before the call returns.  Record i < n takes masks[i]; records
 * from n on have 0xFFFFFFFF.  n == 0 clears the table (`masks` may then be NULL).
 *   - The table indexes records, not models, and belongs to no scene buffer: it survives rt_write_blas, rt_write_blas_lookup,
 *     per-frame instance writes, rt_refit_blas and rt_build_blas, whatever the record count becomes.  It may be written before any
 *     scene, and on a context that holds spheres.
 *   - For queries it is a scene write: a query sees every mask write made before it, on any stream.  The write waits for the queries
 *     enqueued before it, and those keep the table they were enqueued with.
 *   - No frame reads the table: the write does not drain, does not wait for frames and does not disturb them.
 *   - Checks, in this order: a NULL context, then n > 0 with NULL `masks`: RT_ERR_INVALID_ARG.
 *
 * rt_set_query_masks: the two ray masks of the context, both 0xFFFFFFFF until set.  They are copied at each query call, as the
 * parameters are: a later change does not reach a query already enqueued.  A NULL context: RT_ERR_INVALID_ARG.
 *   - `nearest` is the mask of every nearest-hit search: rt_trace_rays, _host, _ex, _host_ex; rt_trace_rays_multi, _host; rt_pick;
 *     rt_render_gbuffer, _host; the primary ray of rt_render_ao, _host; and every ray of rt_shade_rays, _host and rt_render_samples,
 *     _host -- path rays and shadow rays alike, the reference's shadow test (RK:147-165) being a nearest-hit search.
 *   - `occlusion` is the mask of rt_occluded, _host and of the k rays of rt_render_ao, _host.
 *   - With both masks equal, occluded[i] = 1 if and only if rt_trace_rays_ex reports a hit for ray i, as without masks; every
 *     relation between the queries stated above holds among queries that carry the same mask.
 *
 * Frames ignore both: rt_render, rt_render_to, rt_render_gather, rt_group_render and the heatmap see every instance, and their
 * rt_stats are what they are without masks.  A masked frame is rt_render_samples with s = 1.  No entry point above gains a flag bit;
 * there are no per-ray masks. */
int rt_write_instance_masks(rt_ctx* ctx, const uint32_t* masks, uint32_t n);   /* host memory */
int rt_set_query_masks(rt_ctx* ctx, uint32_t nearest, uint32_t occlusion);

/* ---- closest-point queries: the nearest surface point to points the host supplies ----------------------------------------------- */

typedef struct rt_closest {
    float dist2;      /* squared world distance to the nearest surface point; -1: nothing within the radius */
    float u, v;       /* barycentrics of that point on the triangle: weight of corner B, of corner C (rt_hit's meaning) */
    int32_t prim;     /* u32(triangleLookup[slot]), as rt_hit.prim; -1 */
    int32_t instance; /* BLAS record index, as rt_hit.instance; -1 */
    float point[3];   /* the surface point, world space; 0 */
} rt_closest;         /* 32 bytes */

/* rt_closest_points / rt_closest_points_host: for each point {x, y, z, radius} ([n][4] f32) the nearest point of the triangle scene's
 * surface within the radius, in all directions -- the query no ray can stand in for.  Device form: `points` and `out` in device
 * memory of this context's GPU, 16-byte aligned, enqueued on `hip_stream` (NULL = the context's stream), returns at once.  Host
 * form: host memory, synchronous, staged through the context's query buffers.
 *
 * What the answer is (csrc/rt_closest.h holds every expression; it is the definition).
 *   1. Candidates.  Every pair of an instance bi that a leaf of the top-level tree names and whose mask shares a bit with the
 *      context's nearest-hit ray mask (rt_set_query_masks), and a triangle-lookup slot in a leaf under the root of bi's BLAS record:
 *      the slots traceBLAS (RK:246-332) can reach.  Back faces count: nothing is culled.
 *   2. Corners.  The object corners A, B, C are words 0-2, 12-14 and 24-26 of the triangle record.  The instance's forward matrix is
 *      Fm = mat4.invert (rt_build_tlas' invert: float64, one rounding) of record words 0..15, a float32 result.  Component k of a world
 *      corner is ((Fm[k] x + Fm[4+k] y) + Fm[8+k] z) + Fm[12+k] in float64, left to right, rounded once to float32.  The matrix is
 *      treated as affine: its bottom row is not read.
 *   3. Leaf.  The closest point of the float32 point to the float32 world triangle, in float64, by the region tests of Ericson,
 *      Real-Time Collision Detection 5.1.5, tested in the order vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior; every
 *      dot product (x x' + y y') + z z', no fused multiply-add; d2 = (ex ex + ey ey) + ez ez with e = p - q.  dist2, u, v and point are
 *      those float64 values rounded once to float32.  Nothing reported passes through a square root.
 *   4. Acceptance.  r2 = radius * radius in float32; a candidate counts iff dist2 <= r2, compared on the rounded value.  A negative or
 *      NaN radius gives the miss record, +inf an unbounded search.  A candidate whose dist2 is NaN (zero-area triangles, which the ray
 *      tests never hit either) is no candidate.
 *   5. Winner.  The smallest candidate under the total order (dist2, instance, prim).  Miss: dist2 = -1, prim = instance = -1,
 *      everything else 0.
 * The result therefore does not depend on the order of the walk: points on a shared edge or vertex, and coincident instances, tie
 * exactly in dist2 and resolve by index.
 *
 * The walk visits both levels nearest box first and skips a box only when a lower bound of the world distance to anything in it is
 * strictly beyond the best distance so far (so an exact tie is still visited); the bound holds under any affine instance matrix
 * (DESIGN.md 4.7j).  It keeps 20 top-level and 32 bottom-level stack entries per point, one per level: every tree rt_build_blas,
 * rt_build_tlas and the host builders make is searched exhaustively.  On a hand-made tree deeper than that the walk drops what its
 * stacks cannot hold and is memory-safe; it reports only true candidates, and promises no more than that.  Tight top-level boxes
 * (rt_build_tlas) are what make the search prune across instances; under the reference's placeholder boxes every instance is entered.
 *
 * Contract.  That of rt_trace_rays, word for word: sees every write made before it, per-frame instance writes that no frame has
 * carried yet included; takes no slot of the event ring, changes no field of rt_stats, has no rt_kernel_id; is unaffected by
 * rt_select_kernel, rt_set_mode and rt_set_variant; never disturbs frames in flight; queries run in call order, and scene writes
 * after one wait for it.
 *
 * Checks, in this order: a NULL context: RT_ERR_INVALID_ARG; n == 0: RT_OK; a NULL buffer, or in the device form a misaligned one:
 * RT_ERR_INVALID_ARG; no scene written: RT_ERR_STATE; a sphere scene: RT_ERR_UNSUPPORTED (a sphere's distance needs a square root
 * inside the reported value) -- the context stays usable.
 *
 * rt_closest_points_model: the same search, serially, on caller arrays in the layouts of rt_write_* (triangles 40 floats each, nodes 8,
 * BLAS records 20; `masks` as for rt_write_instance_masks, `ray_mask` the nearest-hit mask) -- no device and no context, the same
 * inline arithmetic as the kernel.  *tests (may be NULL) receives the number of (instance, slot) candidates evaluated.  n == 0:
 * RT_OK; a NULL array (masks with n_masks != 0 included): RT_ERR_INVALID_ARG; an empty array: RT_ERR_STATE. */
int rt_closest_points(rt_ctx* ctx, const float* points /* [n][4] {x,y,z,radius} */, uint32_t n, rt_closest* out, void* hip_stream); /* device, async */
int rt_closest_points_host(rt_ctx* ctx, const float* points, uint32_t n, rt_closest* out);                                          /* host, sync   */
int rt_closest_points_model(const float* points, uint32_t n, const float* triangles, uint32_t n_triangles,
                            const float* tri_lookup, uint32_t n_tri_lookup, const float* nodes, uint32_t n_nodes,
                            const float* blas, uint32_t n_blas, const float* blas_lookup, uint32_t n_blas_lookup,
                            const uint32_t* masks, uint32_t n_masks, uint32_t ray_mask,
                            rt_closest* out, uint64_t* tests /* may be NULL */);

/* ---- multi-GPU: render + RCCL gather behind one call (RR:434-470 across a group of GPUs) ------ */

/* One process per GPU.  Rank 0 calls rt_comm_unique_id and hands the bytes to the other ranks by
 * any side channel (a TCP store, MPI, a file); then EVERY rank calls rt_comm_init on its context
 * (collective: ncclCommInitRank on the context's device).  It fixes the context's partition to
 * (rank, world) as rt_set_partition does. */
#define RT355_COMM_ID_BYTES 128
int rt_comm_unique_id(uint8_t id[RT355_COMM_ID_BYTES]);
int rt_comm_init(rt_ctx* ctx, const uint8_t id[RT355_COMM_ID_BYTES], uint32_t rank, uint32_t world);
int rt_comm_destroy(rt_ctx* ctx);      /* back to a single-GPU context (rank 0 of 1) */

/* Failure of a peer.  rt_wait on a context with a communicator polls its frames' events and, between
 * polls, ncclCommGetAsyncError; when RCCL reports an error, or when `ms` > 0 and the frames have not
 * completed within `ms` milliseconds of the rt_wait call, the communicator is aborted (ncclCommAbort:
 * the exchange kernels leave the device), rt_wait returns RT_ERR_COMM, and every later rt_render_gather /
 * rt_group_render on it returns RT_ERR_COMM at once.  The context stays valid for rt_comm_destroy,
 * rt_destroy and single-GPU rendering.  A host that wants to retry forms a new group (in a fresh child
 * process if the GPU itself is gone).  ms = 0 (default): no deadline, errors only.  The deadline bounds the whole rt_wait --
 * the render kernels of the frames in flight AND their exchanges --, so it must be chosen above the slowest batch of frames the
 * host enqueues (a full-size C5 frame renders for ~20 ms on one GPU): it is a liveness bound, not a latency target. */
int rt_set_comm_timeout(rt_ctx* ctx, uint32_t ms);

/* Collective; replaces RendererRaytracing.render()'s submit (RR:442-446, 465) for the whole group:
 * this rank's tiles are rendered, exchanged over RCCL on the same stream and de-interleaved into the
 * row-major W x H frame.  root >= 0: only that rank receives (grouped ncclSend / ncclRecv -- each
 * rank's tiles travel once, over its direct xGMI link to the root); root = -1: every rank receives
 * (ncclAllGather).  Returns after enqueueing; rt_wait completes it.  Frames enqueued back to back
 * overlap on the device as with rt_render (four streams / buffer sets).  Every rank of the group must
 * make the same sequence of rt_render_gather calls with the same root. */
int rt_render_gather(rt_ctx* ctx, int root);

/* The frame of the latest rt_render_gather on a rank that received it: device address (valid until
 * four more frames are enqueued / rt_resize / rt_destroy; after rt_resize or rt_set_partition the call
 * fails with RT_ERR_STATE until the next rt_render_gather), or a copy to host memory (waits first;
 * cap >= W*H*4).  RT_ERR_STATE on a rank that did not receive.  rt_read_pixels / rt_device_pixels
 * keep returning this rank's own tiles. */
int rt_frame_pixels(rt_ctx* ctx, void** out_ptr, size_t* out_bytes);
int rt_read_frame(rt_ctx* ctx, uint8_t* dst, size_t cap);

/* One process, all GPUs -- the shape of the reference's host, ONE JavaScript thread (src/app.ts):
 * a context per device (n_devices = 0: every visible device) joined by ncclCommInitAll.  Scene and
 * parameters are written per member: for (i < rt_group_size(g)) rt_write_*(rt_group_ctx(g, i), ...).
 * rt_group_render enqueues the render on every device, the exchange (one RCCL group over all
 * devices) and the de-interleave; rt_group_wait completes it; the frame is read from the root's
 * context with rt_read_frame / rt_frame_pixels (root = -1: from any member). */
typedef struct rt_group rt_group;
int rt_group_create(int n_devices, rt_group** out);
int rt_group_destroy(rt_group* g);
int rt_group_size(const rt_group* g);
rt_ctx* rt_group_ctx(rt_group* g, int i);
int rt_group_render(rt_group* g, int root);
int rt_group_wait(rt_group* g);

/* ---- diagnostics -------------------------------------------------------------------------- */

/* Runs the HOST side of the sphere path on its own -- the build of the bounding-sphere
 * hierarchy the fast mode walks -- without a device or a context, so that it can
 * be checked on a machine without a GPU.  `records` as for rt_write_spheres.  Writes n_nodes + 1
 * node records (4 floats each: centre * 2^40, (|C|^2 (1-2^-17) - R^2 (1+2^-16)) * 2^80; leaf records
 * are zero here, the device fills them) and links (inner node: 4 * index of the first node after
 * its subtree; leaf: 0x80000000 | sphere index; the last entry is the sentinel).  RT_ERR_CAPACITY
 * when cap_nodes < n_nodes + 1 (*n_nodes is set either way; at most 2 n + 64 nodes). */
int rt_build_hierarchy(const float* records, uint32_t n, float* rec4, uint32_t* link, uint32_t cap_nodes,
                       uint32_t* n_nodes);

/* rt_build_hierarchy with the build's own figures.  The tree is built top-down and then optimised by `passes` rounds of
 * reinsertion ("Structure"); rt_build_hierarchy and the renderer use RT355_HIERARCHY_PASSES, 0 gives the
 * top-down tree as built.  info (may be NULL) receives four doubles: the node count of the top-down tree (the optimised
 * tree has the same), the reinsertions kept, and the cost -- the sum over inner nodes of (radius of the members' bound)^2
 * x children, which goes with the number of node tests a ray makes -- of the top-down tree and of the tree written (never
 * higher). */
#define RT355_HIERARCHY_PASSES 1u
int rt_build_hierarchy_ex(const float* records, uint32_t n, float* rec4, uint32_t* link, uint32_t cap_nodes,
                          uint32_t* n_nodes, uint32_t passes, double* info);

/* Runs the HOST side of the triangle kernel's pair-record forms on its own (no device, no context): the relinked copy of the BLAS
 * trees they walk.  `nodes`: the node buffer as rt_write_nodes receives it (8 f32 per node); `roots`: the
 * rootNodeIndex of every instance.  Writes *n_pairs records of 16 words {c1.min.xyz, meta1, c1.max.xyz, 0, c2.min.xyz, meta2,
 * c2.max.xyz, 0} -- the two children of an inner node, meta = primitiveCount << 16 | x with x = the leaf's first lookup
 * slot or the inner child's own record number -- ordered most-visited first (by the surface area of the parent's box), and
 * per root its meta.  RT_ERR_UNSUPPORTED for a node buffer beyond 65,536 entries or a primitiveCount beyond 65,535 (such scenes
 * are rendered by the tile-per-wave kernel), RT_ERR_CAPACITY when cap_pairs < *n_pairs (*n_pairs is set either way). */
int rt_build_flow(const float* nodes, uint32_t n_nodes, const uint32_t* roots, uint32_t n_roots, float* pairs, uint32_t cap_pairs,
                  uint32_t* n_pairs, uint32_t* root_meta);

/* Diagnostic (needs the context's device): the two kernels that turn the per-tile times of an awaited triangle frame into the
 * next frame's work list (rt_triangles.hip: order_hist, order_scatter), run on `cost[n]` (10 ns ticks) for a
 * device of `wave_slots` resident waves.  Writes order[0] = tiles to be rendered as four quarters, order[1] = as sixteen 2x2
 * blocks, order[2 .. 2 + n) = the tiles, longest class first (quarter-octave classes of the cost; within a class any order).
 * cap: entries of `order`, >= n + 2.  The kernels run twice on the same device buffers (they must leave their scan space and the
 * costs zero for the next frame); the second pass is returned.  The library calls the same kernels behind every awaited frame of
 * >= 4096 tiles. */
int rt_order_tiles(rt_ctx* ctx, const uint32_t* cost, uint32_t n, uint32_t wave_slots, uint32_t* order, size_t cap);

/* The bounding-sphere hierarchy on the device, as the latest frame that walked one left it: inner node records
 * after the refit of moved spheres (rt_bvh.hip: bvh_refit) or as the host built them, leaf records as the
 * device filled them (the filter records of the spheres), the links and the sentinel -- the layout of
 * rt_build_hierarchy.  Waits for the frames in flight first; changes nothing a later frame renders.
 * RT_ERR_STATE when the context holds no hierarchy (a triangle scene, or no frame has walked one yet);
 * RT_ERR_CAPACITY when cap_nodes < n_nodes + 1 (*n_nodes is set either way). */
int rt_read_hierarchy(rt_ctx* ctx, float* rec4, uint32_t* link, uint32_t cap_nodes, uint32_t* n_nodes);

/* ---- deforming meshes: partial triangle writes and a refit of the bottom-level trees on the device ------------------------------ */

/* rt_update_triangles: queue.writeBuffer(triangleBuffer, first * 160, data) -- replaces records [first, first + n) of the triangle
 * buffer, in the layout of rt_write_triangles, from host memory.  A scene-setup call: it waits for the frames in flight, and frames
 * and queries after it see the new records (the library's corner array follows by itself).  On its own it changes no node: it is
 * exactly a partial rt_write_triangles.  first + n (taken in 64 bits) beyond the triangles written: RT_ERR_INVALID_ARG, nothing
 * changes; n == 0: RT_OK.
 *
 * rt_refit_blas: new boxes for every node of the bottom-level trees under `roots` -- node indices, the rootNodeIndex values of the
 * BLAS records as u32(f32) reads them; duplicates are refitted once; roots == NULL with n_roots == 0: every root the current BLAS
 * records name.  The box of a node is, per axis, fminf / fmaxf over the three float32 corners of every triangle in the leaves
 * below it, starting from (float)1e30 and (float)-1e30 (a NaN corner is skipped): exact, so a tree whose vertices did not move
 * comes back bit for bit as the project's builders made it.  Words 3 and 7 of a node are never written, and no node outside the
 * named trees is: the top-level nodes stay the host's (it reads the new root boxes through rt_read_nodes if it wants them).
 * The trees are walked on the host first, on the library's mirror of the node buffer, nothing clamped: a reached node index at
 * or beyond the node count, a leaf run beyond the lookup table, or a node reached twice over all the roots (sharing, a cycle):
 * RT_ERR_INVALID_ARG; a node whose leaves do not form one contiguous run of lookup slots (no builder makes one):
 * RT_ERR_UNSUPPORTED; either way nothing on the device or in the context has changed.  The walk is kept while the structure of
 * the trees, the lookup table's size and the roots stay the same.  The boxes are computed on the device (rt_refit.hip) and
 * stored into every copy a kernel reads: all versions of the node buffer and the library's relinked pair records -- a refit
 * does not make the next frame rebuild those (rt_stats.pair_rebuilds).  Synchronous, and a scene-setup call: waits for the
 * frames in flight.
 *
 * Both: RT_ERR_STATE without a triangle scene; a NULL context (or NULL data / roots with a non-zero count): RT_ERR_INVALID_ARG. */
int rt_update_triangles(rt_ctx* ctx, uint32_t first, uint32_t n, const float* data);      /* host memory */
int rt_refit_blas(rt_ctx* ctx, const uint32_t* roots, uint32_t n_roots);

/* Diagnostic: copies `n` nodes (8 f32 each) starting at node `first_node` from the device to `dst` -- the version of the node
 * buffer the next frame would read, with per-frame writes of its head applied, as a frame or a query sees them.  Waits for the
 * frames in flight.  first_node + n beyond the nodes written: RT_ERR_INVALID_ARG. */
int rt_read_nodes(rt_ctx* ctx, uint32_t first_node, uint32_t n, float* dst);

/* Runs the HOST side of rt_refit_blas on its own (no device, no context): the validation above and its result, one triple
 * {node, first_slot, n_slots} per reached node (roots ascending, each tree depth-first, the left child first): the node's box is
 * the min / max over lookup slots [first_slot, first_slot + n_slots).  `nodes` as rt_write_nodes receives them, n_tri_lookup
 * the length of the triangle lookup table.  Returns rt_refit_blas' status codes; RT_ERR_CAPACITY when cap_nodes < *n_plan
 * (*n_plan is set either way; 0 on the other failures). */
int rt_refit_plan(const float* nodes, uint32_t n_nodes, uint32_t n_tri_lookup, const uint32_t* roots, uint32_t n_roots,
                  uint32_t* plan, uint32_t cap_nodes, uint32_t* n_plan);

/* ---- device mesh deformation: the vertices of a deforming mesh from device memory into the triangle records ---------------------- */

#define RT_DEFORM_FLAT_NORMALS 1u   /* flags of rt_deform_triangles: the three corners get the unit normal of the new triangle */

/* rt_deform_triangles: rewrites the positions (and optionally the normals) of triangle records [first, first + n) from vertex arrays
 * in DEVICE memory, produced on `hip_stream` (NULL: none to wait for) -- rt_update_triangles for callers whose vertices live on the
 * device and who do not keep 160-byte records.  For triangle i of the call and corner c: the vertex index is
 * k = faces ? min(faces[3 i + c], V - 1) : 3 i + c; words 12 c + 0..2 of record first + i become vertices[3 k + 0..2] and, when
 * `normals` is given, words 12 c + 4..6 become normals[3 k + 0..2], all copied bit for bit (NaN and inf as they are).  With
 * RT_DEFORM_FLAT_NORMALS the three corners get n / len instead, computed from the new corners A, B, C in float32 with one rounding
 * per operation: e1 = B - A, e2 = C - A, n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x),
 * len = sqrtf((n.x n.x + n.y n.y) + n.z n.z), IEEE division; no guards (a zero-area triangle stores what 0 / 0 gives; no ray
 * test hits it).  No other word of a record (3, 7, 8..11 of each corner, 36..39) and no other record is written
 * (csrc/rt_deform.h is the definition; csrc/rt_deform.hip stores only the words named).
 * The contract is rt_update_triangles': a scene-setup call, synchronous; it waits for the frames in flight, synchronises
 * hip_stream before it reads the caller's arrays, runs on the context's stream behind the scene-update event and records that
 * event, so frames and queries on any stream see the new records; on return the caller's arrays are free.  It changes no node and
 * no lookup slot -- follow it with rt_refit_blas (a cached refit plan stays valid, the pair records are not marked stale) and,
 * for a tight top level, rt_build_tlas.  The library's corner array follows by itself.
 * Checks, in this order: a NULL context, unknown flag bits, or RT_DEFORM_FLAT_NORMALS together with normals: RT_ERR_INVALID_ARG;
 * no triangle scene (a sphere scene too): RT_ERR_STATE; first + n (taken in 64 bits) beyond the triangles written:
 * RT_ERR_INVALID_ARG, nothing changed; n == 0: RT_OK; NULL vertices, V == 0, no faces and V < 3 n (in 64 bits), or -- the
 * device form -- a pointer that is not 4-byte aligned: RT_ERR_INVALID_ARG.
 *
 * rt_deform_triangles_host: the same with the arrays in HOST memory, staged through a buffer the context owns.
 * rt_deform_triangles_model: the same arithmetic, serially, on caller arrays (triangles: n_triangles records of 40 floats, changed
 * in place), with no device and no context; the same checks, RT_ERR_STATE when `triangles` is NULL or empty.
 * rt_update_triangles_device: rt_update_triangles with the records in DEVICE memory (4-byte aligned), produced on hip_stream. */
int rt_deform_triangles(rt_ctx* ctx, uint32_t first, uint32_t n, const float* vertices /* dev [V][3] */, uint32_t V,
                        const uint32_t* faces /* dev [n][3] or NULL */, const float* normals /* dev [V][3] or NULL */,
                        uint32_t flags, void* hip_stream);
int rt_deform_triangles_host(rt_ctx* ctx, uint32_t first, uint32_t n, const float* vertices /* host [V][3] */, uint32_t V,
                             const uint32_t* faces /* host [n][3] or NULL */, const float* normals /* host [V][3] or NULL */,
                             uint32_t flags);
int rt_deform_triangles_model(float* triangles, uint32_t n_triangles, uint32_t first, uint32_t n, const float* vertices, uint32_t V,
                              const uint32_t* faces, const float* normals, uint32_t flags);
int rt_update_triangles_device(rt_ctx* ctx, uint32_t first, uint32_t n, const float* records_dev, void* hip_stream);

/* Diagnostic: rt_read_nodes for the triangle records -- `n` records (40 f32 each) starting at record `first`, as the next frame
 * would read them.  Waits for the frames in flight.  first + n beyond the triangles written: RT_ERR_INVALID_ARG. */
int rt_read_triangles(rt_ctx* ctx, uint32_t first, uint32_t n, float* dst);

/* ---- device BLAS builds: the builder's SAH tree of a mesh, made on the device ------------------------------------------------------ */

typedef struct rt_blas_range {
    uint32_t root_node;   /* node index of the tree's root (a BLAS record's rootNodeIndex)                */
    uint32_t node_cap;    /* nodes [root_node, root_node + node_cap) are this tree's to use               */
    uint32_t first_slot;  /* the tree's triangles: u32(triangleLookup[first_slot .. first_slot+n_slots)) */
    uint32_t n_slots;
} rt_blas_range;

/* rt_build_blas: for each range, the tree the project's host builder (the reference's bvh.ts: SAH over nine planes per axis at
 * tenths of the node's extent) makes of the triangles the range's lookup slots name, from the float32 corners the device holds
 * (indices clamped to the triangles written).  The root goes to root_node, child pairs are numbered depth-first, the left subtree
 * first, from root_node + 1; word 3 is the child index or a leaf's first slot, word 7 the count; boxes are the exact float32
 * min / max.  The range's lookup slots are permuted so that every leaf owns a contiguous run; inside a leaf the slots keep the
 * relative order they had before the call, so a second build of unchanged triangles changes no byte.  used[i] (when not NULL) is
 * the tree's node count; nodes [root_node + used, root_node + node_cap) are not touched.  2 * n_slots - 1 nodes always suffice.
 * Checks, in this order: a NULL context, or NULL ranges with n != 0: RT_ERR_INVALID_ARG; no triangle scene (triangles, nodes and
 * lookup written): RT_ERR_STATE; n == 0: RT_OK; a range with n_slots == 0 or node_cap == 0, beyond the nodes or slots written
 * (sums in 64 bits), covering node 0, or overlapping another in nodes or in slots: RT_ERR_INVALID_ARG, nothing changed; a tree
 * that needs more than node_cap nodes: RT_ERR_CAPACITY -- used[] is set for every range, and nothing of the scene has changed.
 * Non-finite corners: the call ends, is memory-safe and leaves every slot in exactly one leaf of a well-formed tree; no shape is
 * promised.  Synchronous, and a scene-setup call: waits for the frames in flight.  Afterwards every version of the node buffer,
 * the library's mirror and the head copy that frames carry hold the new records, the relinked pair records are stale -- the next
 * frame rebuilds them (rt_stats.pair_rebuilds) --, and the corner array and any refit plan are remade when next needed. */
int rt_build_blas(rt_ctx* ctx, const rt_blas_range* ranges, uint32_t n, uint32_t* used /* [n], may be NULL */);

/* Diagnostic: rt_read_nodes for the triangle lookup table -- `n` words starting at slot `first_slot`.  Waits for the frames in
 * flight.  first_slot + n beyond the slots written: RT_ERR_INVALID_ARG. */
int rt_read_tri_lookup(rt_ctx* ctx, uint32_t first_slot, uint32_t n, float* dst);

/* Runs rt_build_blas' algorithm on caller arrays in place, serially, with no device and no context: the same inline arithmetic
 * as the kernels (csrc/rt_blas_build.h), the same checks and results.  triangles: 40 floats each; nodes: 8 floats each.
 * RT_ERR_STATE when an array is NULL or empty. */
int rt_build_blas_host(const float* triangles, uint32_t n_triangles, float* tri_lookup, uint32_t n_tri_lookup,
                       float* nodes, uint32_t n_nodes, const rt_blas_range* ranges, uint32_t n, uint32_t* used);

/* ---- device top-level builds: a SAH tree over the instances' tight world boxes ------------------------------------------------------ */

typedef struct rt_tlas_info {
    uint32_t nodes_used;  /* nodes of the tree                        */
    uint32_t depth;       /* levels below the root                    */
    uint32_t leaves;
    uint32_t max_leaf;    /* most instances in one leaf               */
} rt_tlas_info;

/* rt_build_tlas: the whole per-frame instance state -- BLAS records, BLAS lookup, top-level nodes -- made on the device from the
 * instances' FORWARD matrices and the boxes the device holds at their roots.  models: n x 16 floats, column-major; roots: the root
 * node index of each instance's bottom-level tree; nodes [0, node_cap) of the node buffer are the top level's.
 *   BLAS record i = {invert(models[i]), (float)roots[i], 0, 0, 0}, in the caller's instance order (rt_write_instance_masks tables
 *     and rt_hit.instance keep their meaning).  invert is gl-matrix's mat4.invert: float64 minors and cofactors of the float32
 *     entries, each times 1 / det, one rounding to float32; det == 0: the identity.
 *   World box of instance i: the eight corners of the node record at roots[i] (min.xyz, max.xyz as the device holds them NOW, so
 *     after any refit or rebuild) through models[i] as vec3.transformMat4 does it (float64 products and sums left to right,
 *     w || 1, the division, one rounding to float32), min / max from -+1e30; then padded: with m the largest absolute value of the
 *     six bounds and pad = m * 2^-16 (float32), lo - pad and hi + pad.  Centroid (lo + hi) * 0.5f of the padded bounds.
 *   Tree: rt_build_blas' SAH rules over these boxes (27 planes, first strict minimum, the leaf rule, a stable partition, the
 *     children of the split of preorder rank k at 1 + 2k); the root is node 0, a leaf's word 3 is a position in the BLAS lookup,
 *     whose words are the instance indices in leaf order.  Nodes [nodes_used, node_cap) are zero records.
 * On success the context is in exactly the state the same bytes passed to rt_write_blas, rt_write_blas_lookup and
 * rt_write_nodes(ctx, 0, ..., node_cap) leave it in (up to sixteen instances travel with the frames, as after those calls).
 * Synchronous, and a scene-setup call: waits for the frames in flight.  *info (may be NULL) describes the tree.
 * Checks, in this order, nothing changed by any of them: a NULL context, models or roots (or models_dev not 16-byte aligned):
 * RT_ERR_INVALID_ARG; no triangle scene (no nodes written): RT_ERR_STATE; n == 0, n > 2^20, node_cap beyond the nodes written, a
 * root at or beyond the nodes written or below node_cap: RT_ERR_INVALID_ARG; a tree of more than node_cap nodes: RT_ERR_CAPACITY
 * -- info->nodes_used is the need, 2n - 1 always suffice --; a tree deeper than 20 levels: RT_ERR_UNSUPPORTED (the kernels keep
 * twenty stack slots, and walking the nearer child first needs one per level); *info is set in both.  Non-finite matrix entries
 * or boxes: the call ends and is memory-safe; no shape is promised.
 *
 * TWO THINGS DIFFER from the top level the reference's recipe makes (placeholder boxes of -+999999 per mesh, which cover every
 * ray): (1) these boxes are tight, so after anything that GROWS a root box -- rt_update_triangles + rt_refit_blas, rt_build_blas,
 * a node write -- the top level must be built again, or hits can be lost; (2) where two instances are hit at exactly the same t,
 * the winning (instance, prim) may differ from the placeholder tree's, since the instances are visited in another order.  t never
 * differs.
 * Cost: one device-to-host word per level of the tree plus the read-back of the result (148 bytes per instance); for a handful of
 * instances the host recipe is faster (DESIGN.md 4.7i has the figures) -- this call is for scenes of many instances, and for boxes
 * that exist only on the device.
 *
 * rt_build_tlas_device: the same with the matrices in DEVICE memory (16-byte aligned), produced on `hip_stream` (NULL: the
 * context's stream); the call waits for that stream.  roots and info stay host memory. */
int rt_build_tlas(rt_ctx* ctx, const float* models /* host [n][16] */, const uint32_t* roots /* host [n] */, uint32_t n,
                  uint32_t node_cap, rt_tlas_info* info /* may be NULL */);
int rt_build_tlas_device(rt_ctx* ctx, const float* models_dev, const uint32_t* roots, uint32_t n, uint32_t node_cap,
                         rt_tlas_info* info, void* hip_stream);

/* Runs rt_build_tlas' algorithm on caller arrays, serially, with no device and no context: the same inline arithmetic as the
 * kernels (csrc/rt_tlas_build.h), the same checks and results.  nodes: the node buffer the roots index, n_nodes records of 8
 * floats.  Out: tlas_nodes [node_cap][8] (zero records behind the tree), blas [n][20], blas_lookup [n]; written only on RT_OK.  A
 * NULL array: RT_ERR_INVALID_ARG. */
int rt_build_tlas_host(const float* models, const uint32_t* roots, uint32_t n, const float* nodes, uint32_t n_nodes,
                       float* tlas_nodes, float* blas, float* blas_lookup, uint32_t node_cap, rt_tlas_info* info);

/* Diagnostics: rt_read_nodes for the BLAS records (20 f32 each) and the BLAS lookup words -- what the next frame would read, the
 * copies that travel with the frames included.  Wait for the frames in flight.  first + n beyond what was written:
 * RT_ERR_INVALID_ARG. */
int rt_read_blas(rt_ctx* ctx, uint32_t first, uint32_t n, float* dst);
int rt_read_blas_lookup(rt_ctx* ctx, uint32_t first, uint32_t n, float* dst);

/* Which filter forms a frame of this scene may use (no device needed): *filter_ok = 0 when
 * max(|center| + |radius| over the spheres, |cameraPos|, |lightPosition|) is NaN, infinite or
 * >= 2^20 -- fast mode then renders the frame with the literal kernel --, *signed_filter = 1 when
 * that reach is below 342 and no sphere has a radius in (0, 2^-30) (the sign-aware filter and hierarchy
 * walk; the walk's rescaled node test needs the second condition).  A NaN in ANY record, whatever its
 * position, switches both off. */
int rt_filter_plan(const float* records, uint32_t n, const float params[24], int* filter_ok, int* signed_filter);

#ifdef __cplusplus
}
#endif
#endif /* RT355_H */
