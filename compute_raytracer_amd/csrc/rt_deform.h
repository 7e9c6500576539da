// rt_deform.h -- device mesh deformation (include/rt355.h: rt_deform_triangles) as plain float32 arithmetic: what a deformed
// triangle record is, written once for the kernel (rt_deform.hip) and for the serial model (rt_deform_triangles_model), which
// differ only in where the arrays live.  No HIP needed: tests/c/deform_test.cpp compiles it with g++ under ASan + UBSan
// (tests/test_deform_sanitizers_cpu.py).  Everything must be compiled without FMA contraction (-ffp-contract=off).
//
// THIS HEADER IS THE DEFINITION of a deformed record.  For triangle i of the call (record first + i), corner c in {0, 1, 2}:
//   * vertex index: k = faces ? min(faces[3 i + c], V - 1) : 3 i + c (the library's clamp for indices it cannot check on the
//     device; without faces the call has checked V >= 3 n);
//   * position: words 12 c + 0 .. 2 of the record become vertices[3 k + 0 .. 2], copied bit for bit (NaN and inf as they are);
//   * normals from the caller: words 12 c + 4 .. 6 become normals[3 k + 0 .. 2], copied bit for bit;
//   * flat normals (RT_DEFORM_FLAT_NORMALS): all three corners get n / len from the new positions A, B, C in float32, one rounding
//     per operation: e1 = B - A, e2 = C - A, n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x),
//     len = sqrtf((n.x n.x + n.y n.y) + n.z n.z), each word n.k / len by IEEE division -- the oracle's normalize.  No guards: a
//     zero-area triangle stores what 0 / 0 gives (no ray test ever hits it);
//   * every other word of the record (3, 7, 8 .. 11 of each corner, 36 .. 39) and every other record: not written, and nothing of
//     the record is read.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/rt355.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_DF_HD __host__ __device__
#else
#define RT_DF_HD
#endif

constexpr uint32_t kDfRecordWords = 40u, kDfCornerWords = 12u;

struct RtDeformArgs {
    float* tri;                 // the triangle buffer: n_tri records of 40 floats
    uint32_t n_tri;
    uint32_t first, n;          // records [first, first + n) -- inside the buffer, checked by the caller
    const float* vertices;      // [V][3]
    uint32_t V;                 // >= 1; >= 3 n without faces
    const uint32_t* faces;      // [n][3] or null
    const float* normals;       // [V][3] or null
    uint32_t flags;             // RT_DEFORM_*
};

RT_DF_HD inline uint32_t rt_df_vertex(const RtDeformArgs& a, uint32_t i, uint32_t c) {
    if (!a.faces) return 3u * i + c;
    const uint32_t k = a.faces[3u * (size_t)i + c];
    return k < a.V ? k : a.V - 1u;
}

// p: the corners A, B, C (9 floats); out: the unit normal of the plane through them
RT_DF_HD inline void rt_df_flat_normal(const float* p, float* out) {
    const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    out[0] = nx / len; out[1] = ny / len; out[2] = nz / len;
}

// triangle i of the call: partial writes into record first + i
RT_DF_HD inline void rt_df_triangle(const RtDeformArgs& a, uint32_t i) {
    float* rec = a.tri + kDfRecordWords * (size_t)(a.first + i);
    uint32_t k[3];
    float p[9];
    for (uint32_t c = 0; c < 3u; ++c) {
        k[c] = rt_df_vertex(a, i, c);
        const float* v = a.vertices + 3u * (size_t)k[c];
        p[3u * c] = v[0]; p[3u * c + 1u] = v[1]; p[3u * c + 2u] = v[2];
    }
    for (uint32_t c = 0; c < 3u; ++c) {
        float* w = rec + kDfCornerWords * c;
        w[0] = p[3u * c]; w[1] = p[3u * c + 1u]; w[2] = p[3u * c + 2u];
    }
    if (a.normals) {
        for (uint32_t c = 0; c < 3u; ++c) {
            const float* q = a.normals + 3u * (size_t)k[c];
            float* w = rec + kDfCornerWords * c + 4u;
            w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
        }
    } else if (a.flags & RT_DEFORM_FLAT_NORMALS) {
        float nrm[3];
        rt_df_flat_normal(p, nrm);
        for (uint32_t c = 0; c < 3u; ++c) {
            float* w = rec + kDfCornerWords * c + 4u;
            w[0] = nrm[0]; w[1] = nrm[1]; w[2] = nrm[2];
        }
    }
}

// ---- the call shape, shared by the context entry points and the model (the checks of include/rt355.h, in its order) ----------

// before the scene is looked at; null: fine
inline const char* rt_df_check_flags(const float* normals, uint32_t flags) {
    if (flags & ~RT_DEFORM_FLAT_NORMALS) return "unknown flag bits";
    if ((flags & RT_DEFORM_FLAT_NORMALS) && normals) return "RT_DEFORM_FLAT_NORMALS together with normals";
    return nullptr;
}
inline bool rt_df_in_range(uint32_t first, uint32_t n, uint64_t n_written) { return (uint64_t)first + n <= n_written; }
// for n != 0, after the range; null: fine
inline const char* rt_df_check_arrays(uint32_t n, const float* vertices, uint32_t V, const uint32_t* faces) {
    if (!vertices) return "vertices is NULL";
    if (V == 0u) return "V is 0";
    if (!faces && (uint64_t)V < 3u * (uint64_t)n) return "without faces V must be at least 3 n";
    return nullptr;
}

// ---- the model: the whole call on caller arrays, serially (rt_deform_triangles_model) -----------------------------------------
inline int rt_df_model(float* triangles, uint32_t n_triangles, uint32_t first, uint32_t n, const float* vertices, uint32_t V,
                       const uint32_t* faces, const float* normals, uint32_t flags, const char** why) {
    *why = "";
    if (const char* bad = rt_df_check_flags(normals, flags)) { *why = bad; return RT_ERR_INVALID_ARG; }
    if (!triangles || !n_triangles) { *why = "no triangles"; return RT_ERR_STATE; }
    if (!rt_df_in_range(first, n, n_triangles)) { *why = "first + n is beyond the triangles"; return RT_ERR_INVALID_ARG; }
    if (n == 0u) return RT_OK;
    if (const char* bad = rt_df_check_arrays(n, vertices, V, faces)) { *why = bad; return RT_ERR_INVALID_ARG; }
    RtDeformArgs a;
    a.tri = triangles; a.n_tri = n_triangles; a.first = first; a.n = n;
    a.vertices = vertices; a.V = V; a.faces = faces; a.normals = normals; a.flags = flags;
    for (uint32_t i = 0; i < n; ++i) rt_df_triangle(a, i);
    return RT_OK;
}

#if defined(__HIPCC__)
// The launch lives in rt_deform.o.  rt_api.hip reaches it through this pointer, which rt_deform.o sets while the library is loaded
// (null until then), as it reaches the closest-point launch (rt_tri_types.h: rt_closest_launch): rt_api.o names no symbol of
// rt_deform.o, so a host-only program that links rt_api.o for the frame path alone needs no stand-in for a launch no frame makes.
// A null pointer at a call is an error, never a silent miss.
typedef hipError_t (*RtDeformLaunch)(const RtDeformArgs&, hipStream_t);
extern RtDeformLaunch rt_deform_launch;
#endif
