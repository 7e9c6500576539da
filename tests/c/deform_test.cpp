// rt_deform.h -- the arithmetic and the serial model behind rt_deform_triangles / rt_deform_triangles_model -- under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_deform_sanitizers_cpu.py).  Every array is allocated at exactly the
// size the call may read or write (the heap redzones catch a word beyond it): soups and indexed meshes, face indices beyond V
// (0xFFFFFFFF among them), V == 1, ranges at the first and at the last record, NaN / infinite / zero-area input, and the call
// shape.  Checked besides: the words the call may write hold what a second, literal statement of the rule gives, and every other
// word of every record keeps its bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../compute_raytracer_amd/csrc/rt_deform.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static uint32_t word(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return word(a) == word(b) || (std::isnan(a) && std::isnan(b)); }

static float special(std::mt19937& gen, float plain) {
    switch (gen() % 16u) {
        case 0: return std::numeric_limits<float>::quiet_NaN();
        case 1: return std::numeric_limits<float>::infinity();
        case 2: return -std::numeric_limits<float>::infinity();
        case 3: return 0.0f;
        case 4: return 3.0e38f;
        case 5: return 1.0e-42f;
        default: return plain;
    }
}

// one call on fresh arrays of exactly the sizes named
static void run(std::mt19937& gen, uint32_t n_tri, uint32_t first, uint32_t n, uint32_t V, bool use_faces, int mode, bool wild) {
    std::uniform_real_distribution<float> u(-4.0f, 4.0f);
    std::vector<float> tri((size_t)n_tri * 40u), before;
    for (float& x : tri) x = u(gen);
    before = tri;
    std::vector<float> vertices((size_t)V * 3u), normals;
    for (float& x : vertices) x = wild ? special(gen, u(gen)) : u(gen);
    if (mode == 1) { normals.resize((size_t)V * 3u); for (float& x : normals) x = wild ? special(gen, u(gen)) : u(gen); }
    std::vector<uint32_t> faces;
    if (use_faces) {
        faces.resize((size_t)n * 3u);
        for (uint32_t& k : faces) {
            const uint32_t r = gen() % 8u;
            k = r == 0u ? 0xFFFFFFFFu : r == 1u ? V : r == 2u ? V + gen() % 100u : gen() % V;
        }
        if (n > 1u) faces[3] = faces[4] = faces[5] = gen() % V;                  // one vertex three times: zero area
    } else if (n > 1u) {
        for (int k = 0; k < 3; ++k) vertices[3 + k] = vertices[k];               // corners A and B of triangle 0 coincide
    }
    const uint32_t flags = mode == 2 ? RT_DEFORM_FLAT_NORMALS : 0u;
    const char* why = "";
    const int rc = rt_df_model(tri.data(), n_tri, first, n, vertices.data(), V, use_faces ? faces.data() : nullptr,
                               mode == 1 ? normals.data() : nullptr, flags, &why);
    CHECK(rc == RT_OK, "status %d (%s)", rc, why);
    if (rc != RT_OK) return;
    for (uint32_t t = 0; t < n_tri; ++t) {
        const bool in = t >= first && t - first < n;
        const uint32_t i = t - first;
        float p[9] = {0}, nrm[3] = {0};
        uint32_t k[3] = {0, 0, 0};
        if (in) {
            for (uint32_t c = 0; c < 3u; ++c) {
                k[c] = use_faces ? std::min(faces[3u * i + c], V - 1u) : 3u * i + c;
                for (uint32_t j = 0; j < 3u; ++j) p[3u * c + j] = vertices[3u * k[c] + j];
            }
            // the flat normal again, every operation through a volatile float: one rounding each, whatever the compiler would like
            volatile float e1[3], e2[3], cr[3], sq[3], s;
            for (int j = 0; j < 3; ++j) { e1[j] = p[3 + j] - p[j]; e2[j] = p[6 + j] - p[j]; }
            for (int j = 0; j < 3; ++j) {
                const int a = (j + 1) % 3, b = (j + 2) % 3;
                volatile float l = e1[a] * e2[b], r = e1[b] * e2[a];
                cr[j] = l - r;
            }
            for (int j = 0; j < 3; ++j) sq[j] = cr[j] * cr[j];
            s = sq[0] + sq[1]; s = s + sq[2];
            const float len = std::sqrt((float)s);
            for (int j = 0; j < 3; ++j) nrm[j] = cr[j] / len;
        }
        for (uint32_t w = 0; w < 40u; ++w) {
            const uint32_t c = w / 12u, j = w % 12u;
            const float got = tri[40u * (size_t)t + w], was = before[40u * (size_t)t + w];
            if (in && w < 36u && j < 3u) CHECK(word(got) == word(p[3u * c + j]), "triangle %u word %u: position", t, w);
            else if (in && w < 36u && j >= 4u && j < 7u && mode == 1) CHECK(word(got) == word(normals[3u * k[c] + (j - 4u)]), "triangle %u word %u: normal", t, w);
            else if (in && w < 36u && j >= 4u && j < 7u && mode == 2) CHECK(same(got, nrm[j - 4u]), "triangle %u word %u: flat normal %g, want %g", t, w, got, nrm[j - 4u]);
            else CHECK(word(got) == word(was), "triangle %u word %u was written", t, w);
        }
    }
}

static void call_shape() {
    std::vector<float> tri(40u * 4u, 1.0f), v(9, 0.0f), nr(9, 0.0f);
    std::vector<uint32_t> f(3, 0u);
    const char* why = "";
    const int inv = RT_ERR_INVALID_ARG, st = RT_ERR_STATE;
    CHECK(rt_df_model(nullptr, 0, 9, 9, nullptr, 0, nullptr, nullptr, 2u, &why) == inv, "unknown flags come first");
    CHECK(rt_df_model(nullptr, 0, 9, 9, nullptr, 0, nullptr, nr.data(), RT_DEFORM_FLAT_NORMALS, &why) == inv, "flat with normals");
    CHECK(rt_df_model(nullptr, 4, 9, 9, nullptr, 0, nullptr, nullptr, 0u, &why) == st, "NULL triangles");
    CHECK(rt_df_model(tri.data(), 0, 9, 9, nullptr, 0, nullptr, nullptr, 0u, &why) == st, "no triangles");
    CHECK(rt_df_model(tri.data(), 4, 4, 1, nullptr, 0, nullptr, nullptr, 0u, &why) == inv, "range");
    CHECK(rt_df_model(tri.data(), 4, 0xFFFFFFFFu, 2, nullptr, 0, nullptr, nullptr, 0u, &why) == inv, "range in 64 bits");
    CHECK(rt_df_model(tri.data(), 4, 5, 0, nullptr, 0, nullptr, nullptr, 0u, &why) == inv, "range before n == 0");
    CHECK(rt_df_model(tri.data(), 4, 4, 0, nullptr, 0, nullptr, nullptr, 0u, &why) == RT_OK, "n == 0");
    CHECK(rt_df_model(tri.data(), 4, 3, 1, nullptr, 3, nullptr, nullptr, 0u, &why) == inv, "NULL vertices");
    CHECK(rt_df_model(tri.data(), 4, 3, 1, v.data(), 0, f.data(), nullptr, 0u, &why) == inv, "V == 0");
    CHECK(rt_df_model(tri.data(), 4, 3, 1, v.data(), 2, nullptr, nullptr, 0u, &why) == inv, "V < 3 n");
    CHECK(rt_df_model(tri.data(), 4, 3, 1, v.data(), 3, nullptr, nullptr, 0u, &why) == RT_OK, "the last record");
    for (size_t w = 0; w < 120u; ++w) CHECK(tri[w] == 1.0f, "word %zu written by a refused or foreign call", w);
}

int main() {
    std::mt19937 gen(20240611u);
    call_shape();
    const uint32_t ns[] = {1u, 2u, 64u, 65u, 257u};
    for (uint32_t n : ns)
        for (int faces = 0; faces < 2; ++faces)
            for (int mode = 0; mode < 3; ++mode)
                for (int wild = 0; wild < 2; ++wild) {
                    const uint32_t V = faces ? n / 2u + 3u : 3u * n;
                    run(gen, n, 0u, n, V, faces != 0, mode, wild != 0);                       // the whole buffer
                    run(gen, n + 7u, 7u, n, V, faces != 0, mode, wild != 0);                  // ending at the last record
                    run(gen, n + 9u, 4u, n, faces ? V : V + 5u, faces != 0, mode, wild != 0);   // in the middle
                }
    for (int mode = 0; mode < 3; ++mode) run(gen, 12u, 3u, 6u, 1u, true, mode, false);        // V == 1: every index clamps to 0
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("deform ok\n");
    return 0;
}
