// rt_blas_build.h -- the arithmetic and the serial model behind rt_build_blas / rt_build_blas_host -- under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_build_blas_sanitizers_cpu.py).  Inputs: random soups of builder sizes (1 .. 3,000
// triangles, one and two ranges in one call, lookup words that name triangles beyond the buffer), grids and duplicates (ties,
// leaves of many), every bad range of the contract, a tree one node short of its capacity, and garbage floats (NaN, infinities,
// huge and denormal corners and lookup words).  Checked: no bad access or UB (the sanitizers), the documented status, a refusal
// leaves the arrays alone, and on every accepted call: each tree's nodes are exactly [root, root + used), every slot of the range
// lies in exactly one leaf, the lookup words are a permutation of what they were, and a second call changes no byte.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../compute_raytracer_amd/csrc/rt_blas_build.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

struct Scene { std::vector<float> tri, lookup, nodes; };

static Scene soup(uint32_t n_tri, uint32_t n_nodes, std::mt19937& gen, int kind) {
    std::uniform_real_distribution<float> at(-4.0f, 4.0f), d(-0.6f, 0.6f);
    Scene s;
    s.tri.assign(40u * (size_t)n_tri, 0.25f);
    for (uint32_t t = 0; t < n_tri; ++t) {
        float c[3] = {at(gen), at(gen), at(gen)};
        if (kind == 1) { c[0] = (float)(t % 12u); c[1] = 0.0f; c[2] = (float)(t / 12u); }          // a flat grid: ties on y
        if (kind == 2) { c[0] = c[1] = c[2] = 1.0f; }                                             // duplicates
        for (uint32_t k = 0; k < 3u; ++k)
            for (uint32_t a = 0; a < 3u; ++a)
                s.tri[40u * (size_t)t + 12u * k + a] = c[a] + (kind == 0 ? d(gen) : (kind == 1 && a != 1u ? (float)((k + a) % 2u) : 0.0f));
    }
    s.lookup.resize(n_tri);
    for (uint32_t t = 0; t < n_tri; ++t) s.lookup[t] = (float)t;
    s.nodes.assign(8u * (size_t)n_nodes, -7.5f);
    return s;
}

// the promises of an accepted call, for one range
static void check_tree(const Scene& s, const Scene& before, const rt_blas_range& g, uint32_t used) {
    const uint32_t n_nodes = (uint32_t)(s.nodes.size() / 8u);
    CHECK(used >= 1u && used <= g.node_cap && used <= 2u * g.n_slots - 1u, "used %u of %u", used, g.node_cap);
    std::vector<uint8_t> seen(n_nodes, 0), cover(g.n_slots, 0);
    std::vector<uint32_t> todo(1, g.root_node);
    uint32_t reached = 0;
    while (!todo.empty()) {
        const uint32_t i = todo.back(); todo.pop_back();
        if (i < g.root_node || i >= g.root_node + used || seen[i]) { CHECK(false, "node %u outside the tree or reached twice", i); return; }
        seen[i] = 1; ++reached;
        const float* p = &s.nodes[8u * (size_t)i];
        const uint32_t left = rt_bb_u32f(p[3]), count = rt_bb_u32f(p[7]);
        if (count == 0u) { todo.push_back(left + 1u); todo.push_back(left); continue; }
        if (left < g.first_slot || (uint64_t)left + count > (uint64_t)g.first_slot + g.n_slots) { CHECK(false, "leaf run of node %u", i); return; }
        for (uint32_t k = 0; k < count; ++k) ++cover[left - g.first_slot + k];
    }
    CHECK(reached == used, "%u nodes reached, used %u", reached, used);
    for (uint32_t k = 0; k < g.n_slots; ++k) if (cover[k] != 1u) { CHECK(false, "slot %u in %u leaves", g.first_slot + k, cover[k]); break; }
    std::vector<uint32_t> a(g.n_slots), b(g.n_slots);
    std::memcpy(a.data(), &s.lookup[g.first_slot], 4u * (size_t)g.n_slots);
    std::memcpy(b.data(), &before.lookup[g.first_slot], 4u * (size_t)g.n_slots);
    std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
    CHECK(a == b, "the lookup words of the range are not a permutation of what they were");
    for (uint32_t i = g.root_node + used; i < g.root_node + g.node_cap; ++i)
        if (std::memcmp(&s.nodes[8u * (size_t)i], &before.nodes[8u * (size_t)i], 32) != 0) { CHECK(false, "node %u beyond used was touched", i); break; }
}

static int build(Scene& s, const std::vector<rt_blas_range>& r, std::vector<uint32_t>& used) {
    const char* why = nullptr;
    used.assign(r.size() + 1u, 0xFFFFFFFFu);
    return rt_bb_build_host(s.tri.data(), (uint32_t)(s.tri.size() / 40u), s.lookup.data(), (uint32_t)s.lookup.size(), s.nodes.data(),
                            (uint32_t)(s.nodes.size() / 8u), r.data(), (uint32_t)r.size(), used.data(), &why);
}
static bool same(const Scene& a, const Scene& b) {
    return std::memcmp(a.lookup.data(), b.lookup.data(), 4u * a.lookup.size()) == 0 && std::memcmp(a.nodes.data(), b.nodes.data(), 4u * a.nodes.size()) == 0;
}

int main() {
    std::mt19937 gen(355);
    std::vector<uint32_t> used;
    // builder-sized inputs: one range, then two in one call
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t n : {1u, 2u, 3u, 65u, 257u, 3000u}) {
            Scene s = soup(n, 2u * n + 4u, gen, kind);
            if (n > 3u) { s.lookup[1] = 1e9f; s.lookup[2] = NAN; s.lookup[3] = -1.0f; }        // clamped, as tri_corners clamps
            const Scene before = s;
            const uint32_t half = n / 2u;
            std::vector<rt_blas_range> r;
            if (half == 0u) r = {{3u, 2u * n - 1u, 0u, n}};
            else r = {{3u + 2u * half, 2u * (n - half) - 1u, half, n - half}, {2u, 2u * half - 1u, 0u, half}};
            int rc = build(s, r, used);
            CHECK(rc == RT_OK, "kind %d, %u triangles: %d", kind, n, rc);
            for (size_t i = 0; i < r.size(); ++i) check_tree(s, before, r[i], used[i]);
            if (kind == 2 && half == 0u) CHECK(used[0] == 1u, "duplicates: one leaf");
            const Scene once = s;
            std::vector<uint32_t> again;
            rc = build(s, r, again);
            CHECK(rc == RT_OK && same(s, once) && again == used, "a second build changed a byte");
            // one node short: capacity, used[] set, nothing stored
            if (used[0] > 1u) {
                Scene t = before;
                std::vector<rt_blas_range> q = r;
                q[0].node_cap = used[0] - 1u;
                rc = build(t, q, again);
                CHECK(rc == RT_ERR_CAPACITY && same(t, before) && again == used, "capacity: %d", rc);
            }
        }
    // the bad ranges
    {
        Scene s = soup(50u, 120u, gen, 0);
        const Scene before = s;
        const std::vector<std::vector<rt_blas_range>> bad = {
            {{1u, 99u, 0u, 0u}}, {{1u, 0u, 0u, 50u}}, {{0u, 99u, 0u, 50u}}, {{30u, 91u, 0u, 50u}}, {{0xFFFFFFFFu, 2u, 0u, 50u}},
            {{1u, 99u, 49u, 2u}}, {{1u, 99u, 0xFFFFFFFFu, 2u}}, {{1u, 60u, 0u, 25u}, {60u, 60u, 25u, 25u}}, {{1u, 49u, 0u, 26u}, {50u, 49u, 25u, 25u}},
            {{1u, 49u, 0u, 25u}, {1u, 49u, 0u, 25u}}};
        for (size_t k = 0; k < bad.size(); ++k) {
            const int rc = build(s, bad[k], used);
            CHECK(rc == RT_ERR_INVALID_ARG && same(s, before), "bad range %zu: %d", k, rc);
        }
        const char* why = nullptr;
        CHECK(rt_bb_build_host(s.tri.data(), 50u, s.lookup.data(), 50u, s.nodes.data(), 120u, nullptr, 1u, nullptr, &why) == RT_ERR_INVALID_ARG, "NULL ranges");
        CHECK(rt_bb_build_host(nullptr, 0u, s.lookup.data(), 50u, s.nodes.data(), 120u, bad[0].data(), 1u, nullptr, &why) == RT_ERR_STATE, "no triangles");
        CHECK(rt_bb_build_host(s.tri.data(), 50u, s.lookup.data(), 50u, s.nodes.data(), 120u, nullptr, 0u, nullptr, &why) == RT_OK, "no ranges");
        CHECK(same(s, before), "the argument checks changed a byte");
    }
    // garbage floats
    {
        const float odd[] = {NAN, INFINITY, -INFINITY, -1.0f, 0.0f, -0.0f, 3.0e38f, -3.0e38f, 1e30f, -1e30f, 1e-40f, 4294967296.0f,
                             std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max()};
        const uint32_t n_odd = (uint32_t)(sizeof odd / sizeof odd[0]);
        for (int it = 0; it < 300; ++it) {
            const uint32_t n = 1u + gen() % 90u;
            Scene s = soup(n, 2u * n + 1u, gen, 0);
            for (float& f : s.tri) if (gen() % (1u + it % 7u) == 0u) f = odd[gen() % n_odd];
            for (float& f : s.lookup) if (gen() % 5u == 0u) f = odd[gen() % n_odd];
            const Scene before = s;
            const std::vector<rt_blas_range> r = {{1u, 2u * n - 1u, 0u, n}};
            const int rc = build(s, r, used);
            CHECK(rc == RT_OK, "garbage: %d", rc);
            if (rc == RT_OK) check_tree(s, before, r[0], used[0]);
        }
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("blas build ok\n");
    return 0;
}
