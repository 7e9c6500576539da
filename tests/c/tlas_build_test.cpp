// rt_tlas_build.h -- the arithmetic and the serial model behind rt_build_tlas / rt_build_tlas_host -- under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_build_tlas_sanitizers_cpu.py).  Inputs: random instance sets of 1 .. 3,000 instances
// (rotations, scales, translations, some projective rows), coincident instances (one leaf of all), singular matrices, a spine
// deeper than twenty levels, every bad argument of the contract, a capacity one node short, and garbage floats (NaN, infinities,
// huge and denormal matrix entries and root boxes).  Checked: no bad access or UB (the sanitizers), the documented status, a
// refusal leaves the outputs alone, and on every accepted call: the tree's nodes are exactly [0, nodes_used), every instance lies
// in exactly one leaf, the lookup words are a permutation of 0 .. n - 1, the records carry the roots, the nodes behind the tree
// are zero records, info describes the tree, and a second call gives the same bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../compute_raytracer_amd/csrc/rt_tlas_build.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

struct Call {
    std::vector<float> models, nodes;
    std::vector<uint32_t> roots;
    uint32_t node_cap;
};
struct Out {
    std::vector<float> tlas, blas, lookup;
    rt_tlas_info info;
};
static const float kSentinel = -7.5f;

static Call instances(uint32_t n, std::mt19937& gen, int kind) {
    std::uniform_real_distribution<float> at(-12.0f, 12.0f), u(-1.0f, 1.0f), sc(0.3f, 2.5f);
    const uint32_t kinds = 5u;
    Call c;
    c.node_cap = 2u * n - 1u;
    c.nodes.assign(8u * (size_t)(c.node_cap + kinds), 0.0f);
    for (uint32_t k = 0; k < kinds; ++k) {
        float* p = &c.nodes[8u * (size_t)(c.node_cap + k)];
        for (int a = 0; a < 3; ++a) { const float m = u(gen), e = (k == 0u && a == 1) ? 0.0f : 0.75f * (1.0f + u(gen)); p[a] = m - e; p[4 + a] = m + e; }
        p[7] = 2.0f;
    }
    c.models.assign(16u * (size_t)n, 0.0f);
    c.roots.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        float* m = &c.models[16u * (size_t)i];
        const float ang = kind == 1 ? 0.5f : 3.14159265f * u(gen), s = kind == 1 ? 1.0f : sc(gen), co = std::cos(ang) * s, si = std::sin(ang) * s;
        m[0] = co; m[2] = -si; m[5] = s; m[8] = si; m[10] = co; m[15] = 1.0f;
        if (kind != 1) { m[12] = at(gen); m[13] = at(gen); m[14] = at(gen); }          // kind 1: coincident
        if (kind == 0 && i % 7u == 6u) { m[3] = 0.01f * u(gen); m[7] = 0.01f * u(gen); }
        if (kind == 2 && i % 5u == 0u) { m[0] = m[1] = m[2] = m[3] = 0.0f; }           // singular
        c.roots[i] = c.node_cap + (kind == 1 ? 1u : gen() % kinds);
    }
    return c;
}

static int build(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.roots.size();
    o.tlas.assign(8u * (size_t)c.node_cap + 8u, kSentinel);
    o.blas.assign(20u * (size_t)n + 20u, kSentinel);
    o.lookup.assign((size_t)n + 1u, kSentinel);
    o.info = rt_tlas_info{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const char* why = nullptr;
    return rt_tl_build_host(c.models.data(), c.roots.data(), n, c.nodes.data(), (uint32_t)(c.nodes.size() / 8u), o.tlas.data(), o.blas.data(),
                            o.lookup.data(), c.node_cap, &o.info, &why);
}
static bool untouched(const Out& o) {
    for (float f : o.tlas) if (f != kSentinel) return false;
    for (float f : o.blas) if (f != kSentinel) return false;
    for (float f : o.lookup) if (f != kSentinel) return false;
    return true;
}
static bool same(const Out& a, const Out& b) {
    return std::memcmp(a.tlas.data(), b.tlas.data(), 4u * a.tlas.size()) == 0 && std::memcmp(a.blas.data(), b.blas.data(), 4u * a.blas.size()) == 0 &&
           std::memcmp(a.lookup.data(), b.lookup.data(), 4u * a.lookup.size()) == 0 && std::memcmp(&a.info, &b.info, sizeof a.info) == 0;
}

// the promises of an accepted call
static void check_tree(const Call& c, const Out& o) {
    const uint32_t n = (uint32_t)c.roots.size(), used = o.info.nodes_used;
    CHECK(used >= 1u && used <= c.node_cap && used <= 2u * n - 1u, "used %u of %u", used, c.node_cap);
    if (used < 1u || used > c.node_cap) return;
    std::vector<uint8_t> seen(used, 0), cover(n, 0);
    struct Item { uint32_t i, depth; };
    std::vector<Item> todo(1, Item{0u, 0u});
    uint32_t reached = 0, leaves = 0, depth = 0, max_leaf = 0;
    while (!todo.empty()) {
        const Item it = todo.back(); todo.pop_back();
        if (it.i >= used || seen[it.i]) { CHECK(false, "node %u outside the tree or reached twice", it.i); return; }
        seen[it.i] = 1; ++reached;
        depth = std::max(depth, it.depth);
        const float* p = &o.tlas[8u * (size_t)it.i];
        const uint32_t left = rt_bb_u32f(p[3]), count = rt_bb_u32f(p[7]);
        if (count == 0u) { todo.push_back(Item{left + 1u, it.depth + 1u}); todo.push_back(Item{left, it.depth + 1u}); continue; }
        if ((uint64_t)left + count > n) { CHECK(false, "leaf run of node %u", it.i); return; }
        ++leaves; max_leaf = std::max(max_leaf, count);
        for (uint32_t k = 0; k < count; ++k) ++cover[left + k];
    }
    CHECK(reached == used, "%u nodes reached, used %u", reached, used);
    CHECK(o.info.depth == depth && o.info.leaves == leaves && o.info.max_leaf == max_leaf, "info: depth %u / %u, leaves %u / %u, max_leaf %u / %u",
          o.info.depth, depth, o.info.leaves, leaves, o.info.max_leaf, max_leaf);
    CHECK(depth <= kTlMaxDepth, "an accepted tree of depth %u", depth);
    for (uint32_t k = 0; k < n; ++k) if (cover[k] != 1u) { CHECK(false, "position %u in %u leaves", k, cover[k]); break; }
    std::vector<uint8_t> named(n, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const float w = o.lookup[k];
        if (!(w >= 0.0f && w < (float)n && w == std::floor(w)) || named[(uint32_t)w]) { CHECK(false, "lookup word %u is %g", k, (double)w); break; }
        named[(uint32_t)w] = 1;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = &o.blas[20u * (size_t)i];
        if (r[16] != (float)c.roots[i] || r[17] != 0.0f || r[18] != 0.0f || r[19] != 0.0f) { CHECK(false, "record %u", i); break; }
    }
    for (size_t k = 8u * (size_t)used; k < 8u * (size_t)c.node_cap; ++k) if (o.tlas[k] != 0.0f || std::signbit(o.tlas[k])) { CHECK(false, "a node behind the tree is not zero"); break; }
    CHECK(o.tlas[8u * (size_t)c.node_cap] == kSentinel && o.blas[20u * (size_t)n] == kSentinel && o.lookup[n] == kSentinel, "a write beyond an output");
}

int main() {
    std::mt19937 gen(355);
    Out o, again;
    // instance sets of builder sizes
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t n : {1u, 2u, 3u, 16u, 17u, 65u, 257u, 3000u}) {
            Call c = instances(n, gen, kind);
            int rc = build(c, o);
            CHECK(rc == RT_OK, "kind %d, %u instances: %d", kind, n, rc);
            if (rc != RT_OK) continue;
            check_tree(c, o);
            if (kind == 1) CHECK(o.info.nodes_used == 1u && o.info.max_leaf == n, "coincident: one leaf");
            if (kind == 2) {
                const float* r = &o.blas[0];
                bool ident = true;
                for (int k = 0; k < 16; ++k) ident = ident && r[k] == ((k % 5 == 0) ? 1.0f : 0.0f);
                CHECK(ident, "a singular matrix: the identity");
            }
            rc = build(c, again);
            CHECK(rc == RT_OK && same(o, again), "a second build gave other bytes");
            // one node short: capacity, info set, nothing stored
            if (o.info.nodes_used > 1u) {
                Call s = c;
                s.node_cap = o.info.nodes_used - 1u;
                rc = build(s, again);
                CHECK(rc == RT_ERR_CAPACITY && untouched(again) && std::memcmp(&again.info, &o.info, sizeof o.info) == 0, "capacity: %d", rc);
            }
        }
    // the spine: cubes of half-width 2^-50 at x = 11^(i - 12)
    for (uint32_t n : {21u, 23u}) {
        Call c;
        c.node_cap = 2u * n - 1u;
        c.nodes.assign(8u * (size_t)(c.node_cap + 1u), 0.0f);
        const float h = std::ldexp(1.0f, -50);
        for (int a = 0; a < 3; ++a) { c.nodes[8u * (size_t)c.node_cap + a] = -h; c.nodes[8u * (size_t)c.node_cap + 4u + a] = h; }
        c.models.assign(16u * (size_t)n, 0.0f);
        c.roots.assign(n, c.node_cap);
        for (uint32_t i = 0; i < n; ++i) {
            float* m = &c.models[16u * (size_t)i];
            m[0] = m[5] = m[10] = m[15] = 1.0f;
            m[12] = (float)std::pow(11.0, (double)i - 12.0);
        }
        const int rc = build(c, o);
        if (n == 21u) { CHECK(rc == RT_OK && o.info.depth == 20u, "a spine of twenty levels: %d, depth %u", rc, o.info.depth); if (rc == RT_OK) check_tree(c, o); }
        else CHECK(rc == RT_ERR_UNSUPPORTED && o.info.depth == 22u && o.info.nodes_used == 45u && untouched(o), "a spine of 22 levels: %d, depth %u", rc, o.info.depth);
    }
    // the bad arguments
    {
        const Call good = instances(9u, gen, 0);
        const uint32_t n_nodes = (uint32_t)(good.nodes.size() / 8u);
        Call c = good; c.roots[4] = n_nodes;
        CHECK(build(c, o) == RT_ERR_INVALID_ARG && untouched(o), "a root beyond the nodes");
        c = good; c.roots[8] = c.node_cap - 1u;
        CHECK(build(c, o) == RT_ERR_INVALID_ARG && untouched(o), "a root below node_cap");
        c = good; c.roots[0] = 0xFFFFFFFFu;
        CHECK(build(c, o) == RT_ERR_INVALID_ARG && untouched(o), "a root of 2^32 - 1");
        c = good; c.node_cap = n_nodes + 1u;
        CHECK(build(c, o) == RT_ERR_INVALID_ARG && untouched(o), "node_cap beyond the nodes");
        c = good; c.roots.clear(); c.models.clear();
        CHECK(build(c, o) == RT_ERR_INVALID_ARG && untouched(o), "no instances");
        const char* why = nullptr;
        build(good, o);
        CHECK(rt_tl_build_host(good.models.data(), good.roots.data(), (1u << 20) + 1u, good.nodes.data(), n_nodes, o.tlas.data(), o.blas.data(),
                               o.lookup.data(), good.node_cap, nullptr, &why) == RT_ERR_INVALID_ARG, "more than 2^20 instances");
        CHECK(rt_tl_build_host(nullptr, good.roots.data(), 9u, good.nodes.data(), n_nodes, o.tlas.data(), o.blas.data(), o.lookup.data(), good.node_cap,
                               nullptr, &why) == RT_ERR_INVALID_ARG, "NULL models");
        CHECK(rt_tl_build_host(good.models.data(), good.roots.data(), 9u, good.nodes.data(), n_nodes, o.tlas.data(), o.blas.data(), nullptr, good.node_cap,
                               nullptr, &why) == RT_ERR_INVALID_ARG, "NULL lookup");
        CHECK(rt_tl_build_host(good.models.data(), good.roots.data(), 9u, good.nodes.data(), n_nodes, o.tlas.data(), o.blas.data(), o.lookup.data(),
                               good.node_cap, nullptr, &why) == RT_OK, "info may be NULL");
    }
    // garbage floats
    {
        const float odd[] = {NAN, INFINITY, -INFINITY, -1.0f, 0.0f, -0.0f, 3.0e38f, -3.0e38f, 1e30f, -1e30f, 1e-40f, 4294967296.0f,
                             std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max()};
        const uint32_t n_odd = (uint32_t)(sizeof odd / sizeof odd[0]);
        for (int it = 0; it < 300; ++it) {
            const uint32_t n = 1u + gen() % 90u;
            Call c = instances(n, gen, 0);
            for (float& f : c.models) if (gen() % (2u + it % 9u) == 0u) f = odd[gen() % n_odd];
            for (size_t k = 8u * (size_t)c.node_cap; k < c.nodes.size(); ++k) if (gen() % 6u == 0u) c.nodes[k] = odd[gen() % n_odd];
            const int rc = build(c, o);
            CHECK(rc == RT_OK || rc == RT_ERR_UNSUPPORTED, "garbage: %d", rc);
            if (rc == RT_OK) check_tree(c, o);
            else CHECK(untouched(o), "a refusal stored something");
        }
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("tlas build ok\n");
    return 0;
}
