// rt_refit_plan.h -- the host walk behind rt_refit_blas / rt_refit_plan -- under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_refit_sanitizers_cpu.py).  Inputs: trees laid out as a builder lays them out (children side by side, leaves
// partitioning one index run), the hand-made bad trees of tests/refit_common.py, spines deeper than any recursion would like,
// and random garbage (NaN / infinite / negative / huge indices and counts, cycles, roots beyond the buffer).  Checked: no bad
// access or UB (the sanitizers), the documented status of every bad tree, and on every accepted plan: each node once, every run
// inside the lookup table, an inner node's run the two children's runs side by side.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "../../compute_raytracer_amd/csrc/rt_refit_plan.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static void node(std::vector<float>& n, uint32_t i, float left, float count) {
    if (n.size() < 8u * (i + 1u)) n.resize(8u * (i + 1u), 0.0f);
    n[8u * i + 3u] = left; n[8u * i + 7u] = count;
}

// a builder's tree over slots [0, slots) at node `base`: every leaf 1 .. 4 slots
static void builder_tree(std::vector<float>& n, uint32_t base, uint32_t slot0, uint32_t slots, std::mt19937& gen) {
    struct Job { uint32_t node, lo, hi; };
    std::vector<Job> todo{{base, slot0, slot0 + slots}};
    uint32_t used = std::max((uint32_t)(n.size() / 8u), base + 1u);
    while (!todo.empty()) {
        const Job j = todo.back(); todo.pop_back();
        if (j.hi - j.lo <= 1u + gen() % 4u) { node(n, j.node, (float)j.lo, (float)(j.hi - j.lo)); continue; }
        const uint32_t left = used;
        used += 2u;
        node(n, j.node, (float)left, 0.0f);
        const uint32_t mid = j.lo + 1u + gen() % (j.hi - j.lo - 1u);
        todo.push_back({left, j.lo, mid});
        todo.push_back({left + 1u, mid, j.hi});
    }
    node(n, used - 1u, n[8u * (used - 1u) + 3u], n[8u * (used - 1u) + 7u]);
}

static void check_plan(const std::vector<float>& n, uint32_t n_lookup, const std::vector<uint32_t>& plan) {
    const uint32_t n_nodes = (uint32_t)(n.size() / 8u);
    std::map<uint32_t, std::pair<uint32_t, uint32_t>> run;
    for (size_t e = 0; e < plan.size(); e += 3u) {
        CHECK(plan[e] < n_nodes, "node %u", plan[e]);
        CHECK(run.find(plan[e]) == run.end(), "node %u planned twice", plan[e]);
        CHECK(plan[e + 2u] >= 1u && (uint64_t)plan[e + 1u] + plan[e + 2u] <= n_lookup, "run of node %u", plan[e]);
        run[plan[e]] = {plan[e + 1u], plan[e + 2u]};
    }
    for (const auto& kv : run) {
        const float* p = n.data() + 8u * (size_t)kv.first;
        const uint32_t left = rt_flow_u32f(p[3]), count = rt_flow_u32f(p[7]);
        if (count) { CHECK(kv.second.first == left && kv.second.second == count, "leaf %u", kv.first); continue; }
        CHECK(run.count(left) && run.count(left + 1u), "children of %u", kv.first);
        if (!run.count(left) || !run.count(left + 1u)) continue;
        const auto a = run[left], b = run[left + 1u];
        CHECK(kv.second.second == a.second + b.second && kv.second.first == std::min(a.first, b.first) &&
              (a.first + a.second == b.first || b.first + b.second == a.first), "run of inner node %u", kv.first);
    }
}

int main() {
    std::mt19937 gen(355);
    std::vector<uint32_t> plan;
    const char* why = nullptr;
    // builder trees: one, and two side by side in one buffer behind three top-level nodes
    for (uint32_t slots : {1u, 2u, 7u, 64u, 1000u}) {
        std::vector<float> n;
        builder_tree(n, 3u, 0u, slots, gen);
        const uint32_t second = (uint32_t)(n.size() / 8u);
        builder_tree(n, second, slots, slots + 5u, gen);
        const uint32_t roots[3] = {second, 3u, second};
        int rc = rt_refit_plan_build(n.data(), (uint32_t)(n.size() / 8u), 2u * slots + 5u, roots, 3u, plan, &why);
        CHECK(rc == kRefitOk, "builder trees of %u slots: %d %s", slots, rc, why);
        CHECK(plan.size() / 3u == n.size() / 8u - 3u, "every node of both trees");
        CHECK(plan.size() >= 3u && plan[0] == 3u && plan[1] == 0u && plan[2] == slots, "the first root's run");
        check_plan(n, 2u * slots + 5u, plan);
        rc = rt_refit_plan_build(n.data(), (uint32_t)(n.size() / 8u), 2u * slots + 4u, roots, 3u, plan, &why);   // a table one slot short
        CHECK(rc == kRefitInvalid && plan.empty(), "short lookup table: %d", rc);
    }
    // a spine of 100,000 inner nodes: no recursion to overflow
    {
        const uint32_t depth = 100000u;
        std::vector<float> n;
        for (uint32_t k = 0; k < depth; ++k) { node(n, 2u * k, (float)(2u * k + 1u), 0.0f); node(n, 2u * k + 1u, (float)k, 1.0f); }
        node(n, 2u * depth, (float)depth, 1.0f);
        for (uint32_t k = 0; k < depth; ++k) n[8u * (2u * k) + 3u] = (float)(2u * k + 1u);
        // node 2k: children 2k+1 (leaf, slot k) and 2k+2 (the rest)
        const uint32_t root = 0u;
        const int rc = rt_refit_plan_build(n.data(), 2u * depth + 1u, depth + 1u, &root, 1u, plan, &why);
        CHECK(rc == kRefitOk && plan.size() / 3u == 2u * depth + 1u && plan[2] == depth + 1u, "spine: %d %s", rc, why);
    }
    // the bad trees of tests/refit_common.py
    {
        const float good[5][2] = {{1, 0}, {0, 2}, {3, 0}, {2, 1}, {3, 2}};
        auto make = [&](std::vector<float>& n) { n.clear(); for (uint32_t i = 0; i < 5u; ++i) node(n, i, good[i][0], good[i][1]); };
        std::vector<float> n;
        const uint32_t r0 = 0u, r02[2] = {0u, 2u}, r5 = 5u;
        make(n); CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitOk && plan.size() == 15u, "good tree");
        make(n); n[8 * 2 + 3] = 4.0f; CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "child beyond the buffer");
        make(n); n[8 * 2 + 3] = 4294967295.0f; CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "saturated child");
        make(n); n[8 * 4 + 7] = 3.0f; CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "leaf run beyond the table");
        make(n); n[8 * 4 + 3] = 4294967295.0f; CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "leaf slot saturates");
        make(n); n[8 * 2 + 3] = 0.0f; CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "cycle");
        make(n); CHECK(rt_refit_plan_build(n.data(), 5u, 5u, r02, 2u, plan) == kRefitInvalid, "two roots sharing a subtree");
        make(n); CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r5, 1u, plan) == kRefitInvalid, "root beyond the buffer");
        make(n); CHECK(rt_refit_plan_build(n.data(), 0u, 5u, &r0, 1u, plan) == kRefitInvalid, "empty buffer");
        make(n); CHECK(rt_refit_plan_build(n.data(), 5u, 5u, nullptr, 0u, plan) == kRefitOk && plan.empty(), "no roots");
        n.clear(); node(n, 0, 1, 0); node(n, 1, 3, 0); node(n, 2, 3, 0); node(n, 3, 0, 2); node(n, 4, 2, 3);
        CHECK(rt_refit_plan_build(n.data(), 5u, 5u, &r0, 1u, plan) == kRefitInvalid, "node shared by two parents");
        n.clear(); node(n, 0, 1, 0); node(n, 1, 3, 2); node(n, 2, 0, 2);
        CHECK(rt_refit_plan_build(n.data(), 3u, 5u, &r0, 1u, plan) == kRefitUnsupported && plan.empty(), "a gap between the runs");
        n.clear(); node(n, 0, 1, 0); node(n, 1, 1, 3); node(n, 2, 0, 2);
        CHECK(rt_refit_plan_build(n.data(), 3u, 5u, &r0, 1u, plan) == kRefitUnsupported, "overlapping runs");
    }
    // garbage: whatever comes back, an accepted plan keeps its promises
    {
        const float odd[] = {NAN, INFINITY, -INFINITY, -1.0f, 0.0f, 0.5f, 1.0f, 2.0f, 3.0f, 7.0f, 4294967040.0f, 4294967296.0f, 1e30f,
                             std::numeric_limits<float>::denorm_min()};
        uint32_t ok = 0;
        for (int it = 0; it < 4000; ++it) {
            const uint32_t nn = 1u + gen() % 12u, nl = gen() % 10u;
            std::vector<float> n(8u * nn);
            for (float& f : n) f = (gen() % 3u) ? (float)(gen() % (nn + 2u)) : odd[gen() % (sizeof odd / sizeof odd[0])];
            uint32_t roots[3] = {gen() % (nn + 2u), gen() % (nn + 2u), gen() % 2u ? 0xFFFFFFFFu : gen() % nn};
            const int rc = rt_refit_plan_build(n.data(), nn, nl, roots, gen() % 4u, plan, &why);
            CHECK(rc == kRefitOk || rc == kRefitInvalid || rc == kRefitUnsupported, "status %d", rc);
            CHECK(rc == kRefitOk || plan.empty(), "a refused tree leaves a plan");
            if (rc == kRefitOk) { ++ok; check_plan(n, nl, plan); }
        }
        CHECK(ok > 100u, "only %u accepted garbage trees", ok);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("refit plan ok\n");
    return 0;
}
