// rt_refit_plan.h -- host side of the BLAS refit (rt_refit.hip: refit_nodes): which nodes hang under a set of roots and which run
// of triangle-lookup slots each of them covers.  Host-only, no HIP: tests/c/refit_plan_test.cpp compiles it with g++ under
// ASan + UBSan (tests/test_refit_sanitizers_cpu.py), on builder trees and on the bad trees below.
//
// A node of the reference's buffer is {min.xyz, leftChildIndex | max.xyz, primitiveCount} (RK:271-330): an inner node
// (u32(primitiveCount) == 0) has its children side by side at leftChildIndex and leftChildIndex + 1, a leaf owns the lookup slots
// [leftChildIndex, leftChildIndex + primitiveCount).  Every tree the project's builders make (acceleration/bvh.py, the
// reference's bvh.ts) partitions ONE index run in place, so the leaves under any node form one contiguous run of slots: the
// box of a node is then a plain min / max over corners [first, first + n) of the corner array, whatever lies between the node
// and its leaves -- no dependence between nodes, no order of evaluation.  The plan is that run per node; the walk here is what
// proves it before a kernel is launched.
//
// Unlike the render walk nothing is clamped: an index the walk would clamp to the last node names a node the tree does not
// own, and a refit must not write there.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "rt_flow_build.h"     // rt_flow_u32f: WGSL's u32(f32)

enum RtRefitStatus {
    kRefitOk = 0,
    kRefitInvalid = -1,        // = RT_ERR_INVALID_ARG: an index beyond the buffers, or a node reached twice (sharing, a cycle)
    kRefitUnsupported = -4     // = RT_ERR_UNSUPPORTED: a node whose leaves do not form one contiguous run
};

// nodes: the node buffer as rt_write_nodes receives it (8 floats per node); roots: node indices (any order, duplicates allowed).
// plan: one triple {node, first_slot, n_slots} per reached node -- roots in ascending order, each tree in depth-first order,
// the left child first.  Empty unless the result is kRefitOk.  why: a static string naming the first failure.
inline int rt_refit_plan_build(const float* nodes, uint32_t n_nodes, uint32_t n_tri_lookup, const uint32_t* roots, uint32_t n_roots,
                               std::vector<uint32_t>& plan, const char** why = nullptr) {
    plan.clear();
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    std::vector<uint32_t> rs(roots, roots + n_roots);
    std::sort(rs.begin(), rs.end());
    rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
    std::vector<uint8_t> seen(n_nodes, 0);
    std::vector<uint32_t> right;                                   // per plan entry of an inner node: the entry of its right child
    struct Todo { uint32_t node, parent; };                        // parent: the entry whose RIGHT child this is, 0xFFFFFFFF: none
    std::vector<Todo> todo;
    for (uint32_t r : rs) {
        todo.push_back({r, 0xFFFFFFFFu});
        while (!todo.empty()) {
            const Todo t = todo.back();
            todo.pop_back();
            if (t.node >= n_nodes) { plan.clear(); *why = "a node index beyond the node buffer"; return kRefitInvalid; }
            if (seen[t.node]) { plan.clear(); *why = "a node reached twice (shared by two parents or roots, or a cycle)"; return kRefitInvalid; }
            seen[t.node] = 1;
            const uint32_t e = (uint32_t)right.size();
            if (t.parent != 0xFFFFFFFFu) right[t.parent] = e;
            const float* p = nodes + 8u * (size_t)t.node;
            const uint32_t left = rt_flow_u32f(p[3]), count = rt_flow_u32f(p[7]);
            plan.push_back(t.node);
            right.push_back(0xFFFFFFFFu);
            if (count != 0u) {                                     // a leaf: its own run
                if ((uint64_t)left + count > n_tri_lookup) { plan.clear(); *why = "a leaf run beyond the triangle lookup table"; return kRefitInvalid; }
                plan.push_back(left);
                plan.push_back(count);
                continue;
            }
            plan.push_back(0u);
            plan.push_back(0u);
            if ((uint64_t)left + 1u >= n_nodes) { plan.clear(); *why = "a child index beyond the node buffer"; return kRefitInvalid; }
            todo.push_back({left + 1u, e});                        // popped second: entered after the whole left subtree
            todo.push_back({left, 0xFFFFFFFFu});                   // popped first: entry e + 1
        }
    }
    // runs of the inner nodes, children before parents (a child's entry lies behind its parent's)
    bool gap = false;
    for (size_t e = right.size(); e-- > 0;) {
        if (right[e] == 0xFFFFFFFFu) continue;                     // a leaf
        const uint32_t* a = &plan[3u * (e + 1u)];
        const uint32_t* b = &plan[3u * (size_t)right[e]];
        const uint64_t af = a[1], an = a[2], bf = b[1], bn = b[2];
        uint64_t first = 0, n = 0;
        if (an == 0u || bn == 0u) gap = true;                      // a child that already failed
        else if (af + an == bf) { first = af; n = an + bn; }
        else if (bf + bn == af) { first = bf; n = an + bn; }
        else gap = true;
        plan[3u * e + 1u] = (uint32_t)first;
        plan[3u * e + 2u] = (uint32_t)n;
    }
    if (gap) { plan.clear(); *why = "a node whose leaves do not form one contiguous run of lookup slots"; return kRefitUnsupported; }
    return kRefitOk;
}
