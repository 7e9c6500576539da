// rt_refit.h -- arguments of the BLAS refit kernel (rt_refit.hip), shared with rt_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr uint32_t kRefitVersions = 4u;      // = rt_ctx.h kVersions: the versions of the node buffer
constexpr uint32_t kRefitPlanWords = 5u;     // per planned node: {node, first_slot, n_slots, pair half of its copy as a left child, as a
                                             // right child}; a pair half is record * 2 + child, 0xFFFFFFFF: the node has no such copy

struct RtRefitArgs {
    const uint32_t* plan;                    // [n_plan][kRefitPlanWords]
    uint32_t n_plan;
    const float4* corners;                   // [n_slots][3]: rt_triangles.hip tri_corners
    uint32_t n_slots;
    float* nodes[kRefitVersions];            // every version of the node buffer, n_nodes nodes of 8 floats each
    uint32_t n_nodes;
    float* pairs;                            // the relinked pair records (16 floats each), or null when they are not current
    uint32_t n_pairs;
};

hipError_t rt_launch_refit_nodes(const RtRefitArgs& a, hipStream_t s);
