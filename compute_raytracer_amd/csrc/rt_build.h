// rt_build.h -- scratch layout and launchers of the device BLAS build (rt_build.hip), shared with rt_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rt_blas_build.h"

constexpr uint32_t kBuildVersions = 4u;      // = rt_ctx.h kVersions: the versions of the node buffer

// A node of the build, level by level: the nodes of level L are [off[L], off[L] + cnt[L]) of these arrays (the host keeps off / cnt).
struct RtBuildNode {                         // 32 bytes
    float lo[3]; uint32_t first;             // the node's run: positions [first, first + count) of the lookup table
    float hi[3]; uint32_t count;
};
struct RtBuildDec {                          // what price decided, 80 bytes
    double plane;
    uint32_t axis, n_left;
    uint32_t split;                          // 0: a leaf
    uint32_t child;                          // a split: its children are nodes child and child + 1 of the NEXT level
    float box[12];                           // the children's boxes {lo, hi} x {left, right}: the winning plane's two sides
    uint32_t pad[2];
};

// The other front end (rt_tlas.hip, rt_build_tlas): the primitives of the one range are INSTANCES -- their padded world boxes --
// instead of triangles.  models == nullptr: triangles.
struct RtBuildInstances {
    const float* models;                     // n_slots x 16 floats, column-major, 16-byte aligned
    const uint32_t* roots;                   // n_slots root node indices
    const float* nodes; uint32_t n_nodes;    // the node buffer the roots index (one version of it)
    float* blas;                             // out: n_slots x 20 floats, 16-byte aligned
};

struct RtBuildArgs {
    // the scene
    const float* tri; uint32_t n_tri;        // 40-float records
    float* lookup; uint32_t n_slots;         // the lookup table (read by prep, written by emit)
    float* nodes[kBuildVersions]; uint32_t n_nodes;
    // the call
    const rt_blas_range* ranges; uint32_t n_ranges;
    // scratch: per lookup slot ...
    RtBbPrim* prim;                          // by ORIGINAL slot
    uint32_t* order[2];                      // by position: the original slot there, level L reads order[L & 1]
    uint32_t* final_order;                   // by position, written by the leaf that ends up owning it
    // ... and per build node (node_cap of them)
    RtBuildNode* node; RtBuildDec* dec;
    uint32_t* sub;                           // splits in the node's subtree, itself included
    uint32_t* rank;                          // preorder rank of a split node among its tree's splits
    uint32_t* index;                         // where the node goes in the node buffer
    uint32_t* root;                          // the root_node of the node's tree
    uint32_t node_cap;
    uint32_t* next_count;                    // one word: the node count of the next level
    RtBuildInstances inst = {};
};

// h_ranges: the host's copy of a.ranges (grid sizes come from it)
hipError_t rt_launch_build_prep(const RtBuildArgs& a, const rt_blas_range* h_ranges, hipStream_t s);        // prims, order[0], level 0
hipError_t rt_launch_tlas_prep(const RtBuildArgs& a, hipStream_t s);         // rt_tlas.hip: prims and order[0] of a.inst (build_prep calls it)
hipError_t rt_launch_build_level(const RtBuildArgs& a, uint32_t level, uint32_t off, uint32_t cnt, hipStream_t s);   // price, scan (-> next_count), split
hipError_t rt_launch_build_count_up(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s);
hipError_t rt_launch_build_rank_down(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s);
hipError_t rt_launch_build_emit_nodes(const RtBuildArgs& a, uint32_t off, uint32_t cnt, hipStream_t s);
hipError_t rt_launch_build_emit_lookup(const RtBuildArgs& a, const rt_blas_range* h_ranges, hipStream_t s);
