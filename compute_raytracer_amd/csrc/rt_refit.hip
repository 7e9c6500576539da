// rt_refit.hip -- the device side of rt_refit_blas (include/rt355.h): new boxes for the nodes of BLAS trees whose triangles moved.
//
// The host has walked the trees (rt_refit_plan.h) and hands over, per node, the run of lookup slots its leaves cover.  The box of
// a node is the float32 min / max over the three corners of every slot of its run, read from the corner array the traversal
// itself reads (rt_triangles.hip: tri_corners) -- exact, and independent of the order the corners are met in, so one wave per
// node reduces its run in whatever order its lanes stride over it: no atomics, no dependence between nodes, no second pass.
// The cost is the sum of the run lengths (triangles x depth for a builder's tree): 48 bytes per slot and level out of L2.
//
// One lane then stores the six floats wherever a kernel reads that node's box from: the node itself in every version of the node
// buffer (a frame reads the version of its slot of the event ring), and the halves of the relinked pair records that hold a copy
// of it (rt_flow_build.h).  Words 3 and 7 -- child or slot index, count, the pair records' metas -- are never written.
#include "rt_refit.h"

namespace rtk {

__global__ __launch_bounds__(256) void refit_nodes(RtRefitArgs A) {
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (e >= A.n_plan) return;                             // (whole waves leave: e is uniform in a wave)
    const uint32_t* p = A.plan + kRefitPlanWords * (size_t)e;
    const uint32_t node = p[0];
    // the plan was validated against these sizes on the host; clamped all the same
    const uint32_t first = p[1] < A.n_slots ? p[1] : A.n_slots;
    const uint32_t n = p[2] < A.n_slots - first ? p[2] : A.n_slots - first;
    const float huge = 1e30f;                              // the builder's starting values (acceleration/bvh.py: fit)
    float lo[3] = {huge, huge, huge}, hi[3] = {-huge, -huge, -huge};
    for (uint32_t k = lane; k < n; k += 64u) {
        const float4* c = A.corners + 3u * (size_t)(first + k);
#pragma unroll
        for (int j = 0; j < 3; ++j) {                      // fminf / fmaxf: a NaN corner is skipped
            const float4 v = c[j];
            lo[0] = fminf(lo[0], v.x); lo[1] = fminf(lo[1], v.y); lo[2] = fminf(lo[2], v.z);
            hi[0] = fmaxf(hi[0], v.x); hi[1] = fmaxf(hi[1], v.y); hi[2] = fmaxf(hi[2], v.z);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
    // every lane holds the box: lanes 0 .. kRefitVersions-1 store it into a version each, the next two into the pair records
    float* dst = nullptr;
    if (lane < kRefitVersions) {
        if (A.nodes[lane] && node < A.n_nodes) dst = A.nodes[lane] + 8u * (size_t)node;
    } else if (lane < kRefitVersions + 2u) {
        const uint32_t half = p[3u + (lane - kRefitVersions)];             // pair record * 2 + which child
        if (A.pairs && half != 0xFFFFFFFFu && (half >> 1) < A.n_pairs) dst = A.pairs + 8u * (size_t)half;
    }
    if (dst) {
        dst[0] = lo[0]; dst[1] = lo[1]; dst[2] = lo[2];
        dst[4] = hi[0]; dst[5] = hi[1]; dst[6] = hi[2];
    }
}

}  // namespace rtk

hipError_t rt_launch_refit_nodes(const RtRefitArgs& a, hipStream_t s) {
    if (a.n_plan == 0u) return hipSuccess;
    hipLaunchKernelGGL(rtk::refit_nodes, dim3((a.n_plan + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}
