// rt_tlas.hip -- the device side of rt_build_tlas (include/rt355.h): a second front end for the level-synchronous SAH builder of
// rt_build.hip.  Its primitives are the instances' world boxes instead of triangles: one lane per instance reads the instance's
// forward matrix and the node record at its root, and leaves the BLAS record (the inverse matrix and the root index), the padded
// world box with its centroid as an RtBbPrim, and order[0] = identity.  From there on the builder's own passes run unchanged over
// one range {root_node 0, first_slot 0, n_slots n}: build_root, then price / scan / split per level, count_up, rank_down, emit.
//
// The arithmetic is rt_tlas_build.h's, the same inline functions the host model (rt_build_tlas_host) calls.  Built with
// -ffp-contract=off -fno-slp-vectorize: the cofactors and the corner transforms are float64 sums of products and must stay so.
// No atomics; the root index, the one index read from memory, is clamped before it addresses anything.
#include "rt_build.h"
#include "rt_tlas_build.h"

namespace rtk {

__global__ __launch_bounds__(256) void tlas_prep(RtBuildArgs A) {
    const RtBuildInstances& T = A.inst;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_slots || T.n_nodes == 0u) return;
    const float4* mp = reinterpret_cast<const float4*>(T.models) + 4u * (size_t)i;
    float m[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 col = mp[c];
        m[4 * c] = col.x; m[4 * c + 1] = col.y; m[4 * c + 2] = col.z; m[4 * c + 3] = col.w;
    }
    const uint32_t root = T.roots[i];
    const uint32_t at = root < T.n_nodes ? root : T.n_nodes - 1u;
    const float4* np = reinterpret_cast<const float4*>(T.nodes) + 2u * (size_t)at;
    const float4 n0 = np[0], n1 = np[1];
    const float rec[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    float out[20];
    rt_tl_record(m, root, out);
    float4* bp = reinterpret_cast<float4*>(T.blas) + 5u * (size_t)i;
#pragma unroll
    for (int c = 0; c < 5; ++c) bp[c] = make_float4(out[4 * c], out[4 * c + 1], out[4 * c + 2], out[4 * c + 3]);
    RtBbPrim p;
    rt_tl_prim(m, rec, i, p);
    A.prim[i] = p;
    A.order[0][i] = i;
}

}  // namespace rtk

hipError_t rt_launch_tlas_prep(const RtBuildArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(rtk::tlas_prep, dim3((a.n_slots + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}
