// rt_deform.hip -- the device side of rt_deform_triangles (include/rt355.h): the vertices of a deforming mesh, gathered from device
// memory into the 160-byte triangle records.
//
// One lane per triangle.  It gathers up to nine vertex floats (through the face indices, clamped, when there are any), nine normal
// floats or the flat normal of the new corners, and stores only those words -- 36 or 72 of the record's 160 bytes, as partial
// writes: the record is never read, so its uv, its colour and its padding words keep their bytes.  Every stored bit comes from
// rt_deform.h (rt_df_triangle), which the host model compiles too; the flat normal is float32 with one rounding per operation, so
// this file is compiled without FMA contraction and without SLP vectorisation, like the other exact kernels.
// Neighbouring lanes write records 160 bytes apart: the stores are strided, 12 bytes a piece.  At 72 bytes per triangle the
// kernel is far below anything a frame costs (tools/deform_rate.py); plain vector stores, nothing else.
#include "rt_deform.h"

namespace rtk {

__global__ __launch_bounds__(256) void deform_triangles(RtDeformArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    // the call has checked first + n against the records written; clamped all the same
    if (i >= A.n || A.first >= A.n_tri || i >= A.n_tri - A.first) return;
    rt_df_triangle(A, i);
}

}  // namespace rtk

static hipError_t rt_launch_deform_triangles(const RtDeformArgs& a, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rtk::deform_triangles, dim3(a.n / 256u + (a.n % 256u ? 1u : 0u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

static const bool rt_deform_registered = (rt_deform_launch = &rt_launch_deform_triangles, true);
