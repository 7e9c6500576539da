// rt_query_device.h -- what the query kernels of rt_query.hip and rt_shade.hip share: the workgroup shape, the size of a staged
// sphere chunk, and the ray record.
#pragma once
#include "rt_device.h"

namespace rtk {

constexpr int kQueryWaves = 4;
constexpr uint32_t kQueryThreads = 64u * kQueryWaves;
constexpr uint32_t kSphereChunk = 1024u;       // sphere records {centre, radius^2} staged per round: 16 KB of LDS

__device__ __forceinline__ void load_ray(const float4* __restrict__ rays, size_t i, v3& o, v3& d) {
    const float4 a = rays[2u * i], b = rays[2u * i + 1u];
    o = V(a.x, a.y, a.z);
    d = V(b.x, b.y, b.z);
}

}  // namespace rtk
