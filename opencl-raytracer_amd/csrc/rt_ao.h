// rt_ao.h - launch interface of the ambient-occlusion pass (rt_ao.hip): K occlusion rays per item of a G-buffer - its hit point and
// normal - traced and counted in one kernel (hip_raytracer.h, "ambient-occlusion frames"; ao.py is the executable definition).
#pragma once

#include "rt_gbuffer.h"
#include "rt_query.h"

namespace rt {

// Inputs of one pass, device pointers: n items. point / normal: float4, 16-byte aligned. index: null (every item may be live) or n
// int32, 4-byte aligned. dirs: n_sets * samples float4 (w ignored), 16-byte aligned. samples: 1, 2, 4 ... 64. inv_samples: 1.0f / samples.
struct AoInputs {
    const float4* point;
    const float4* normal;
    const int32_t* index;
    const float4* dirs;
    uint32_t samples, n_sets;
    float bias, inv_samples;
};

// Outputs, device pointers: each may be null, not both. unoccluded: n bytes, any alignment; ao: n floats, 4-byte aligned.
struct AoOutputs {
    uint8_t* unoccluded;
    float* ao;
};

// What a pass adds up, once per wave: QueryCounters for its rays (n_rays == samples * n_live) and the live items.
struct AoCounters {
    QueryCounters q;
    unsigned long long n_live;
};

// One lane per (item, sample), 256 per workgroup, workgroups loop; any n = shard.n_local (n == 0 launches nothing). The set of item i
// is chosen by its GLOBAL work-item number, which `shard` gives as the G-buffer's record kernel computes it (world <= 1: i itself;
// shard.n_rays plays no part - a frame's padding arrives dead, index -1). `arith`: kUnfused / kFused / kDeviceCL.
hipError_t launch_ao(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const GBufferShard& shard, const AoInputs& in,
                     const AoOutputs& out, AoCounters* d_counters, hipStream_t stream);

}  // namespace rt
