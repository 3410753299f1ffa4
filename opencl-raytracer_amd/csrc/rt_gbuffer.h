// rt_gbuffer.h - launch interface of the G-buffer record kernel (rt_gbuffer.hip): the (t, index) a hittest frame left per local
// work-item, turned into hit records and the winner's albedo (hip_raytracer.h, "G-buffer frames").
#pragma once

#include "rt_device.h"
#include "rt_query.h"

namespace rt {

// Which global work-item a local one is: the shard's fields of RenderParams (rt_kernels.h), as global_ray_of reads them on the
// LOCAL PIXEL index (the records are in pixel order, so the tile order of a wavefront frame plays no part).
struct GBufferShard {
    uint64_t n_rays;      // rays of the whole frame: a local work-item whose global one is not below it is padding
    uint64_t n_local;     // work-items of the pass
    uint64_t tile_rays;   // shard tile length in rays (>= 1)
    uint32_t rank, world;
};

// Inputs and outputs of one pass, device pointers. t and index are READ (n_local elements each, what the frame's primary round
// wrote) and never written. point / normal / albedo: each may be null, not all of them; 16-byte aligned.
struct GBufferRecords {
    const float* t;
    const int32_t* index;
    float4* point;
    float4* normal;
    float4* albedo;
};

// One thread per local work-item, 256 per workgroup, workgroups loop. `arith`: kUnfused / kFused / kDeviceCL. d_hits: one
// unsigned long long the kernel ADDS the work-items with index >= 0 to (once per wave); the caller zeroes it on the stream.
hipError_t launch_gbuffer_records(const Scene& scene, const QueryCamera& camera, const GBufferShard& shard, int arith,
                                  const GBufferRecords& rec, unsigned long long* d_hits, hipStream_t stream);

}  // namespace rt
