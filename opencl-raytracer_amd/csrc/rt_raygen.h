// rt_raygen.h - host-side launchers of the posed-grid generator (rt_raygen.hip): the rays of rays.posed_rays, written on the
// device (rt_generate_rays_device / rt_set_pose), and the verdict of that grid without one ray stored.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rt_rays.h"

namespace rt {

// A pinhole grid (width, height, z) seen through the fp32 matrix m (row-major, m[3 r + c]) from `origin`. width and height are
// at most 2^24 (rt_set_camera's rule), so a column and a row are exact in fp32.
struct PoseGrid {
    uint32_t width, height;
    float z;
    float m[9];
    float origin[3];
};

// Writes width * height rays (2 float4 each: start, direction; d_rays 16-byte aligned) on `stream`. Reads nothing, writes nothing
// behind the last ray. A zero-sized grid launches nothing.
hipError_t launch_pose_rays(const PoseGrid& g, float4* d_rays, hipStream_t stream);

// Clears *d_result and ORs kRayDomain into its flags if a direction of the grid has |d|^2 outside (1e-30, 1e30) - the predicate of
// the ray scan (rt_rays.hip) on the rays launch_pose_rays would write. The other words of the record stay 0: direction.w and the
// starts of such a grid are known on the host (the origin is one point).
hipError_t launch_pose_verdict(const PoseGrid& g, RayScan* d_result, hipStream_t stream);

}  // namespace rt
