// rt_rays.h - host-side launcher of the ray scan (rt_rays.hip): what rt_create's host loops find out about an uploaded ray
// array, found out on the device about rays that already are in device memory (rt_set_rays_device / rt_set_rays).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

// The scan's result, eight words in device memory. All of it is a bitwise OR or an unsigned maximum over the rays, so the
// order the rays are met in does not matter and an all-zero record is the identity (launch_ray_scan clears it).
//   flags       kRayDirW | kRayDomain | kRayStart: some ray fails that predicate (rt_rays.hip states them)
//   lo_inv[a]   max over the rays of ~key(start[a])   -> the smallest start[a] is unkey(~lo_inv[a])
//   hi[a]       max over the rays of  key(start[a])   -> the largest  start[a] is unkey(hi[a])
// key() maps the BITS of a float to an unsigned integer that orders like the number does (ray_key below): negative values,
// -0.0f (just below +0.0f) and denormals keep their place, and no floating-point instruction ever sees them.
struct RayScan {
    uint32_t flags;
    uint32_t lo_inv[3];
    uint32_t hi[3];
    uint32_t pad;
};
constexpr uint32_t kRayDirW = 1u;    // a direction.w != 0.0f
constexpr uint32_t kRayDomain = 2u;  // a direction with |d|^2 outside (1e-30, 1e30), NaN included
constexpr uint32_t kRayStart = 4u;   // a start.w != 1.0f, or (sx + sy) + sz not finite in fp32

__host__ __device__ inline uint32_t ray_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ inline uint32_t ray_unkey(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// Clears *d_result and scans n rays (n x 2 float4: start, direction; 16-byte aligned) on `stream`. Reads the rays, writes
// d_result only. n == 0 leaves the cleared record.
hipError_t launch_ray_scan(const float4* d_rays, uint64_t n, RayScan* d_result, hipStream_t stream);

}  // namespace rt
