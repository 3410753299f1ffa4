// rt_pack.h - host-side launcher of the 8-bit output pass (rt_pack.hip): float4 frame -> RGBA8 / RGB8 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

// `format` is an rt_pixel_format (hip_raytracer.h). src: n float4 pixels, 16-byte aligned; dst: 4-byte aligned, n * 4 or
// n * 3 bytes, written in work-item order and not one byte beyond. lane_pixels: 0 = the measured choice (RGBA8: one pixel per
// lane, RGB8: four), 4 or 1 (RGBA8 only) = that form, for the A/B of tools/ab/packed_timing.py. n == 0 launches nothing.
hipError_t launch_pack(const float4* src, uint64_t n, int format, void* dst, hipStream_t stream, int lane_pixels = 0);

}  // namespace rt
