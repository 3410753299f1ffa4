// rt_resolve.h - host-side launcher of the supersampling filter (rt_resolve.hip): s x s samples -> one pixel, float4 or bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

enum ResolveForm { kResolveAuto = 0, kResolveLanePerPixel = 1, kResolveLanePerSample = 2 };

// src: sample_rows rows of sample_width float4 samples, 16-byte aligned; both multiples of s (2, 3 or 4). dst: (sample_width / s)
// x (sample_rows / s) pixels in row-major order - float4 (format 0, 16-byte aligned) or the bytes of an rt_pixel_format (4-byte
// aligned), written in pixel order and not one byte beyond. The pixel is hip_raytracer.h's ("supersampled frames"): the samples
// added in (b, a) order, one multiplication by fl(1 / s^2); the byte forms quantise that value in registers (rt_pack.hip's
// table). form: kResolveAuto = the measured choice (a lane per sample for s = 4 and for s = 2 but RGB8 when a row fills a wave, a
// lane per pixel otherwise), the other two for the A/B of tools/ab/supersample_timing.py. Zero pixels launch nothing.
hipError_t launch_resolve(const float4* src, uint32_t sample_width, uint32_t sample_rows, uint32_t s, int format, void* dst,
                          hipStream_t stream, int form = kResolveAuto);

}  // namespace rt
