// rt_pack.hip - the 8-bit output pass: one sweep over a device-resident float4 frame, bytes out in work-item order.
//
// The byte a channel becomes (hip_raytracer.h, "8-bit frames"): p = v * 255.0f (one fp32 multiplication), f = floorf(p);
// NaN or f < 0 -> 0, f >= 255 -> 255, else (uint8_t)f. Where the reference's PPMExporter::ExportP3 expression
// min(255, (int)floorf(v * 255.f)) (PPMExporter.cpp:7-30) yields 0..255 this is that expression; outside it the
// reference's (int) conversion is undefined and a byte cannot carry what it happens to give.
//
// A streaming kernel: 20 (RGBA8) or 19 (RGB8) bytes of traffic per pixel, next to no arithmetic. Two forms:
//   pack_pixels         a lane converts FOUR consecutive pixels - four 16-byte loads, then one 16-byte (RGBA8) or one 12-byte
//                       (RGB8) store. The launcher cuts the frame into a head (RGBA8 only: the pixels in front of the first
//                       16-byte boundary of the destination), the body of whole groups and a tail of n % 4 pixels; head and tail
//                       pixels get a lane each and narrow stores, so nothing is written beyond the last pixel's last byte.
//   pack_pixels_narrow  RGBA8 only: a lane converts ONE pixel - one 16-byte load (a wave reads 1 KiB contiguous), one 4-byte
//                       store (plain stores: a wave's 256 bytes merge in L2).
// Measured on a resident 4096^2 frame (tools/ab/packed_timing.py, profiles/packed_output_timing.json): RGBA8 0.0589 ms narrow
// against 0.0596 ms in fours (medians of 7; 0.0592 against 0.0611 in an earlier run) - the store width does not matter here,
// plain stores merge in L2, and the narrow form was never the slower one - so RGBA8 is packed the narrow way and the form in
// fours stays selectable (launch_pack's lane_pixels) for the A/B; RGB8, which cannot be written a pixel at a time without byte
// stores, goes in fours (0.053 ms).
#include "rt_pack.h"
#include "hip_raytracer.h"

namespace rt {
namespace {

constexpr uint32_t kPackBlock = 256;

__device__ __forceinline__ uint32_t quantise(float v) {
    const float f = floorf(v * 255.0f);
    // branch-free clamp: fmaxf returns its other operand for a NaN (C99 7.12.12.2), so NaN, negatives and -inf become 0, then
    // everything from 255 up, +inf included, becomes 255; the conversion only ever sees 0 .. 255
    return (uint32_t)fminf(fmaxf(f, 0.0f), 255.0f);
}

__device__ __forceinline__ uint32_t rgba8(const float4 p) {
    return quantise(p.x) | (quantise(p.y) << 8) | (quantise(p.z) << 16) | (quantise(p.w) << 24);
}

struct alignas(4) Bytes12 { uint32_t a, b, c; };

// one pixel, narrow stores: a word (RGBA8) or three bytes (RGB8)
template <int FORMAT>
__device__ __forceinline__ void pack_one(const float4* __restrict__ src, uint8_t* __restrict__ dst, uint64_t i) {
    const float4 p = src[i];
    if (FORMAT == RT_PIXEL_RGBA8) {
        reinterpret_cast<uint32_t*>(dst)[i] = rgba8(p);
    } else {
        uint8_t* q = dst + 3 * i;
        q[0] = (uint8_t)quantise(p.x);
        q[1] = (uint8_t)quantise(p.y);
        q[2] = (uint8_t)quantise(p.z);
    }
}

// work-item g < groups: pixels head + 4 g .. head + 4 g + 3, one wide store; the `head` + `tail` work-items behind them: one
// pixel each in front of / behind the body
template <int FORMAT>
__global__ __launch_bounds__(kPackBlock) void pack_pixels(const float4* __restrict__ src, uint8_t* __restrict__ dst, uint64_t groups,
                                                          uint32_t head, uint32_t tail) {
    const uint64_t g = (uint64_t)blockIdx.x * kPackBlock + threadIdx.x;
    if (g < groups) {
        const uint64_t i = head + 4 * g;
        const float4 p0 = src[i], p1 = src[i + 1], p2 = src[i + 2], p3 = src[i + 3];
        if (FORMAT == RT_PIXEL_RGBA8) {
            *reinterpret_cast<uint4*>(dst + 4 * i) = make_uint4(rgba8(p0), rgba8(p1), rgba8(p2), rgba8(p3));  // 16-byte aligned: the head saw to it
        } else {
            Bytes12 w;
            w.a = quantise(p0.x) | (quantise(p0.y) << 8) | (quantise(p0.z) << 16) | (quantise(p1.x) << 24);
            w.b = quantise(p1.y) | (quantise(p1.z) << 8) | (quantise(p2.x) << 16) | (quantise(p2.y) << 24);
            w.c = quantise(p2.z) | (quantise(p3.x) << 8) | (quantise(p3.y) << 16) | (quantise(p3.z) << 24);
            *reinterpret_cast<Bytes12*>(dst + 3 * i) = w;  // 12 i bytes from a 4-byte aligned base
        }
        return;
    }
    const uint64_t j = g - groups;
    if (j < head) pack_one<FORMAT>(src, dst, j);
    else if (j < (uint64_t)head + tail) pack_one<FORMAT>(src, dst, head + 4 * groups + (j - head));
}

// the one-pixel-per-lane form (RGBA8): one 16-byte load, one 4-byte store
__global__ __launch_bounds__(kPackBlock) void pack_pixels_narrow(const float4* __restrict__ src, uint8_t* __restrict__ dst, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kPackBlock + threadIdx.x;
    if (i < n) pack_one<RT_PIXEL_RGBA8>(src, dst, i);
}

}  // namespace

hipError_t launch_pack(const float4* src, uint64_t n, int format, void* dst, hipStream_t stream, int lane_pixels) {
    if (format != RT_PIXEL_RGBA8 && format != RT_PIXEL_RGB8) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst);
    if (!src || !dst || (d & 3u) || (reinterpret_cast<uintptr_t>(src) & 15u)) return hipErrorInvalidValue;
    uint8_t* out = static_cast<uint8_t*>(dst);
    if (format == RT_PIXEL_RGBA8 && lane_pixels != 4) {
        const uint64_t blocks = (n + kPackBlock - 1) / kPackBlock;
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pack_pixels_narrow, dim3((uint32_t)blocks), dim3(kPackBlock), 0, stream, src, out, n);
        return hipGetLastError();
    }
    // RGBA8: 0..3 pixels up to the destination's first 16-byte boundary (the source stays 16-byte aligned: a pixel is 16 bytes of it)
    const uint64_t to_boundary = format == RT_PIXEL_RGBA8 ? ((16u - (d & 15u)) & 15u) / 4u : 0u;
    const uint32_t head = (uint32_t)(to_boundary < n ? to_boundary : n);
    const uint64_t groups = (n - head) / 4;
    const uint32_t tail = (uint32_t)((n - head) % 4);
    const uint64_t items = groups + head + tail;
    const uint64_t blocks = (items + kPackBlock - 1) / kPackBlock;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (format == RT_PIXEL_RGBA8)
        hipLaunchKernelGGL(pack_pixels<RT_PIXEL_RGBA8>, dim3((uint32_t)blocks), dim3(kPackBlock), 0, stream, src, out, groups, head, tail);
    else
        hipLaunchKernelGGL(pack_pixels<RT_PIXEL_RGB8>, dim3((uint32_t)blocks), dim3(kPackBlock), 0, stream, src, out, groups, head, tail);
    return hipGetLastError();
}

}  // namespace rt
