// rt_resolve.hip - the supersampling filter: one sweep over a device-resident float4 SAMPLE frame, one pixel out per s x s block.
//
// The pixel (hip_raytracer.h, "supersampled frames"), each of the four channels by itself, fp32, every addition rounded:
//     acc = sample[(s j) w + s i];  for b in 0..s-1, a in 0..s-1, (b, a) != (0, 0), b outer:  acc = acc + sample[(s j + b) w + s i + a]
//     pixel = acc * fl(1 / s^2)
// The order is part of the definition (another order changes bits), so both forms below add in exactly that order; this file is
// built with -ffp-contract=off like the rest of the library, so no addition is fused with the multiplication.
//
// A streaming kernel: 16 s^2 bytes read and 16, 4 or 3 bytes written per pixel. Two load patterns, selectable per launch:
//   resolve_lane_per_pixel   a lane owns a pixel and issues its s^2 16-byte loads itself. Neighbouring lanes are 16 s bytes apart:
//                            one load instruction of a wave touches s KiB and uses 1 / s of every line, the s loads of a sample
//                            row use the rest of the same lines.
//   resolve_lane_per_sample  a lane owns a sample COLUMN of a pixel row: every load instruction of a wave reads 1 KiB contiguous
//                            (1008 bytes for s = 3: 63 samples, so that triples stay inside the wave). The lane of the a = 0 column
//                            carries acc: its own sample of row b, then its neighbours' (lane + 1 .. lane + s - 1, fetched with a
//                            DPP row shift for s = 2 and 4, with __shfl_down for s = 3), then row b + 1. The other lanes only fetch.
// The byte outputs are fused: filter, then rt_pack.hip's quantisation in registers - the float pixel never travels.
#include "rt_resolve.h"
#include "hip_raytracer.h"

namespace rt {
namespace {

constexpr uint32_t kResolveBlock = 256;

// rt_pack.hip's byte, restated (that file stays as it is): floorf(v * 255.0f), NaN and negatives -> 0, 255 and up -> 255, branch-free
__device__ __forceinline__ uint32_t quantise(float v) {
    const float f = floorf(v * 255.0f);
    return (uint32_t)fminf(fmaxf(f, 0.0f), 255.0f);
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int S>
__device__ __forceinline__ float4 scale4(const float4 a) {
    constexpr float k = 1.0f / (float)(S * S);  // fl(1 / s^2): exact for 2 and 4, rounded once for 3
    return make_float4(a.x * k, a.y * k, a.z * k, a.w * k);
}

// pixel p of the output, in the output's form: 0 = float4, else an rt_pixel_format
template <int FORMAT>
__device__ __forceinline__ void store_pixel(void* __restrict__ dst, uint64_t p, const float4 v) {
    if (FORMAT == 0) {
        static_cast<float4*>(dst)[p] = v;
    } else if (FORMAT == RT_PIXEL_RGBA8) {
        static_cast<uint32_t*>(dst)[p] = quantise(v.x) | (quantise(v.y) << 8) | (quantise(v.z) << 16) | (quantise(v.w) << 24);
    } else {
        uint8_t* q = static_cast<uint8_t*>(dst) + 3 * p;
        q[0] = (uint8_t)quantise(v.x);
        q[1] = (uint8_t)quantise(v.y);
        q[2] = (uint8_t)quantise(v.z);
    }
}

// w: samples per row, pw = w / S pixels per row, n_pixels = pw * pixel rows (< 2^32: the launcher sees to it)
template <int S, int FORMAT>
__global__ __launch_bounds__(kResolveBlock) void resolve_lane_per_pixel(const float4* __restrict__ src, void* __restrict__ dst, uint32_t w,
                                                                        uint32_t pw, uint32_t n_pixels) {
    const uint64_t g = (uint64_t)blockIdx.x * kResolveBlock + threadIdx.x;
    if (g >= n_pixels) return;
    const uint32_t p = (uint32_t)g;
    const uint32_t j = p / pw, i = p - j * pw;
    const float4* q = src + (uint64_t)j * S * w + (uint64_t)i * S;
    float4 acc = q[0];
#pragma unroll
    for (int b = 0; b < S; ++b) {
#pragma unroll
        for (int a = 0; a < S; ++a)
            if (a | b) acc = add4(acc, q[(uint64_t)b * w + a]);
    }
    store_pixel<FORMAT>(dst, p, scale4<S>(acc));
}

// the value of lane + DELTA. S = 2, 4: a pixel's lanes share a DPP row of 16, so the fetch is a row_shl modifier (no LDS crossbar trip);
// S = 3: triples straddle rows, __shfl_down (ds_bpermute_b32)
template <int S, int DELTA>
__device__ __forceinline__ float lane_down(float v) {
    if (S == 3) return __shfl_down(v, DELTA);
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + DELTA, 0xf, 0xf, true));  // row_shl:DELTA
}
template <int S, int DELTA>
__device__ __forceinline__ float4 lane_down4(const float4 v) {
    return make_float4(lane_down<S, DELTA>(v.x), lane_down<S, DELTA>(v.y), lane_down<S, DELTA>(v.z), lane_down<S, DELTA>(v.w));
}

// a wave = kSpan consecutive samples of a pixel row's S sample rows; `chunks` waves per pixel row, `units` = pixel rows * chunks
template <int S, int FORMAT>
__global__ __launch_bounds__(kResolveBlock) void resolve_lane_per_sample(const float4* __restrict__ src, void* __restrict__ dst, uint32_t w,
                                                                         uint32_t pw, uint32_t chunks, uint32_t units) {
    constexpr uint32_t kSpan = 64 / S * S;  // 64, 63, 64: whole pixels only
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g = (uint64_t)blockIdx.x * (kResolveBlock / 64) + (threadIdx.x >> 6);
    if (g >= units) return;  // the whole wave leaves
    const uint32_t u = (uint32_t)g;
    const uint32_t j = u / chunks, c = u - j * chunks;
    const uint32_t x = c * kSpan + lane;
    const bool live = lane < kSpan && x < w;  // w is a multiple of S: a pixel is live or not as a whole
    const float4* q = src + (uint64_t)j * S * w + x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int b = 0; b < S; ++b) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = q[(uint64_t)b * w];
        acc = b == 0 ? v : add4(acc, v);
        // every lane fetches; only the a = 0 lanes' sums are used
        if (S > 1) acc = add4(acc, lane_down4<S, 1>(v));
        if (S > 2) acc = add4(acc, lane_down4<S, 2>(v));
        if (S > 3) acc = add4(acc, lane_down4<S, 3>(v));
    }
    if (live && lane % S == 0) store_pixel<FORMAT>(dst, (uint64_t)j * pw + x / S, scale4<S>(acc));
}

template <int S, int FORMAT>
hipError_t launch_one(const float4* src, uint32_t w, uint32_t rows, void* dst, hipStream_t stream, bool per_sample) {
    const uint32_t pw = w / S;
    const uint64_t n_pixels = (uint64_t)pw * (rows / S);
    if (n_pixels > 0xffffffffull) return hipErrorInvalidValue;
    if (per_sample) {
        constexpr uint32_t kSpan = 64 / S * S;
        const uint32_t chunks = (w + kSpan - 1) / kSpan;
        const uint64_t units = (uint64_t)chunks * (rows / S);
        if (units > 0xffffffffull) return hipErrorInvalidValue;
        const uint64_t blocks = (units + kResolveBlock / 64 - 1) / (kResolveBlock / 64);
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        hipLaunchKernelGGL((resolve_lane_per_sample<S, FORMAT>), dim3((uint32_t)blocks), dim3(kResolveBlock), 0, stream, src, dst, w, pw, chunks,
                           (uint32_t)units);
    } else {
        const uint64_t blocks = (n_pixels + kResolveBlock - 1) / kResolveBlock;
        hipLaunchKernelGGL((resolve_lane_per_pixel<S, FORMAT>), dim3((uint32_t)blocks), dim3(kResolveBlock), 0, stream, src, dst, w, pw,
                           (uint32_t)n_pixels);
    }
    return hipGetLastError();
}

template <int S>
hipError_t launch_factor(const float4* src, uint32_t w, uint32_t rows, int format, void* dst, hipStream_t stream, bool per_sample) {
    if (format == 0) return launch_one<S, 0>(src, w, rows, dst, stream, per_sample);
    if (format == RT_PIXEL_RGBA8) return launch_one<S, RT_PIXEL_RGBA8>(src, w, rows, dst, stream, per_sample);
    return launch_one<S, RT_PIXEL_RGB8>(src, w, rows, dst, stream, per_sample);
}

}  // namespace

hipError_t launch_resolve(const float4* src, uint32_t sample_width, uint32_t sample_rows, uint32_t s, int format, void* dst,
                          hipStream_t stream, int form) {
    if (s < 2 || s > 4 || (format != 0 && format != RT_PIXEL_RGBA8 && format != RT_PIXEL_RGB8)) return hipErrorInvalidValue;
    if (sample_width % s || sample_rows % s) return hipErrorInvalidValue;
    if (sample_width == 0 || sample_rows == 0) return hipSuccess;
    if (!src || !dst || (reinterpret_cast<uintptr_t>(src) & 15u) || (reinterpret_cast<uintptr_t>(dst) & (format ? 3u : 15u)))
        return hipErrorInvalidValue;
    // The measured choice (tools/ab/supersample_timing.py, profiles/supersample_timing.json; resident 4096^2
    // sample frame, best of 7, two processes): a lane per sample is 3 - 6 % faster for s = 2 (float 0.0566 against 0.0602 ms, RGBA8
    // 0.0443 / 0.0456) and for s = 4 (0.0398 / 0.0411, 0.0379 / 0.0395, RGB8 0.0376 / 0.0384); a lane per pixel is 2 % faster for
    // RGB8 at s = 2 (0.0396 / 0.0405: a sample lane's byte stores come from every second lane only) and for s = 3 the two tie on
    // float and RGBA8 (0.0444 / 0.0437, 0.0398 / 0.0398) and the lane per pixel wins RGB8 (0.0382 / 0.0393): the simpler form there.
    // (a row shorter than a wave goes a lane per pixel whatever the factor: a wave per row chunk would idle most of its lanes)
    const bool measured = sample_width >= 64 && (s == 4 || (s == 2 && format != RT_PIXEL_RGB8));
    const bool per_sample = form == kResolveAuto ? measured : form == kResolveLanePerSample;
    switch (s) {
        case 2: return launch_factor<2>(src, sample_width, sample_rows, format, dst, stream, per_sample);
        case 3: return launch_factor<3>(src, sample_width, sample_rows, format, dst, stream, per_sample);
        default: return launch_factor<4>(src, sample_width, sample_rows, format, dst, stream, per_sample);
    }
}

}  // namespace rt
