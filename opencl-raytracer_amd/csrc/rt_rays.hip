// rt_rays.hip - the ray scan: one streaming pass over a device-resident ray array, eight words out.
//
// rt_create decides from three predicates over the uploaded rays, and from the box of their origins, which path renders a
// frame: the default path (grid, exact eliminations), the literal loops or brute force. Its host loops are single-threaded;
// for rays that already live in device memory (rt_set_rays_device) the same predicates are a reduction here. Per ray, in
// fp32, nothing contracted (the translation unit is built with -ffp-contract=off), left to right, as rt_api.cpp and rt_context.h state them:
//   direction.w == 0.0f                                                          else kRayDirW
//   dd = (dx*dx + dy*dy) + dz*dz;  dd > 1e-30f && dd < 1e30f  (a NaN fails)      else kRayDomain   (direction_in_domain)
//   start.w == 1.0f && isfinite((sx + sy) + sz)                                  else kRayStart
//   the minimum and maximum of start.x, .y, .z as NUMBERS, taken on integer keys of the bits (rt_rays.h: ray_key)
// 32 bytes read per ray, nothing written but the result: the kernel is bound by the read. A lane takes ray after ray in a
// grid-stride loop, two 16-byte loads each (a wave reads 2 KiB contiguous per trip); its partial result is combined across the
// wave with xor-shuffles, across the workgroup's four waves through LDS, and one lane per workgroup issues seven atomics (an
// OR, six unsigned maxima). Everything is order-free, so the result does not depend on the launch shape or the schedule.
#include "rt_rays.h"

namespace rt {
namespace {

constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanWaves = kScanBlock / 64;
// 1024 workgroups of four waves: half of what 256 CUs hold at full occupancy, 8 MiB of loads in flight; a larger array is
// walked in further trips of the grid-stride loop
constexpr uint32_t kScanMaxBlocks = 1024;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(kScanBlock) void scan_rays(const float4* __restrict__ rays, uint64_t n, RayScan* __restrict__ result) {
    uint32_t flags = 0u;
    uint32_t lo_inv[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    const uint64_t stride = (uint64_t)gridDim.x * kScanBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x; i < n; i += stride) {
        const float4 s = rays[2 * i];
        const float4 d = rays[2 * i + 1];
        if (!(d.w == 0.0f)) flags |= kRayDirW;
        const float dd = (d.x * d.x + d.y * d.y) + d.z * d.z;
        if (!(dd > 1.0e-30f && dd < 1.0e30f)) flags |= kRayDomain;
        if (!(s.w == 1.0f) || !isfinite((s.x + s.y) + s.z)) flags |= kRayStart;
        const uint32_t k[3] = {ray_key(__float_as_uint(s.x)), ray_key(__float_as_uint(s.y)), ray_key(__float_as_uint(s.z))};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo_inv[a] = umax(lo_inv[a], ~k[a]);
            hi[a] = umax(hi[a], k[a]);
        }
    }
    // across the wave (lanes that met no ray carry the identity)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        flags |= (uint32_t)__shfl_xor((int)flags, m, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo_inv[a] = umax(lo_inv[a], (uint32_t)__shfl_xor((int)lo_inv[a], m, 64));
            hi[a] = umax(hi[a], (uint32_t)__shfl_xor((int)hi[a], m, 64));
        }
    }
    // across the workgroup, then one set of atomics
    __shared__ uint32_t part[kScanWaves][7];
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (lane == 0u) {
        part[wave][0] = flags;
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[wave][1 + a] = lo_inv[a]; part[wave][4 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 7u) {
        const uint32_t j = threadIdx.x;
        uint32_t v = part[0][j];
#pragma unroll
        for (uint32_t w = 1; w < kScanWaves; ++w) v = j == 0u ? (v | part[w][j]) : umax(v, part[w][j]);
        uint32_t* out = reinterpret_cast<uint32_t*>(result) + j;  // flags, lo_inv[3], hi[3]: the record's first seven words
        if (v != 0u) {  // (0 is the identity of both operations)
            if (j == 0u) atomicOr(out, v);
            else atomicMax(out, v);
        }
    }
}

}  // namespace

hipError_t launch_ray_scan(const float4* d_rays, uint64_t n, RayScan* d_result, hipStream_t stream) {
    static_assert(sizeof(RayScan) == 32 && offsetof(RayScan, lo_inv) == 4 && offsetof(RayScan, hi) == 16, "the kernel addresses the record by word");
    if (!d_result || (n && !d_rays) || (reinterpret_cast<uintptr_t>(d_rays) & 15u)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_result, 0, sizeof(RayScan), stream);
    if (e != hipSuccess || n == 0) return e;
    const uint64_t blocks = (n + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(scan_rays, dim3((uint32_t)(blocks < kScanMaxBlocks ? blocks : kScanMaxBlocks)), dim3(kScanBlock), 0, stream, d_rays, n,
                       d_result);
    return hipGetLastError();
}

}  // namespace rt
