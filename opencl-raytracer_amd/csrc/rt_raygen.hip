// rt_raygen.hip - the posed-grid generator: one streaming pass that writes the rays of rays.posed_rays, nothing read.
//
// The pinhole grid (W, H, z) - direction (i - W/2, (H - j) - H/2, z) for work-item j W + i, camera.grid_rays - with every direction
// multiplied by an fp32 3 x 3 matrix M and every start set to one origin (a panned, tilted, rolled or moved camera). Per ray, in
// fp32, every product and sum rounded, nothing fused, left to right (rays.posed_rays is the definition):
//   x = fl(i) - fl(W/2);  y = (fl(H) - fl(j)) - fl(H/2)
//   direction[r] = (M[r][0] * x + M[r][1] * y) + M[r][2] * z,  direction.w = 0,  start = (origin, 1)
// The roundings are spelled with __fmul_rn / __fadd_rn, which the compiler never contracts (the unit is built with
// -ffp-contract=off like the others all the same). 32 bytes written per ray: the kernel is bound by the write. A lane takes ray
// after ray in a grid-stride loop, two 16-byte stores each (a wave writes 2 KiB contiguous per trip, the mirror of the ray scan's
// reads). M, the origin, W/2, H/2 and z are kernel arguments, the same for every lane. A lane keeps its (row, column) beside the
// linear index and advances them by the stride's quotient and remainder by W - one 32-bit division per lane before the loop, none
// per ray; W and H are at most 2^24, so fl(i) and fl(j) are exact.
// The same loop with kStore = false stores no ray and reduces the ray scan's direction predicate instead (rt_rays.hip):
//   dd = (dx*dx + dy*dy) + dz*dz;  dd > 1e-30f && dd < 1e30f  (a NaN fails)      else kRayDomain
// across the wave with xor-shuffles, across the workgroup through LDS, one atomic OR per workgroup that found such a ray.
#include "rt_raygen.h"

namespace rt {
namespace {

constexpr uint32_t kGenBlock = 256;
constexpr uint32_t kGenWaves = kGenBlock / 64;
// as the ray scan: 1024 workgroups of four waves, 8 MiB of stores per trip of the whole launch; a larger grid takes further trips
constexpr uint32_t kGenMaxBlocks = 1024;

struct PoseArgs {
    PoseGrid g;
    float half_w, half_h, height_f;
    uint32_t step_rows, step_cols;  // the launch's stride (workgroups x kGenBlock rays) = step_rows * width + step_cols
};

template <bool kStore>
__global__ __launch_bounds__(kGenBlock) void pose_rays(float4* __restrict__ rays, PoseArgs a, RayScan* __restrict__ result) {
    const uint32_t W = a.g.width, H = a.g.height;
    const uint32_t first = blockIdx.x * kGenBlock + threadIdx.x;  // < kGenMaxBlocks * kGenBlock
    uint32_t row = first / W, col = first - row * W;
    uint64_t i = first;
    const uint64_t stride = (uint64_t)gridDim.x * kGenBlock;
    const float4 start = make_float4(a.g.origin[0], a.g.origin[1], a.g.origin[2], 1.0f);
    const float mz[3] = {__fmul_rn(a.g.m[2], a.g.z), __fmul_rn(a.g.m[5], a.g.z), __fmul_rn(a.g.m[8], a.g.z)};
    uint32_t flags = 0u;
    while (row < H) {
        const float x = __fsub_rn((float)col, a.half_w);
        const float y = __fsub_rn(__fsub_rn(a.height_f, (float)row), a.half_h);
        float d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            d[r] = __fadd_rn(__fadd_rn(__fmul_rn(a.g.m[3 * r], x), __fmul_rn(a.g.m[3 * r + 1], y)), mz[r]);
        if (kStore) {
            rays[2 * i] = start;
            rays[2 * i + 1] = make_float4(d[0], d[1], d[2], 0.0f);
        } else {
            const float dd = __fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2]));
            if (!(dd > 1.0e-30f && dd < 1.0e30f)) flags |= kRayDomain;
        }
        i += stride;
        row += a.step_rows;
        col += a.step_cols;  // < 2 W <= 2^25
        if (col >= W) { col -= W; ++row; }
    }
    if (kStore) return;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) flags |= (uint32_t)__shfl_xor((int)flags, m, 64);
    __shared__ uint32_t part[kGenWaves];
    if (threadIdx.x % 64u == 0u) part[threadIdx.x / 64u] = flags;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t v = part[0];
#pragma unroll
        for (uint32_t w = 1; w < kGenWaves; ++w) v |= part[w];
        if (v != 0u) atomicOr(&result->flags, v);
    }
}

bool pose_args(const PoseGrid& g, PoseArgs& a, uint32_t& blocks) {
    const uint64_t n = (uint64_t)g.width * g.height;
    if (n == 0) return false;
    const uint64_t want = (n + kGenBlock - 1) / kGenBlock;
    blocks = (uint32_t)(want < kGenMaxBlocks ? want : kGenMaxBlocks);
    const uint32_t stride = blocks * kGenBlock;
    a.g = g;
    a.half_w = (float)g.width / 2.0f;
    a.half_h = (float)g.height / 2.0f;
    a.height_f = (float)g.height;
    a.step_rows = stride / g.width;
    a.step_cols = stride % g.width;
    return true;
}

}  // namespace

hipError_t launch_pose_rays(const PoseGrid& g, float4* d_rays, hipStream_t stream) {
    if (g.width > 0x1000000u || g.height > 0x1000000u) return hipErrorInvalidValue;
    PoseArgs a;
    uint32_t blocks = 0;
    if (!pose_args(g, a, blocks)) return hipSuccess;
    if (!d_rays || (reinterpret_cast<uintptr_t>(d_rays) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_rays<true>, dim3(blocks), dim3(kGenBlock), 0, stream, d_rays, a, static_cast<RayScan*>(nullptr));
    return hipGetLastError();
}

hipError_t launch_pose_verdict(const PoseGrid& g, RayScan* d_result, hipStream_t stream) {
    if (!d_result || g.width > 0x1000000u || g.height > 0x1000000u) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_result, 0, sizeof(RayScan), stream);
    PoseArgs a;
    uint32_t blocks = 0;
    if (e != hipSuccess || !pose_args(g, a, blocks)) return e;
    hipLaunchKernelGGL(pose_rays<false>, dim3(blocks), dim3(kGenBlock), 0, stream, static_cast<float4*>(nullptr), a, d_result);
    return hipGetLastError();
}

}  // namespace rt
