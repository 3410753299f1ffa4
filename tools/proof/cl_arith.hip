// Exhaustive check, on the GPU, of the RT_FLAG_DEVICE_OPENCL helpers of rt_device.h (cl_div, cl_sqrt, cl_rsq) against the
// compiler's own lowering of the same operations in a translation unit built WITHOUT -fhip-fp32-correctly-rounded-divide-sqrt,
// which is how ROCm's OpenCL compiler lowers the reference's `/` and sqrt() for gfx950 (and OCML's rsqrtf, which the OpenCL
// library's normalize() calls). The helpers are written with explicit builtins, so this file's flags do not change them.
//   sqrt, rsqrt, 1 / x: every one of the 2^32 inputs
//   a / b: every numerator for 1 024 denominators (both signs, every exponent of 0..255, two significands each), plus
//          random pairs (default 2^30) drawn with +-0, denormals, +-inf and NaN mixed in
// Results compare bit for bit; two NaNs count as equal (their payloads are not part of the contract).
// Build: hipcc -O3 --offload-arch=gfx950 -fno-hip-fp32-correctly-rounded-divide-sqrt -ffp-contract=off -I opencl-raytracer_amd/csrc tools/proof/cl_arith.hip -o tools/proof/cl_arith
// Run:   ./cl_arith [log2 of the number of random pairs, default 30]
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rt_device.h"

struct Tally {
    unsigned long long bad[4];   // sqrt, rsqrt, 1/x, a/b
    unsigned long long n[4];
    uint32_t first[4][2];
};

__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

__device__ __forceinline__ void note(Tally* t, int k, unsigned long long bad, unsigned long long n, uint32_t a, uint32_t b) {
    if (bad) { atomicAdd(&t->bad[k], bad); t->first[k][0] = a; t->first[k][1] = b; }
    atomicAdd(&t->n[k], n);
}

__global__ __launch_bounds__(256) void unary(uint32_t hi, Tally* out) {  // inputs hi << 16 | lo, lo in 0..65535
    const uint32_t x_bits = (hi << 16) | (blockIdx.x * 256u + threadIdx.x);
    const float x = __uint_as_float(x_bits);
    unsigned long long b0 = !same(rt::cl_sqrt(x), __builtin_sqrtf(x));
    unsigned long long b1 = !same(rt::cl_rsq(x), rsqrtf(x));
    unsigned long long b2 = !same(rt::cl_div(1.0f, x), 1.0f / x);
    const unsigned long long a0 = __ballot(b0), a1 = __ballot(b1), a2 = __ballot(b2);
    if ((threadIdx.x & 63u) == 0u) {
        note(out, 0, __popcll(a0), 64, x_bits, 0);
        note(out, 1, __popcll(a1), 64, x_bits, 0);
        note(out, 2, __popcll(a2), 64, x_bits, 0);
    }
}

__global__ __launch_bounds__(256) void divide_all(uint32_t b_bits, Tally* out) {  // every numerator for one denominator
    const float b = __uint_as_float(b_bits);
    unsigned long long bad = 0, n = 0;
    uint32_t fa = 0;
    for (uint64_t a = blockIdx.x * 256u + threadIdx.x; a < (1ull << 32); a += (uint64_t)gridDim.x * 256u) {
        const float x = __uint_as_float((uint32_t)a);
        ++n;
        if (!same(rt::cl_div(x, b), x / b)) { if (!bad) fa = (uint32_t)a; ++bad; }
    }
    note(out, 3, bad, n, fa, b_bits);
}

__device__ __forceinline__ uint32_t mix(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)(z ^ (z >> 31));
}
__device__ __forceinline__ float special(uint32_t r) {  // 1 in 8: a special value instead of the random bits
    const uint32_t s = r & 0x80000000u;
    switch ((r >> 3) & 7u) {
        case 0: return __uint_as_float(s);                              // +-0
        case 1: return __uint_as_float(s | (r & 0x007fffffu) | 1u);     // denormal
        case 2: return __uint_as_float(s | 0x7f800000u);                // inf
        case 3: return __uint_as_float(0x7fc00000u);                    // NaN
        case 4: return __uint_as_float(s | 0x00800000u);                // smallest normal
        case 5: return __uint_as_float(s | 0x7f7fffffu);                // largest finite
        default: return __uint_as_float(r);
    }
}
__global__ __launch_bounds__(256) void divide_random(uint64_t base, uint32_t per_thread, Tally* out) {
    const uint64_t gid = base + blockIdx.x * 256ull + threadIdx.x;
    unsigned long long bad = 0;
    uint32_t fa = 0, fb = 0;
    for (uint32_t k = 0; k < per_thread; ++k) {
        const uint64_t id = gid * per_thread + k;
        const uint32_t ra = mix(2 * id), rb = mix(2 * id + 1);
        const float a = (ra & 7u) == 0u ? special(ra) : __uint_as_float(ra);
        const float b = (rb & 7u) == 0u ? special(rb) : __uint_as_float(rb);
        if (!same(rt::cl_div(a, b), a / b)) { if (!bad) { fa = __float_as_uint(a); fb = __float_as_uint(b); } ++bad; }
    }
    note(out, 3, bad, per_thread, fa, fb);
}

int main(int argc, char** argv) {
    const int lg = argc > 1 ? atoi(argv[1]) : 30;
    Tally* d;
    if (hipMalloc(&d, sizeof(Tally)) != hipSuccess) return 2;
    hipMemset(d, 0, sizeof(Tally));
    for (uint32_t hi = 0; hi < 65536u; ++hi) hipLaunchKernelGGL(unary, dim3(256), dim3(256), 0, 0, hi, d);
    for (uint32_t e = 0; e < 256u; ++e)
        for (uint32_t m : {0u, 0x5a5a5au})
            for (uint32_t s : {0u, 0x80000000u}) hipLaunchKernelGGL(divide_all, dim3(4096), dim3(256), 0, 0, s | (e << 23) | m, d);
    const uint64_t pairs = 1ull << lg, per_thread = 256, threads = pairs / per_thread, per_launch = 1ull << 20;
    for (uint64_t t0 = 0; t0 < threads; t0 += per_launch)
        hipLaunchKernelGGL(divide_random, dim3((uint32_t)(per_launch / 256)), dim3(256), 0, 0, t0, (uint32_t)per_thread, d);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    Tally h;
    hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    const char* name[4] = {"sqrt", "rsqrt", "1/x", "a/b"};
    unsigned long long total = 0;
    for (int k = 0; k < 4; ++k) {
        printf("%-6s inputs %llu mismatches %llu (first %08x %08x)\n", name[k], h.n[k], h.bad[k], h.first[k][0], h.first[k][1]);
        total += h.bad[k];
    }
    printf("cl_arith: TOTAL mismatches %llu\n", total);
    return total ? 1 : 0;
}
