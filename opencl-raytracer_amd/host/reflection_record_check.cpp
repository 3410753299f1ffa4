// reflection_record_check - the 16-byte reflection record (csrc/rt_wavefront.hip: reflection_rays_rebuilt) on the host:
// no library, no GPU (tests/test_reflection_record_cpu.py).
//
//   reflection_record_check <n_hits> <seed>
//
// A frame that keeps the 16-byte record stores a reflection ray's direction and rebuilds its start from the stored hit
// point with reflection_origin(); the ray that left the hit came from reflection_ray(). For every arithmetic mode and
// n_hits seeded hits (among them zero reflection vectors, denormal, infinite and NaN components) the two starts must be
// the same words. Then the record's fourth word (reflection_word) must give back `bounces` and the self-test bit.
//
// rt_device.h is device code. It is compiled here for the host: its functions are made __host__ __device__, and the
// handful of gfx950 builtins it uses stand in as plain C (they need not round as the hardware does: both sides of the
// comparison go through the same stand-in, and what is checked is that both sides are the same computation).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
static inline float host_frexp_mant(float x) { int e; return std::frexp(x, &e); }
static inline int host_frexp_exp(float x) { int e; (void)std::frexp(x, &e); return e; }
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_rsqf(x) (1.0f / std::sqrt(x))
#define __builtin_amdgcn_sqrtf(x) (std::sqrt(x))
#define __builtin_amdgcn_frexp_mantf(x) host_frexp_mant(x)
#define __builtin_amdgcn_frexp_expf(x) host_frexp_exp(x)
#define __builtin_amdgcn_exp2f(x) (std::exp2(x))
#define __builtin_amdgcn_logf(x) (std::log2(x))
#include "rt_device.h"

namespace {

uint64_t rng_state;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffffu) * (1.0f / 16777216.0f); }

// one component of a given kind: 0 ordinary, 1 zero (either sign), 2 denormal, 3 NaN, 4 infinity, 5 any bit pattern, 6 huge, 7 tiny
float component(uint32_t kind) {
    switch (kind) {
        case 1: return from_bits(rnd() & 0x80000000u);
        case 2: return from_bits((rnd() & 0x80000000u) | (1u + (rnd() & 0x7ffffeu)));
        case 3: return from_bits(0x7fc00000u | (rnd() & 0x803fffffu));
        case 4: return from_bits((rnd() & 0x80000000u) | 0x7f800000u);
        case 5: return from_bits(rnd() ^ (rnd() << 16));
        case 6: return uniform(-1.f, 1.f) * 3.0e37f;
        case 7: return uniform(-1.f, 1.f) * 1.0e-30f;
        default: return uniform(-50.f, 50.f);
    }
}

template <int AM>
unsigned long long check_mode(uint32_t n_hits, const char* name) {
    unsigned long long bad = 0, nan_starts = 0;
    for (uint32_t k = 0; k < n_hits; ++k) {
        rt::HitRec h = {};
        // every eighth hit is ordinary throughout; the others draw a kind for the whole vector or per component
        const uint32_t plan = k & 7u;
        const uint32_t vec_kind = rnd() & 7u;
        float* r[3] = {&h.rx, &h.ry, &h.rz};
        float* p[3] = {&h.px, &h.py, &h.pz};
        for (int j = 0; j < 3; ++j) {
            *r[j] = component(plan == 0u ? 0u : (plan < 4u ? vec_kind : (rnd() & 7u)));
            *p[j] = component(plan == 7u ? (rnd() & 7u) : 0u);
        }
        if (k == 1u) { h.rx = 0.f; h.ry = 0.f; h.rz = 0.f; }       // the zero vector itself, both signs
        if (k == 2u) { h.rx = -0.f; h.ry = 0.f; h.rz = -0.f; }
        h.pw = 1.0f;
        h.index = (int)(rnd() & 0xffffu);
        rt::Ray ray;
        rt::reflection_ray<AM>(h, ray);
        float sx, sy, sz;
        rt::reflection_origin<AM>(h.px, h.py, h.pz, ray.dx, ray.dy, ray.dz, sx, sy, sz);  // (from the DIRECTION, as a reader of the record has it)
        // ... and the start written out as the reference has it: intersection + 0.001 * normalize(reflection)
        float nx = h.rx, ny = h.ry, nz = h.rz;
        rt::normalize3_<AM>(nx, ny, nz);
        const float wx = rt::fma_<AM>(nx, 0.001f, h.px), wy = rt::fma_<AM>(ny, 0.001f, h.py), wz = rt::fma_<AM>(nz, 0.001f, h.pz);
        const bool same = bits(sx) == bits(ray.sx) && bits(sy) == bits(ray.sy) && bits(sz) == bits(ray.sz) &&
                          bits(wx) == bits(ray.sx) && bits(wy) == bits(ray.sy) && bits(wz) == bits(ray.sz) &&
                          bits(ray.sw) == bits(1.0f) && bits(ray.dw) == 0u &&
                          bits(ray.dx) == bits(h.rx) && bits(ray.dy) == bits(h.ry) && bits(ray.dz) == bits(h.rz);
        if (!same) {
            if (bad < 5) std::printf("%s: hit %u: start %08x %08x %08x, rebuilt %08x %08x %08x\n", name, k, bits(ray.sx), bits(ray.sy), bits(ray.sz), bits(sx), bits(sy), bits(sz));
            ++bad;
        }
        if (sx != sx || sy != sy || sz != sz) ++nan_starts;
    }
    std::printf("%s hits %u nan_starts %llu mismatches %llu\n", name, n_hits, nan_starts, bad);
    return bad;
}

unsigned long long check_words() {
    unsigned long long bad = 0;
    const uint32_t bounces[] = {0u, 1u, 5u, 0x7fffffffu};
    for (uint32_t b : bounces)
        for (int self = 0; self < 2; ++self) {
            const uint32_t word = rt::reflection_word(self != 0, b);
            if (rt::reflection_word_bounces(word) != b || rt::reflection_word_self_hit(word) != (self != 0)) {
                std::printf("word: bounces %u self %d -> %08x -> bounces %u self %d\n", b, self, word, rt::reflection_word_bounces(word), (int)rt::reflection_word_self_hit(word));
                ++bad;
            }
        }
    // a count that does not fit must not reach the self-test bit
    if (rt::reflection_word_self_hit(rt::reflection_word(false, 0xffffffffu))) ++bad;
    std::printf("words mismatches %llu\n", bad);
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: reflection_record_check <n_hits> <seed>\n"); return 2; }
    const uint32_t n_hits = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    rng_state = std::strtoull(argv[2], nullptr, 10);
    unsigned long long bad = 0;
    bad += check_mode<rt::kUnfused>(n_hits, "unfused");
    bad += check_mode<rt::kFused>(n_hits, "fused");
    bad += check_mode<rt::kDeviceCL>(n_hits, "device_opencl");
    bad += check_words();
    return bad ? 1 : 0;
}
