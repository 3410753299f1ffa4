// rt_query_device.h - what the query kernels share (rt_query.hip, rt_query_shade.hip): the per-ray route predicate, the ray sources,
// the workgroup shape and the once-per-wave counter flush - and, host side, what their launchers share: the arithmetic dispatch and the
// argument predicates. Included by the kernel units only (rt_gbuffer.hip with them).
#pragma once

#include <initializer_list>
#include <type_traits>

#include "rt_query.h"

namespace rt {

constexpr uint32_t kQueryBlock = 256;
constexpr uint64_t kQueryMaxBlocks = 1ull << 20;  // 2^28 rays per trip of the workgroups' loop; beyond that a workgroup takes further rays

__device__ __forceinline__ bool finite_(float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // (NaN: false)

__device__ __forceinline__ bool finite3(const Ray& r) {  // start.xyz and direction.xyz
    return finite_(r.sx) && finite_(r.sy) && finite_(r.sz) && finite_(r.dx) && finite_(r.dy) && finite_(r.dz);
}

// The per-ray route (hip_raytracer.h; rays.py: query_route is the executable definition), one predicate with two readers. BOX: the
// whole of it - the context's grid serves queries, the ray is inside the walks' domain (every component finite, start.w == 1,
// direction.w == 0, |d|^2 inside their window) and its origin inside the box. Without BOX the domain part alone: a PRIMARY ray of a
// shaded query that fails it makes its whole path literal (rt_query_shade.hip).
template <bool BOX>
__device__ __forceinline__ bool query_predicate(const QueryBox& b, const Ray& r) {
    if (BOX && !b.grid) return false;
    const bool finite = finite_(r.sx) && finite_(r.sy) && finite_(r.sz) && finite_(r.sw) && finite_(r.dx) && finite_(r.dy) &&
                        finite_(r.dz) && finite_(r.dw);
    const float dd = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;  // scan_rays' order; nothing contracted in these translation units
    const bool inside = !BOX || (r.sx >= b.lox && r.sx <= b.hix && r.sy >= b.loy && r.sy <= b.hiy && r.sz >= b.loz && r.sz <= b.hiz);
    return finite && r.sw == 1.0f && r.dw == 0.0f && dd > 1.0e-30f && dd < 1.0e30f && inside;
}
__device__ __forceinline__ bool query_on_grid(const QueryBox& b, const Ray& r) { return query_predicate<true>(b, r); }
__device__ __forceinline__ bool query_in_domain(const Ray& r) { return query_predicate<false>(QueryBox{}, r); }

// ray i of an array the kernel may also write (rt_query.hip: AliasedRays): a plain pointer
__device__ __forceinline__ Ray load_ray_aliased(const float4* rays, uint64_t i) {
    const float4 s = rays[2 * i];
    const float4 d = rays[2 * i + 1];
    Ray ray;
    ray.sx = s.x; ray.sy = s.y; ray.sz = s.z; ray.sw = s.w;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z; ray.dw = d.w;
    return ray;
}
__device__ __forceinline__ Ray load_ray(const float4* __restrict__ rays, uint64_t i) { return load_ray_aliased(rays, i); }

// work-item g's primary ray: the pinhole grid of rt_set_camera (rt_wavefront.hip: primary_ray) or the context's buffer
__device__ __forceinline__ Ray camera_ray(const QueryCamera& c, uint64_t g) {
    if (!c.pinhole) return load_ray(c.rays, g);
    const uint32_t gi = (uint32_t)g;
    const uint32_t row = gi / c.width;
    const uint32_t col = gi - row * c.width;
    Ray ray;
    ray.sx = 0.f; ray.sy = 0.f; ray.sz = 0.f; ray.sw = 1.f;
    ray.dx = (float)col - c.half_w;
    ray.dy = (c.height_f - (float)row) - c.half_h;
    ray.dz = c.z;
    ray.dw = 0.f;
    return ray;
}

struct WaveCount {
    unsigned long long rays = 0, grid = 0, tests = 0;  // rays / grid: wave-uniform (ballots); tests: this lane's
    __device__ __forceinline__ void route(bool active, bool on_grid) {
        rays += (unsigned long long)__popcll(__ballot(active));
        grid += (unsigned long long)__popcll(__ballot(active && on_grid));
    }
    // every lane of the wave arrives here (no lane returns early)
    __device__ __forceinline__ void flush(QueryCounters* __restrict__ out) {
        unsigned long long t = tests;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if ((threadIdx.x & 63u) == 0u && rays) {
            atomicAdd(&out->n_rays, rays);
            if (grid) atomicAdd(&out->n_grid, grid);
            if (rays - grid) atomicAdd(&out->n_brute, rays - grid);
            if (t) atomicAdd(&out->tests, t);
        }
    }
};

// (T, index) of the reference's loop for one ray, by the ray's route
template <int AM>
__device__ __forceinline__ void query_closest_one(const Scene& S, const GridDesc& g, bool on_grid, const Ray& ray, float& T, int& idx,
                                                  WaveCount& wc) {
    T = kMaxFloat;
    idx = -1;
    if (on_grid) {
        uint32_t tested = 0;
        closest_hit_grid<AM, true>(g, S.hot, ray, T, idx, tested);
        wc.tests += tested;
    } else {
        closest_hit<AM, false>(S.pairs, S.n_pairs, ray, T, idx);
        wc.tests += 2ull * S.n_pairs;
    }
}

// where a query's rays come from: the caller's buffer, or the context's own primary rays of a work-item list (rt_query_primary)
struct BufferRays {
    const float4* __restrict__ rays;
    __device__ __forceinline__ Ray operator()(uint64_t i) const { return load_ray(rays, i); }
};
struct PrimaryRays {
    QueryCamera cam;
    const uint64_t* __restrict__ items;
    __device__ __forceinline__ Ray operator()(uint64_t i) const { return camera_ray(cam, items[i]); }
};

inline dim3 query_blocks(uint64_t n) {
    const uint64_t blocks = (n + kQueryBlock - 1) / kQueryBlock;
    return dim3((uint32_t)(blocks < kQueryMaxBlocks ? blocks : kQueryMaxBlocks));
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0; }

// what every launcher that reads primary rays refuses of the camera
inline bool camera_refused(const QueryCamera& c) {
    return (!c.pinhole && (!c.rays || misaligned(c.rays, 16))) || (c.pinhole && c.width == 0);
}

// ... and of a set of outputs of which each may be null, not all: none given, or one misaligned
struct OutputPointer { const void* p; uintptr_t align; };
inline bool outputs_refused(std::initializer_list<OutputPointer> outputs) {
    bool any = false;
    for (const OutputPointer& o : outputs) {
        if (misaligned(o.p, o.align)) return true;
        any = any || o.p;
    }
    return !any;
}

// The run-time arithmetic mode as a compile-time constant: launch(std::integral_constant<int, kUnfused | kFused | kDeviceCL>) once.
template <class Launch>
hipError_t launch_for_arith(int arith, Launch&& launch) {
    switch (arith) {
        case kUnfused: launch(std::integral_constant<int, kUnfused>{}); break;
        case kFused: launch(std::integral_constant<int, kFused>{}); break;
        case kDeviceCL: launch(std::integral_constant<int, kDeviceCL>{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rt
