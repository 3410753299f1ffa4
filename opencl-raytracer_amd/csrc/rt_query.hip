// rt_query.hip - ray queries (hip_raytracer.h): closest hit and occlusion for arbitrary rays on a live context.
//
// The walks are the ones the frames are tested with (rt_grid.h: closest_hit_grid, any_hit_grid; rt_device.h: closest_hit); what is
// new here is only who feeds them. One thread per ray, 256 per workgroup. Each lane decides the route of ITS ray (query_on_grid):
// the grid serves a ray whose components are all finite, with start.w == 1, direction.w == 0, |d|^2 inside the walks' window and
// its origin inside the box the grid's radii were derived for; every other ray runs the ordered loop over the pair stream, which
// is the reference's loop in the reference's order (NaN rays included: no closed form is consulted). The pair stream arrives through
// wave-uniform scalar loads, so the brute-force lanes of one wave share one pass over it - while the wave's grid lanes wait: a
// brute-force ray costs n_objs tests and serialises its wave. That is the price of never refusing a ray and never approximating one.
//
// Counters: once per wave, one lane adds the wave's rays per route (from ballots) and its exact tests (a wave sum) to the
// context's QueryCounters with vector atomics.
#include "rt_query_device.h"

namespace rt {
namespace {

// t: the loop's value; index: the hittest rule of rt_set_aux_device - the winner where t < MAX_FLOAT, else -1
__device__ __forceinline__ void store_closest(float* __restrict__ t, int32_t* __restrict__ index, uint64_t i, float T, int idx) {
    if (t) t[i] = T;
    if (index) index[i] = (T < kMaxFloat) ? idx : -1;
}

// The one body of the three kernels. A workgroup takes 256 consecutive rays per trip (the trip count is wave-uniform, no lane leaves
// early: WaveCount::flush needs the whole wave); each lane routes its own ray. OCCLUDED: one byte per ray - any_hit_grid on the
// grid, the reference's shadow predicate (shade_and_reflect_kernel.cl:229; a NaN reads occluded) on the ordered loop's time off it;
// else t and index as two coalesced 4-byte stores.
template <int AM, bool OCCLUDED, class RAYS>
__device__ __forceinline__ void query_body(const Scene& S, const GridDesc& g, const QueryBox& box, const RAYS& rays, uint64_t n,
                                           float* __restrict__ t, int32_t* __restrict__ index, uint8_t* __restrict__ occluded,
                                           QueryCounters* __restrict__ counters) {
    WaveCount wc;
    const uint64_t stride = (uint64_t)gridDim.x * kQueryBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kQueryBlock; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool active = i < n;
        bool on_grid = false;
        if (active) {
            const Ray ray = rays(i);
            on_grid = query_on_grid(box, ray);
            if (OCCLUDED && on_grid) {
                uint32_t tested = 0;
                const bool blocked = any_hit_grid<AM>(g, S, ray, tested);
                wc.tests += tested;
                occluded[i] = blocked ? (uint8_t)1 : (uint8_t)0;
            } else {
                float T;
                int idx;
                query_closest_one<AM>(S, g, on_grid, ray, T, idx, wc);
                if constexpr (OCCLUDED) occluded[i] = !(T >= 1.f || T < 0.f) ? (uint8_t)1 : (uint8_t)0;
                else store_closest(t, index, i, T, idx);
            }
        }
        wc.route(active, on_grid);
    }
    wc.flush(counters);
}

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void query_closest(const Scene S, const GridDesc g, const QueryBox box,
                                                             const float4* __restrict__ rays, uint64_t n, float* __restrict__ t,
                                                             int32_t* __restrict__ index, QueryCounters* __restrict__ counters) {
    query_body<AM, false>(S, g, box, BufferRays{rays}, n, t, index, nullptr, counters);
}

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void query_primary(const Scene S, const GridDesc g, const QueryBox box, const QueryCamera cam,
                                                             const uint64_t* __restrict__ items, uint64_t n, float* __restrict__ t,
                                                             int32_t* __restrict__ index, QueryCounters* __restrict__ counters) {
    query_body<AM, false>(S, g, box, PrimaryRays{cam, items}, n, t, index, nullptr, counters);
}

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void query_occluded(const Scene S, const GridDesc g, const QueryBox box,
                                                              const float4* __restrict__ rays, uint64_t n, uint8_t* __restrict__ occluded,
                                                              QueryCounters* __restrict__ counters) {
    query_body<AM, true>(S, g, box, BufferRays{rays}, n, nullptr, nullptr, occluded, counters);
}

// ---- hit records (hip_raytracer.h, "hit-record queries") -------------------------------------------------------------------------
// The closest-hit query with what raycast() leaves in the HitRecord of the winner: the same route decision and the same walks, then -
// where T < MAX_FLOAT - materialise<AM>() and reflection_ray<AM>() as the frames call them (but for the affine shortcut of a ray with
// an inf or a NaN in it, below). A ray whose mask entry is negative is not
// traced and reads as a miss (T = MAX_FLOAT, index -1): it enters no counter. A miss's records are all-zero bytes. Each record leaves
// as one 16-byte store per lane (two for the reflected ray). A lane reads ray i and mask[i] before it writes anything of element i
// and touches no other element, so `reflected` may be the ray array and `index` the mask: the caller's rays are loaded through
// AliasedRays, and no pointer on the way from the kernel's parameters to a load or store of rays, mask or outputs is __restrict__.
struct AliasedRays {  // BufferRays for an array the kernel may also write (out.reflected == rays): plain pointers throughout
    const float4* rays;
    __device__ __forceinline__ Ray operator()(uint64_t i) const { return load_ray_aliased(rays, i); }
};

template <int AM, class RAYS>
__device__ __forceinline__ void query_hits_body(const Scene& S, const GridDesc& g, const QueryBox& box, const RAYS& rays, uint64_t n,
                                                const int32_t* mask, const QueryHits& out, QueryCounters* __restrict__ counters) {
    WaveCount wc;
    const uint64_t stride = (uint64_t)gridDim.x * kQueryBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kQueryBlock; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        bool active = false, on_grid = false;
        if (i < n) {
            const Ray ray = rays(i);
            active = mask ? (mask[i] >= 0) : true;
            float T = kMaxFloat;
            int idx = -1;
            if (active) {
                on_grid = query_on_grid(box, ray);
                query_closest_one<AM>(S, g, on_grid, ray, T, idx, wc);
            }
            float4 P = make_float4(0.f, 0.f, 0.f, 0.f), N = P, RS = P, RD = P;
            if (T < kMaxFloat) {
                HitRec h;
                // the frames' call; the affine shortcut (w taken from the ray) is the reference's 0*x + 0*y + 0*z + 1*w only for
                // finite x, y, z, and a query's brute-force rays may hold an inf or a NaN: those fetch the bottom rows
                materialise<AM>(S.objrec, S.cold, idx, T, ray, h, S.affine != 0u && finite3(ray));
                Ray r;
                reflection_ray<AM>(h, r);
                P = make_float4(h.px, h.py, h.pz, h.pw);
                N = make_float4(h.nx, h.ny, h.nz, 0.f);
                RS = make_float4(r.sx, r.sy, r.sz, r.sw);
                RD = make_float4(r.dx, r.dy, r.dz, r.dw);
            }
            if (out.t) out.t[i] = T;
            if (out.index) out.index[i] = (T < kMaxFloat) ? idx : -1;  // (store_closest's rule, through pointers that may alias)
            if (out.point) out.point[i] = P;
            if (out.normal) out.normal[i] = N;
            if (out.reflected) {
                out.reflected[2 * i] = RS;
                out.reflected[2 * i + 1] = RD;
            }
        }
        wc.route(active, on_grid);
    }
    wc.flush(counters);
}

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void query_hits(const Scene S, const GridDesc g, const QueryBox box, const float4* rays, uint64_t n,
                                                          const int32_t* mask, const QueryHits out, QueryCounters* __restrict__ counters) {
    query_hits_body<AM>(S, g, box, AliasedRays{rays}, n, mask, out, counters);
}

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void query_primary_hits(const Scene S, const GridDesc g, const QueryBox box, const QueryCamera cam,
                                                                  const uint64_t* __restrict__ items, uint64_t n, const QueryHits out,
                                                                  QueryCounters* __restrict__ counters) {
    query_hits_body<AM>(S, g, box, PrimaryRays{cam, items}, n, nullptr, out, counters);
}

}  // namespace

hipError_t launch_query_closest(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays,
                                uint64_t n, float* d_t, int32_t* d_index, QueryCounters* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_rays || misaligned(d_rays, 16) || outputs_refused({{d_t, 4}, {d_index, 4}}) || !d_counters) return hipErrorInvalidValue;
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((query_closest<am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, d_rays, n, d_t, d_index, d_counters);
    });
}

hipError_t launch_query_occluded(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays,
                                 uint64_t n, uint8_t* d_occluded, QueryCounters* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_rays || misaligned(d_rays, 16) || !d_occluded || !d_counters) return hipErrorInvalidValue;
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((query_occluded<am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, d_rays, n, d_occluded, d_counters);
    });
}

hipError_t launch_query_primary(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const QueryCamera& camera,
                                const uint64_t* d_items, uint64_t n, float* d_t, int32_t* d_index, QueryCounters* d_counters,
                                hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_items || misaligned(d_items, 8) || outputs_refused({{d_t, 4}, {d_index, 4}}) || !d_counters || camera_refused(camera))
        return hipErrorInvalidValue;
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((query_primary<am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, camera, d_items, n, d_t, d_index, d_counters);
    });
}

namespace {
bool hits_refused(const QueryHits& o) {
    return outputs_refused({{o.t, 4}, {o.index, 4}, {o.point, 16}, {o.normal, 16}, {o.reflected, 16}});
}
}  // namespace

hipError_t launch_query_hits(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays, uint64_t n,
                             const int32_t* d_mask, const QueryHits& out, QueryCounters* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_rays || misaligned(d_rays, 16) || misaligned(d_mask, 4) || hits_refused(out) || !d_counters) return hipErrorInvalidValue;
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((query_hits<am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, d_rays, n, d_mask, out, d_counters);
    });
}

hipError_t launch_query_primary_hits(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const QueryCamera& camera,
                                     const uint64_t* d_items, uint64_t n, const QueryHits& out, QueryCounters* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_items || misaligned(d_items, 8) || hits_refused(out) || !d_counters || camera_refused(camera)) return hipErrorInvalidValue;
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((query_primary_hits<am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, camera, d_items, n, out, d_counters);
    });
}

}  // namespace rt
