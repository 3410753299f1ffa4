// rt_query_shade.hip - shaded queries (hip_raytracer.h): the colour along arbitrary rays on a live context.
//
// One thread per ray, 256 per workgroup, the workgroup loop and the once-per-wave counter flush of rt_query.hip. A lane runs the
// reference's per-pixel program - the functions the frames are tested with: materialise, shade_forward / shade_assign,
// shade_and_reflect_pixel with its bounce loop, reflection_ray (rt_device.h) - with RouteTracer in place of the small-scene
// traversal: EVERY ray of the path, primary, shadow or reflection, is routed by query_on_grid (rt_query_device.h), to the grid walks
// or to the ordered loop over the pair stream. A path is literal - shade_forward, closest-hit shadow tests, no dead-ray elimination -
// when the context is (Scene::literal as the host fills it) or when its primary ray fails query_in_domain: what a fresh context does
// for the whole frame when one such ray is in its buffer. The lane carries that decision in its own copy of Scene::literal; the
// rest of the Scene stays in scalar registers.
//
// Nothing here is wave-uniform but the trip count: lanes of one wave are in different bounces, different lights and on different
// routes. The loops this leans on were read for that:
//  * closest_hit / any_hit_before_one fetch the pair stream through wave-uniform scalar loads and touch it ahead with a clamped
//    vector load (l2_warm): both are defined for any set of active lanes.
//  * any_hit_before_one leaves when `__ballot(!occluded) == 0`. A ballot counts ACTIVE lanes only, so inside divergent control it
//    says "every lane that is in this loop now has its occluder"; the lanes that are elsewhere neither vote nor are affected. The
//    exit is uniform over the lanes that run the loop, which is all the scalar branch needs, and it only ever skips pairs whose
//    result could not change a lane's answer (occluded is an OR). The same holds for the odd pair's ballot behind the loop.
//  * closest_hit_grid / any_hit_grid are per-lane walks (wf_finish runs them one thread per ray).
#include "rt_query_device.h"

namespace rt {
namespace {

// The tracer of the shading functions (rt_device.h: SmallSceneTracer is the frames'): each ray by its own route. Secondary rays have
// direction.w == 0 by construction (shadow_ray_to, reflection_ray), hence DW0 = true on both routes, as in the frames.
struct RouteTracer {
    const GridDesc* g;
    const QueryBox* box;
    unsigned long long* tests;
    template <int AM>
    __device__ __forceinline__ void closest(const Scene& S, const Ray& ray, float& T, int& idx) const {
        if (query_on_grid(*box, ray)) {
            uint32_t tested = 0;
            closest_hit_grid<AM, true>(*g, S.hot, ray, T, idx, tested);
            *tests += tested;
        } else {
            closest_hit<AM, true>(S.pairs, S.n_pairs, ray, T, idx);
            *tests += 2ull * S.n_pairs;
        }
    }
    template <int AM>
    __device__ __forceinline__ bool any(const Scene& S, const Ray& ray) const {
        if (query_on_grid(*box, ray)) {
            uint32_t tested = 0;
            const bool blocked = any_hit_grid<AM>(*g, S, ray, tested);
            *tests += tested;
            return blocked;
        }
        uint32_t visited = 0;
        const bool blocked = any_hit_before_one<AM>(S.pairs, S.n_pairs, ray, &visited);
        *tests += 2ull * visited;
        return blocked;
    }
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// KERNEL: 1 shade_kernel.cl, 2 shade_and_reflect_kernel.cl - render_pixels' numbering (rt_kernels.hip), and its rules for a hit
// (:167 `t < MAX_FLOAT` / :173 `!(t == MAX_FLOAT)`: a NaN time is a hit of kernel 2 only), the background pixel and the aux pair.
template <int KERNEL, int AM>
__global__ __launch_bounds__(kQueryBlock) void query_shade(const Scene S, const GridDesc g, const QueryBox box, uint32_t max_bounces,
                                                           const float4* __restrict__ rays, const QueryCamera cam,
                                                           const uint64_t* __restrict__ items, uint64_t n, const int32_t* __restrict__ mask,
                                                           const QueryShade out, QueryShadeCounters* __restrict__ counters) {
    WaveCount wc;
    Counters ctr = {};
    unsigned long long n_literal = 0;  // wave-uniform (ballots)
    const uint64_t stride = (uint64_t)gridDim.x * kQueryBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kQueryBlock; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        bool active = false, on_grid = false, literal = false;
        if (i < n) {
            active = mask ? (mask[i] >= 0) : true;
            float outr = 0.f, outg = 0.f, outb = 0.f;
            float T = kMaxFloat;
            int idx = -1;
            bool hit = false;
            if (active) {
                const Ray ray = items ? camera_ray(cam, items[i]) : load_ray(rays, i);
                on_grid = query_on_grid(box, ray);
                literal = S.literal != 0u || !query_in_domain(ray);
                query_closest_one<AM>(S, g, on_grid, ray, T, idx, wc);
                hit = (KERNEL == 2) ? !(T == kMaxFloat) : (T < kMaxFloat);
                ctr.traced += 1;
                ctr.reference += 1;
                ctr.hits += hit ? 1 : 0;
                if (hit) {
                    Scene L = S;
                    L.literal = literal ? 1u : 0u;
                    const RouteTracer tracer{&g, &box, &wc.tests};
                    HitRec h;
                    materialise<AM>(S.objrec, S.cold, idx, T, ray, h, S.affine != 0u);  // (the frames' call: render_pixels)
                    if constexpr (KERNEL == 1) shade_forward<AM, true, true>(L, h, outr, outg, outb, ctr, tracer);
                    else shade_and_reflect_pixel<AM, true>(L, max_bounces, h, outr, outg, outb, ctr, tracer);
                }
            }
            if (out.rgba) out.rgba[i] = make_float4(outr, outg, outb, 1.0f);  // a miss: the reference's upload-time pixel {0,0,0,1}
            if (out.t) out.t[i] = T;
            if (out.index) out.index[i] = hit ? idx : -1;
        }
        wc.route(active, on_grid);
        n_literal += (unsigned long long)__popcll(__ballot(active && literal));
    }
    wc.flush(&counters->q);
    const unsigned long long a = wave_sum64(ctr.traced), b = wave_sum64(ctr.reference), c = wave_sum64(ctr.hits);
    if ((threadIdx.x & 63u) == 0u && wc.rays) {
        if (n_literal) atomicAdd(&counters->n_literal, n_literal);
        if (c) atomicAdd(&counters->hits, c);
        atomicAdd(&counters->traced, a);
        atomicAdd(&counters->reference, b);
    }
}

}  // namespace

hipError_t launch_query_shade(const Scene& scene, const GridDesc& grid, const QueryBox& box, int kernel, int arith, uint32_t max_bounces,
                              const float4* d_rays, const QueryCamera& camera, const uint64_t* d_items, uint64_t n, const int32_t* d_mask,
                              const QueryShade& out, QueryShadeCounters* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (outputs_refused({{out.rgba, 16}, {out.t, 4}, {out.index, 4}}) || misaligned(d_mask, 4) || !d_counters) return hipErrorInvalidValue;
    if (d_items) {
        if (misaligned(d_items, 8) || camera_refused(camera)) return hipErrorInvalidValue;
    } else if (!d_rays || misaligned(d_rays, 16)) {
        return hipErrorInvalidValue;
    }
    const auto launch = [&](auto k) {
        return launch_for_arith(arith, [&](auto am) {
            hipLaunchKernelGGL((query_shade<decltype(k)::value, am()>), query_blocks(n), dim3(kQueryBlock), 0, stream, scene, grid, box, max_bounces, d_rays, camera, d_items, n, d_mask, out, d_counters);
        });
    };
    switch (kernel) {
        case 1: return launch(std::integral_constant<int, 1>{});
        case 2: return launch(std::integral_constant<int, 2>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rt
