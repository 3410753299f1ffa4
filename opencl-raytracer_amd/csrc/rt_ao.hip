// rt_ao.hip - ambient-occlusion frames (hip_raytracer.h): K occlusion rays per item of a G-buffer, traced and counted in one kernel.
//
// One lane per (item, sample): with K = samples a wave covers 64 / K consecutive items, lane l takes item base + l / K and sample
// l % K; 256 lanes per workgroup, workgroups loop with a wave-uniform trip count (WaveCount::flush needs the whole wave, as in
// rt_query.hip's query_body). The K lanes of an item load the same point / normal / index words - same-address loads that merge - and
// each its own direction of the item's set from the table, which is n_sets * K float4 and stays in the cache. A lane builds its ray as
// ao.py defines it (fp32, product then sum, nothing contracted in this unit in any arithmetic mode), routes it with query_on_grid
// and traces it through any_hit_grid<AM> on the grid, through the ordered loop with the reference's shadow predicate off it: the calls
// rt_query.hip's occlusion query makes, so occluded(ray) is rt_query_occluded's answer. The reduction takes no LDS and no atomics: one
// ballot of "unoccluded", of which an item's K-bit field is counted; the lane with l % K == 0 stores the byte and the float. A dead
// item (index < 0, or a point / normal that is not finite) and the tail beyond n keep their lanes idle; no lane leaves early.
//
// Counters go through WaveCount (rays per route, exact tests); the live items are a ballot of the sample-0 lanes per trip, added once
// per wave.
#include "rt_ao.h"
#include "rt_query_device.h"

namespace rt {
namespace {

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void ao_pass(const Scene S, const GridDesc g, const QueryBox box, const GBufferShard sh, const AoInputs in,
                                                       const uint32_t log_k, uint8_t* __restrict__ unoccluded, float* __restrict__ ao,
                                                       AoCounters* __restrict__ counters) {
    WaveCount wc;
    unsigned long long live_items = 0;  // wave-uniform
    const uint32_t K = 1u << log_k;
    const uint32_t k = threadIdx.x & (K - 1u);
    const uint32_t field_shift = (threadIdx.x & 63u) & ~(K - 1u);  // where this lane's item starts in the wave's ballot
    const unsigned long long field_mask = K == 64u ? ~0ull : ((1ull << K) - 1ull);
    const uint64_t block_items = kQueryBlock >> log_k;
    const uint64_t stride = (uint64_t)gridDim.x * block_items;
    for (uint64_t base = (uint64_t)blockIdx.x * block_items; base < sh.n_local; base += stride) {
        const uint64_t i = base + (threadIdx.x >> log_k);
        const bool in_range = i < sh.n_local;
        bool live = false, on_grid = false, blocked = false;
        if (in_range) {
            const float4 p = in.point[i];
            const float4 n = in.normal[i];
            live = (in.index ? in.index[i] >= 0 : true) && finite_(p.x) && finite_(p.y) && finite_(p.z) && finite_(n.x) && finite_(n.y) &&
                   finite_(n.z);
            if (live) {
                uint64_t w = i;  // the global work-item: gbuffer_records' arithmetic
                if (sh.world > 1u) {
                    const uint64_t run = i / sh.tile_rays;
                    w = (run * sh.world + sh.rank) * sh.tile_rays + (i - run * sh.tile_rays);
                }
                const uint32_t h = (uint32_t)w * 0x9E3779B1u;
                const uint32_t set = (h >> 16) % in.n_sets;
                float4 d = in.dirs[(uint64_t)set * K + k];
                const float s = (d.x * n.x + d.y * n.y) + d.z * n.z;
                if (s < 0.f) {  // (a NaN or a zero keeps d)
                    d.x = -d.x;
                    d.y = -d.y;
                    d.z = -d.z;
                }
                Ray ray;
                ray.sx = p.x + in.bias * n.x;
                ray.sy = p.y + in.bias * n.y;
                ray.sz = p.z + in.bias * n.z;
                ray.sw = 1.f;
                ray.dx = d.x; ray.dy = d.y; ray.dz = d.z; ray.dw = 0.f;
                on_grid = query_on_grid(box, ray);
                if (on_grid) {
                    uint32_t tested = 0;
                    blocked = any_hit_grid<AM>(g, S, ray, tested);
                    wc.tests += tested;
                } else {
                    float T;
                    int idx;
                    query_closest_one<AM>(S, g, false, ray, T, idx, wc);
                    blocked = !(T >= 1.f || T < 0.f);  // query_body's predicate: a NaN reads occluded
                }
            }
        }
        wc.route(live, on_grid);
        live_items += (unsigned long long)__popcll(__ballot(live && k == 0u));
        const unsigned long long open = __ballot(live && !blocked);
        if (in_range && k == 0u) {
            const uint32_t count = live ? (uint32_t)__popcll((open >> field_shift) & field_mask) : K;  // a dead item reads K / 1.0f
            if (unoccluded) unoccluded[i] = (uint8_t)count;
            if (ao) ao[i] = (float)count * in.inv_samples;
        }
    }
    wc.flush(&counters->q);
    if ((threadIdx.x & 63u) == 0u && live_items) atomicAdd(&counters->n_live, live_items);
}

}  // namespace

hipError_t launch_ao(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const GBufferShard& shard, const AoInputs& in,
                     const AoOutputs& out, AoCounters* d_counters, hipStream_t stream) {
    const uint64_t n = shard.n_local;
    if (n == 0) return hipSuccess;
    uint32_t log_k = 0;
    while (log_k < 6u && (1u << log_k) != in.samples) ++log_k;
    if ((1u << log_k) != in.samples || in.n_sets == 0 || !in.point || !in.normal || !in.dirs || misaligned(in.point, 16) ||
        misaligned(in.normal, 16) || misaligned(in.dirs, 16) || misaligned(in.index, 4) || outputs_refused({{out.unoccluded, 1}, {out.ao, 4}}) ||
        !d_counters || shard.tile_rays == 0)
        return hipErrorInvalidValue;
    const uint64_t block_items = kQueryBlock >> log_k;
    const uint64_t want = (n + block_items - 1) / block_items;
    const dim3 blocks((uint32_t)(want < kQueryMaxBlocks ? want : kQueryMaxBlocks));
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((ao_pass<am()>), blocks, dim3(kQueryBlock), 0, stream, scene, grid, box, shard, in, log_k, out.unoccluded, out.ao, d_counters);
    });
}

}  // namespace rt
