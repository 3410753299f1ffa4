// rt_gbuffer.hip - G-buffer frames (hip_raytracer.h): the record kernel behind the frame pipeline's own primary round.
//
// The trace is not here: rt_render.cpp runs the context's primary round as a hittest frame (screen tiles, grid, literal and
// brute-force routes - whatever the frame takes), which leaves (t, index) per local work-item in pixel order. This kernel streams over
// them: one thread per local work-item, 256 per workgroup, workgroups loop. A lane reads t[i] and index[i] (two coalesced 4-byte
// loads), finds its global work-item by global_ray_of's arithmetic on the local PIXEL index (rt_wavefront.hip; the outputs are in
// pixel order, so pixel_of is not needed), regenerates the pinhole ray or reads the ray buffer (primary_ray's two branches, shared
// with the queries as camera_ray) and - where t < MAX_FLOAT - calls materialise<AM>() exactly as query_hits_body does, then gathers
// the winner's diffuse words. Every requested record leaves as one 16-byte store per lane; a miss, a NaN time and a padding
// work-item of a ragged last tile (the frame wrote MAX_FLOAT, -1 there) store zero bytes. Neighbouring pixels mostly hit the same
// object, so the 128-byte record gathers of a wave merge into a few lines.
//
// t and index are only read. The count of hits is a ballot per trip, added once per wave by one lane with a vector atomic
// (WaveCount::flush's form); no lane leaves the loop early, the trip count is wave-uniform.
#include "rt_gbuffer.h"
#include "rt_query_device.h"

namespace rt {
namespace {

constexpr uint32_t kGBufferMaxBlocks = 2048;  // 8 workgroups per CU; a streaming kernel gains nothing from more, the loop takes the rest

template <int AM>
__global__ __launch_bounds__(kQueryBlock) void gbuffer_records(const Scene S, const QueryCamera cam, const GBufferShard sh,
                                                               const GBufferRecords rec, unsigned long long* __restrict__ d_hits) {
    unsigned long long hits = 0;  // wave-uniform
    const bool records = rec.point != nullptr || rec.normal != nullptr;
    const uint64_t stride = (uint64_t)gridDim.x * kQueryBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kQueryBlock; base < sh.n_local; base += stride) {
        const uint64_t i = base + threadIdx.x;
        bool hit = false;
        if (i < sh.n_local) {
            const float T = rec.t[i];
            const int idx = rec.index[i];
            uint64_t g = i;
            if (sh.world > 1u) {  // (a shard's run is one tile: RenderParams::run_rays == tile_rays)
                const uint64_t run = i / sh.tile_rays;
                g = (run * sh.world + sh.rank) * sh.tile_rays + (i - run * sh.tile_rays);
            }
            // the frame's rule makes index >= 0 exactly where t < MAX_FLOAT; the two bounds keep a gather inside the arrays whatever
            // the buffers hold
            hit = T < kMaxFloat && (uint32_t)idx < S.n_objs && g < sh.n_rays;
            float4 P = make_float4(0.f, 0.f, 0.f, 0.f), N = P, A = P;
            if (hit) {
                if (records) {
                    const Ray ray = camera_ray(cam, g);
                    HitRec h;
                    materialise<AM>(S.objrec, S.cold, idx, T, ray, h, S.affine != 0u && finite3(ray));  // query_hits_body's call
                    P = make_float4(h.px, h.py, h.pz, h.pw);
                    N = make_float4(h.nx, h.ny, h.nz, 0.f);
                }
                if (rec.albedo) {
                    const float4 dif = S.cold[idx].dif_shine;  // moved, not computed with: a NaN keeps its bits
                    A = make_float4(dif.x, dif.y, dif.z, 1.0f);
                }
            }
            if (rec.point) rec.point[i] = P;
            if (rec.normal) rec.normal[i] = N;
            if (rec.albedo) rec.albedo[i] = A;
        }
        hits += (unsigned long long)__popcll(__ballot(hit));
    }
    if ((threadIdx.x & 63u) == 0u && hits) atomicAdd(d_hits, hits);
}

}  // namespace

hipError_t launch_gbuffer_records(const Scene& scene, const QueryCamera& camera, const GBufferShard& shard, int arith,
                                  const GBufferRecords& rec, unsigned long long* d_hits, hipStream_t stream) {
    if (shard.n_local == 0) return hipSuccess;
    if (!rec.t || !rec.index || misaligned(rec.t, 4) || misaligned(rec.index, 4) || misaligned(rec.point, 16) ||
        misaligned(rec.normal, 16) || misaligned(rec.albedo, 16) || !d_hits || shard.tile_rays == 0 || camera_refused(camera))
        return hipErrorInvalidValue;
    const uint64_t want = (shard.n_local + kQueryBlock - 1) / kQueryBlock;
    const dim3 blocks((uint32_t)(want < kGBufferMaxBlocks ? want : kGBufferMaxBlocks));
    return launch_for_arith(arith, [&](auto am) {
        hipLaunchKernelGGL((gbuffer_records<am()>), blocks, dim3(kQueryBlock), 0, stream, scene, camera, shard, rec, d_hits);
    });
}

}  // namespace rt
