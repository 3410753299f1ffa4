// rt_materials.hip - the material patch: one streaming pass that rewrites the material words of a range of objects in place.
//
// Of an object's 64-byte material the frame's kernels read eleven floats, and rt_create keeps them in two record arrays
// (rt_device.h): ColdObject::amb_absorb (ambient rgb, absorption), ::dif_shine (diffuse rgb, shininess), ::spec_type.xyz
// (specular rgb; .w holds the type bits) and a second copy of the absorption in ObjectRecord::absorption. No table, list or
// predicate of a context is derived from them, so new materials are this patch and nothing else. Per material 64 bytes are read
// and 40 + 4 written; the values are moved, never computed with, so NaNs keep their bits.
//
// Form kept: FOUR LANES PER MATERIAL. Lane k of a group loads the k-th float4 of the record, so a wave reads 1 KiB contiguous
// (16 records) in one instruction; the fourth float4 holds the two scalars that belong into the w lanes of the first two, and
// reaches lanes 0 and 1 by a shuffle within the group. Lane 0 stores amb_absorb and lane 1 dif_shine (16 bytes each), lane 2
// the three specular floats - 12 bytes: the type bits behind them are never read, never written - and lane 3 the ObjectRecord's
// absorption and, where the context keeps compact records, the CompactObject's. The alternative, one lane per material, would issue four 16-byte loads per lane that lie 64 bytes apart across the
// wave - each instruction touches 64 lines for 1 KiB of use. It was not built: the four-lane form patches cfg4's 100 000
// materials in 8 microseconds, which is a launch, and leaves nothing to compare on.
// A group is active or idle as a whole (the bound is a material count), so the shuffle's source lane is active whenever its
// readers are; idle lanes load nothing and carry zeros through the shuffle.
#include "rt_materials.h"
#include "rt_device.h"

namespace rt {
namespace {

constexpr uint32_t kPatchBlock = 256;                 // 64 materials per workgroup, 16 per wave
constexpr uint32_t kPatchLanes = 4;                   // lanes per material: one per float4 of the record
static_assert(offsetof(ColdObject, amb_absorb) == 80 && offsetof(ColdObject, dif_shine) == 96 && offsetof(ColdObject, spec_type) == 112 &&
              offsetof(ObjectRecord, absorption) == 56 && offsetof(CompactObject, absorption) == 28, "the patch addresses the records by member");

__global__ __launch_bounds__(kPatchBlock) void patch_materials(const float4* __restrict__ materials, uint32_t first, uint32_t count,
                                                               ColdObject* __restrict__ cold, ObjectRecord* __restrict__ objrec,
                                                               CompactObject* __restrict__ compact) {
    const uint64_t t = (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x;   // = 4 m + k: the index of this lane's float4
    const uint64_t m = t / kPatchLanes;
    const uint32_t k = (uint32_t)(t % kPatchLanes);
    const bool active = m < (uint64_t)count;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) v = materials[t];
    // the group's lane 3 holds (absorption, reflection, transparency, shininess)
    const int last = (int)((threadIdx.x % 64u) | 3u);
    const float absorption = __shfl(v.x, last, 64);
    const float shininess = __shfl(v.w, last, 64);
    if (!active) return;
    const uint64_t o = (uint64_t)first + m;
    if (k == 0u) {
        cold[o].amb_absorb = make_float4(v.x, v.y, v.z, absorption);
    } else if (k == 1u) {
        cold[o].dif_shine = make_float4(v.x, v.y, v.z, shininess);
    } else if (k == 2u) {
        float* spec = &cold[o].spec_type.x;   // three words; spec_type.w (the type bits) stays as it is
        spec[0] = v.x;
        spec[1] = v.y;
        spec[2] = v.z;
    } else {
        if (objrec) objrec[o].absorption = v.x;
        if (compact) compact[o].absorption = v.x;
    }
}

}  // namespace

hipError_t launch_patch_materials(const float4* d_materials, uint32_t first, uint32_t count, ColdObject* d_cold, ObjectRecord* d_objrec,
                                  CompactObject* d_compact, uint32_t n_objs, hipStream_t stream) {
    if ((uint64_t)first + (uint64_t)count > (uint64_t)n_objs) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (!d_materials || (reinterpret_cast<uintptr_t>(d_materials) & 15u) || !d_cold) return hipErrorInvalidValue;
    const uint64_t blocks = ((uint64_t)count * kPatchLanes + kPatchBlock - 1) / kPatchBlock;   // <= 2^26
    hipLaunchKernelGGL(patch_materials, dim3((uint32_t)blocks), dim3(kPatchBlock), 0, stream, d_materials, first, count, d_cold, d_objrec, d_compact);
    return hipGetLastError();
}

}  // namespace rt
