// rt_transforms.hip - the transform patch: one pass that rewrites every copy of mv and mvInverse a context keeps of a range of objects.
//
// rt_create spreads an object's two matrices over five arrays (rt_device.h), each in the layout its reader wants: the walks' 64-byte
// HotObject (rows x, y, z of mvInverse), the shading record ColdObject (mv by rows, row w of mvInverse), the round machine's
// ObjectRecord (rows x, y, z of both), and the two pair streams, where the twelve words of mvInverse's rows x, y, z are interleaved
// with those of a neighbour - the traversal stream pairs objects 2p and 2p + 1, the shadow stream pairs them in rt_create's size order.
// A context without triangles keeps a sixth copy, the CompactObject: the diagonal and the translation column of both (rt_device.h).
// Per object 128 bytes are read and 48 + 80 + 96 + 48 + 48 (+ 48) written. The values are moved, never computed with: NaNs keep their bits.
// What depends on the matrices beyond these words - bounds, registration spheres, tables - is the host's business (rt_geometry.cpp).
//
// Form kept: EIGHT LANES PER OBJECT, ONE PER MATRIX ROW. The upload is column-major and every record wants rows, so somebody has to
// transpose. Lane k of a group gathers row (k & 3) of mv (k < 4) or of mvInverse (k >= 4): four 4-byte loads, 16 bytes apart. The
// group's 32 loads cover its object's 128 bytes exactly once, a wave's cover 1 KiB contiguous (8 records), so every line that is
// touched is used whole, and each lane then holds a float4 that IS a record member: all stores but the pair streams' are 16 bytes
// wide and need no lane to talk to another. The alternative - lane k loads the k-th float4 (a column) with one 16-byte load and the
// rows are put together by shuffles, as rt_materials.hip moves its two scalars - saves three load instructions per lane and costs
// twelve shuffles; it was not built. A grid context moves at most 64 objects per call (8 waves, one launch), and for the contexts
// without that cap the pass is bound by its 320 scattered bytes per object either way: it is a launch in both forms (DESIGN.md
// section 6 has the time), so the form without cross-lane traffic and without an "is my source lane active" argument stays.
// The pair streams take 4-byte stores (a half of a HotPair is every other word): the neighbour's half and type_a / type_b are never
// written, so two objects of one pair can be patched by one launch, or by two, in any order.
#include "rt_transforms.h"
#include "rt_device.h"

namespace rt {
namespace {

constexpr uint32_t kPatchBlock = 256;   // 32 objects per workgroup, 8 per wave
constexpr uint32_t kPatchLanes = 8;     // lanes per object: one per row of mv, one per row of mvInverse
static_assert(offsetof(HotObject, row0) == 0 && offsetof(HotObject, row1) == 16 && offsetof(HotObject, row2) == 32 && offsetof(HotObject, type) == 48 &&
              offsetof(ColdObject, mv_row) == 0 && offsetof(ColdObject, inv_row3) == 64 && offsetof(ColdObject, amb_absorb) == 80 &&
              offsetof(ObjectRecord, inv_row) == 0 && offsetof(ObjectRecord, type) == 48 && offsetof(ObjectRecord, mv_row) == 64 &&
              offsetof(ObjectRecord, spare1) == 112 && offsetof(CompactObject, a0) == 0 && offsetof(CompactObject, b0) == 16 &&
              offsetof(CompactObject, s0) == 32 && offsetof(CompactObject, x) == 48 && offsetof(HotPair, m) == 0 && offsetof(HotPair, type_a) == 96 && sizeof(f2) == 8,
              "the patch addresses the records by member");

// the half `slot & 1` of pair `slot / 2`: words m[4 r + c][half], c = 0..3
__device__ __forceinline__ void store_pair_row(HotPair* pairs, uint32_t slot, uint32_t r, const float4& v) {
    float* w = reinterpret_cast<float*>(&pairs[slot >> 1].m[4u * r]) + (slot & 1u);
    w[0] = v.x;
    w[2] = v.y;
    w[4] = v.z;
    w[6] = v.w;
}

__global__ __launch_bounds__(kPatchBlock) void patch_transforms(const float* __restrict__ transforms, const uint32_t* __restrict__ shadow_slots,
                                                                uint32_t first, uint32_t count, TransformTargets to) {
    const uint64_t t = (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x;   // = 8 m + k
    const uint64_t m = t / kPatchLanes;
    const uint32_t k = (uint32_t)(t % kPatchLanes);
    if (m >= (uint64_t)count) return;
    const uint32_t r = k & 3u;
    const float* src = transforms + 32u * m + (k < 4u ? 0u : 16u) + r;   // column-major: row r is words r, 4 + r, 8 + r, 12 + r
    const float4 v = make_float4(src[0], src[4], src[8], src[12]);
    const uint32_t o = first + (uint32_t)m;   // < n_objs (the launcher checked the range)
    if (k < 4u) {   // a row of mv
        to.cold[o].mv_row[r] = v;
        if (r < 3u) {
            to.objrec[o].mv_row[r] = v;
            if (to.compact) { (&to.compact[o].s0)[r] = (&v.x)[r]; (&to.compact[o].x)[r] = v.w; }   // the diagonal word and the translation's
        }
        return;
    }
    if (r == 3u) {   // row w of mvInverse
        to.cold[o].inv_row3 = v;
        return;
    }
    (&to.hot[o].row0)[r] = v;
    to.objrec[o].inv_row[r] = v;
    if (to.compact) { (&to.compact[o].a0)[r] = (&v.x)[r]; (&to.compact[o].b0)[r] = v.w; }
    store_pair_row(to.pairs, o, r, v);
    const uint32_t slot = shadow_slots[m];
    if (slot < to.n_objs) store_pair_row(to.shadow_pairs, slot, r, v);   // (a permutation's slots always are)
}

}  // namespace

hipError_t launch_patch_transforms(const float* d_transforms, const uint32_t* d_shadow_slots, uint32_t first, uint32_t count,
                                   const TransformTargets& to, hipStream_t stream) {
    if ((uint64_t)first + (uint64_t)count > (uint64_t)to.n_objs) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (!d_transforms || (reinterpret_cast<uintptr_t>(d_transforms) & 15u) || !d_shadow_slots || !to.pairs || !to.shadow_pairs || !to.hot ||
        !to.cold || !to.objrec)
        return hipErrorInvalidValue;
    const uint64_t blocks = ((uint64_t)count * kPatchLanes + kPatchBlock - 1) / kPatchBlock;   // <= 2^27
    hipLaunchKernelGGL(patch_transforms, dim3((uint32_t)blocks), dim3(kPatchBlock), 0, stream, d_transforms, d_shadow_slots, first, count, to);
    return hipGetLastError();
}

}  // namespace rt
