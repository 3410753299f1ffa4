// rt_visibility.hip - the visibility patch: one pass that rewrites every copy of the TYPE WORD a context keeps of a range of objects.
//
// rt_create writes an object's type into five places (rt_device.h, rt_scene.cpp): HotObject::type (the walks, the literal loops, brute
// force), ObjectRecord::type (the round machine's materialise), the fourth word of ColdObject::spec_type (type bits beside the specular
// colour), and type_a / type_b of the object's half of its HotPair in the traversal stream (pair o / 2, half o & 1) and in the shadow
// stream (where rt_create's size order put it). A type that is none of 0, 1, 2 is never hit - the reference's switch has no default -
// so hiding an object is writing RT_TYPE_HIDDEN into all five, and showing it is writing the create-time word back. A context without
// triangles keeps a sixth copy, CompactObject::type (the frames of scale-and-translate scenes), written with the others. Per object one
// mask byte and two support words (create-time type, shadow slot) are read and five words written. The values are moved, never
// computed with. What follows the types on the host - the NaN-ray winner, RT_FLAG_DEVICE_OPENCL's predicate - is rt_visibility_host.cpp's.
//
// Form kept: ONE LANE PER OBJECT. A wave reads 64 contiguous mask bytes (one line at most two, whatever the array's alignment - a
// torch bool tensor is byte-aligned and nothing wider can be assumed), 256 contiguous bytes of create-time types and 256 of shadow
// slots, and each lane issues five 4-byte stores: four at a fixed stride of its record size (64 / 128 / 128 bytes apart across the
// wave, pair halves 4 bytes apart in one line) and one scattered by the size order. Nothing is shared between lanes: no shuffle, no
// LDS, no "is my source lane active" argument, and a lane beyond the range simply returns. The alternative - several lanes per object,
// one per copy, as rt_transforms.hip gives a lane to a matrix row - would only spread five independent stores of one word over five
// lanes and read the three inputs five times; there is no wide member to move here. The pass writes 20 bytes per object into five
// different lines, so it is bound by lines touched, not by lanes: for cfg4's 100 000 objects that is 27 MB of line traffic at most,
// microseconds, under one launch's latency (DESIGN.md section 6 has the measured time).
// type_a and type_b of one pair belong to two objects, hence to two lanes: each stores its own 4-byte word, never the 8-byte pair, so
// the neighbour's half - and the pad half 0xffffffff of an odd count, which is nobody's - is not written.
#include "rt_visibility.h"
#include "rt_device.h"
#include "rt_records.h"

namespace rt {
namespace {

constexpr uint32_t kPatchBlock = 128;   // 128 objects per workgroup, 64 per wave (nothing is shared: a small group only spreads the scattered stores over more CUs)
static_assert(offsetof(HotObject, type) == 48 && offsetof(ObjectRecord, type) == 48 && offsetof(CompactObject, type) == 12 && offsetof(ColdObject, spec_type) == 112 &&
              offsetof(HotPair, type_a) == 96 && offsetof(HotPair, type_b) == 100, "the patch addresses the records by member");

__global__ __launch_bounds__(kPatchBlock) void patch_visibility(const uint8_t* __restrict__ visible, uint32_t first, uint32_t count, VisibilityTargets to) {
    const uint64_t m = (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x;
    if (m >= (uint64_t)count) return;
    const uint32_t o = first + (uint32_t)m;   // < n_objs (the launcher checked the range)
    const uint32_t created = to.create_types[o];
    if (created == kTypeKeep) return;         // created with a type of its own: left alone
    const uint32_t word = visible[m] ? created : RT_TYPE_HIDDEN;
    to.hot[o].type = word;
    to.objrec[o].type = word;
    if (to.compact) to.compact[o].type = word;
    reinterpret_cast<uint32_t*>(&to.cold[o].spec_type)[3] = word;   // the type bits; the three specular floats stay
    (&to.pairs[o >> 1].type_a)[o & 1u] = word;
    const uint32_t slot = to.shadow_slots[o];
    if (slot < to.n_objs) (&to.shadow_pairs[slot >> 1].type_a)[slot & 1u] = word;   // (a permutation's slots always are)
}

}  // namespace

hipError_t launch_patch_visibility(const uint8_t* d_visible, uint32_t first, uint32_t count, const VisibilityTargets& to, hipStream_t stream) {
    if ((uint64_t)first + (uint64_t)count > (uint64_t)to.n_objs) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (!d_visible || !to.pairs || !to.shadow_pairs || !to.hot || !to.cold || !to.objrec || !to.create_types || !to.shadow_slots)
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((uint64_t)count + kPatchBlock - 1) / kPatchBlock);   // <= 2^25
    hipLaunchKernelGGL(patch_visibility, dim3(blocks), dim3(kPatchBlock), 0, stream, d_visible, first, count, to);
    return hipGetLastError();
}

}  // namespace rt
