// rt_transforms.h - host-side launcher of the transform patch (rt_transforms.hip): every copy of mv and mvInverse that a live
// context keeps of a range of objects, rewritten in place from rt_transform records that are in device memory (rt_set_transforms).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

struct HotPair;       // rt_device.h
struct HotObject;
struct ColdObject;
struct ObjectRecord;
struct CompactObject;

// the record arrays of a context (rt_context.h); `n_objs` records each, (n_objs + 1) / 2 pairs in either stream
struct TransformTargets {
    HotPair* pairs;
    HotPair* shadow_pairs;
    HotObject* hot;
    ColdObject* cold;
    ObjectRecord* objrec;
    CompactObject* compact;   // null: the context keeps no compact records (triangles)
    uint32_t n_objs;
};

// Patches objects first .. first + count - 1 from `count` rt_transform records at d_transforms (128 bytes each, 16-byte aligned)
// on `stream`. d_shadow_slots holds `count` positions: object first + m sits at position d_shadow_slots[m] of the shadow stream
// (pair slot / 2, half slot & 1); in the traversal stream an object's position is its index. Written per object: HotObject::row0..2,
// ColdObject::mv_row[0..3] and inv_row3, ObjectRecord::inv_row[0..2] and mv_row[0..2], the twelve matrix words of its CompactObject
// (whatever the matrices are: whether a frame reads them is the host's predicate), and the object's half of its HotPair in both
// streams - the words repack_objects, pack_pairs and rt_create's ObjectRecord fill derive from the two matrices, the same bits.
// Type words, pads, materials and the neighbour's half of a pair are never touched. The slots are NOT checked against n_objs here
// (they are device memory): the caller passes a permutation's. hipErrorInvalidValue for a null or misaligned array, a null target or
// a range that leaves the n_objs records; count == 0 launches nothing.
hipError_t launch_patch_transforms(const float* d_transforms, const uint32_t* d_shadow_slots, uint32_t first, uint32_t count,
                                   const TransformTargets& to, hipStream_t stream);

}  // namespace rt
