// rt_visibility.h - host-side launcher of the visibility patch (rt_visibility.hip): every copy of the type word that a live context
// keeps of a range of objects, set to RT_TYPE_HIDDEN or back to the word rt_create was given, from a byte mask that is in device
// memory (rt_set_visibility / rt_set_visibility_device).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

struct HotPair;       // rt_device.h
struct HotObject;
struct ColdObject;
struct ObjectRecord;
struct CompactObject;

constexpr uint32_t kTypeKeep = 0xffffffffu;   // in `create_types`: an object created with a type other than 0, 1, 2 - never written

// the record arrays of a context (rt_context.h) and what the pass needs of rt_create: `n_objs` entries each, (n_objs + 1) / 2 pairs
struct VisibilityTargets {
    HotPair* pairs;
    HotPair* shadow_pairs;
    HotObject* hot;
    ColdObject* cold;
    ObjectRecord* objrec;
    CompactObject* compact;   // null: the context keeps no compact records (triangles)
    const uint32_t* create_types;   // per object: the type word rt_create was given (0, 1, 2), or kTypeKeep
    const uint32_t* shadow_slots;   // per object: its position in the shadow stream (pair slot / 2, half slot & 1)
    uint32_t n_objs;
};

// Patches objects first .. first + count - 1 from `count` bytes at d_visible (any alignment) on `stream`: 0 writes RT_TYPE_HIDDEN,
// anything else create_types[o], into HotObject::type, ObjectRecord::type, the fourth word of ColdObject::spec_type and the object's
// type_a / type_b in both pair streams. Nothing else is touched: no matrix, no material, not the neighbour's half of a pair, not the
// pad half of an odd count, not the spare record behind the last object; an object whose create_types entry is kTypeKeep is skipped.
// The slots are NOT checked against n_objs here (they are device memory): the caller passes a permutation's.
// hipErrorInvalidValue for a null mask or target or a range that leaves the n_objs records; count == 0 launches nothing.
hipError_t launch_patch_visibility(const uint8_t* d_visible, uint32_t first, uint32_t count, const VisibilityTargets& to, hipStream_t stream);

}  // namespace rt
