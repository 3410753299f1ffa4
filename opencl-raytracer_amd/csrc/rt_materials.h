// rt_materials.h - host-side launcher of the material patch (rt_materials.hip): the material words of a range of objects of a
// live context, rewritten in place from rt_material records that are in device memory (rt_set_materials / rt_set_materials_device).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

struct ColdObject;    // rt_device.h
struct ObjectRecord;
struct CompactObject;

// Patches objects first .. first + count - 1 of d_cold (and of d_objrec and d_compact, where the context has those tables: either may be null) from
// `count` rt_material records at d_materials (64 bytes each, 16-byte aligned) on `stream`. Written per object: ColdObject's
// amb_absorb, dif_shine and the first three words of spec_type, ObjectRecord::absorption and CompactObject::absorption - the words repack_objects and
// rt_create's ObjectRecord fill derive from a material, the same bits. Nothing else is touched. hipErrorInvalidValue for a null or
// misaligned array, a null d_cold, or a range that leaves the n_objs records; count == 0 launches nothing.
hipError_t launch_patch_materials(const float4* d_materials, uint32_t first, uint32_t count, ColdObject* d_cold, ObjectRecord* d_objrec,
                                  CompactObject* d_compact, uint32_t n_objs, hipStream_t stream);

}  // namespace rt
