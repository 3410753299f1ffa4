// rt_object_patch.cpp - what the calls that patch a range of a live context's objects share (rt_set_materials, rt_set_transforms,
// rt_set_visibility and their _device, _multi and rt_read_* companions): the two refusals every one of them makes of its range, the
// one staging buffer a host array is uploaded through, the three-event trace timer, and the re-evaluation of RT_FLAG_DEVICE_OPENCL's
// predicate on the lights. Behind them the replaceable materials (hip_raytracer.h): rt_set_materials, rt_set_materials_device,
// rt_read_materials - of the three patches the one with nothing of its own on the host.
#include "rt_context.h"

namespace rt::host {

int check_object_range(rt_context* c, const void* p, uint32_t first, uint32_t count, const char* what, bool null_first) {
    const bool null = count && !p, past = (uint64_t)first + (uint64_t)count > (uint64_t)c->n_objs;
    if (past && !(null && null_first)) return fail(c, RT_ERR_INVALID_ARGUMENT, "first + count exceeds the context's object count");
    if (null) return fail(c, RT_ERR_INVALID_ARGUMENT, std::string(what) + " is NULL with a non-zero count");
    return RT_OK;
}

int check_set_materials(rt_context* c, const void* materials, uint32_t first, uint32_t count) {
    return check_object_range(c, materials, first, count, "materials");
}

// Grow-only. The larger buffer first, then the old one freed: a failed allocation leaves the context as it was (Buffer::grow frees
// first). One buffer serves every patch call because each of them synchronises its stream before it returns and a context is
// driven by one thread at a time: no call finds another's bytes still in flight.
int ensure_patch_stage(rt_context* c, size_t bytes) {
    Buffer& stage = c->d_patch_stage;
    if (bytes <= stage.bytes) return RT_OK;
    Buffer larger;
    if (const int rc = larger.grow(c, bytes)) return rc;
    std::swap(stage.p, larger.p);  // (the old one goes with `larger`)
    std::swap(stage.bytes, larger.bytes);
    return RT_OK;
}

PatchTrace::~PatchTrace() {
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

int PatchTrace::begin(hipStream_t stream) {
    if (!std::getenv(env)) return RT_OK;
    for (hipEvent_t& e : ev) RT_HIP(c, hipEventCreate(&e));
    on = true;
    return mark(0, stream);
}

int PatchTrace::mark(int k, hipStream_t stream) {
    if (on) RT_HIP(c, hipEventRecord(ev[k], stream));
    return RT_OK;
}

int PatchTrace::report(uint32_t count) {
    if (!on) return RT_OK;
    float copy_ms = 0.f, patch_ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&copy_ms, ev[0], ev[1]));
    RT_HIP(c, hipEventElapsedTime(&patch_ms, ev[1], ev[2]));
    std::fprintf(stderr, "[%s] copy %.4f ms patch %.4f ms %s %u\n", label, (double)copy_ms, (double)patch_ms, unit, count);
    return RT_OK;
}

// RT_FLAG_DEVICE_OPENCL's predicate on the lights (rt_create: lights_need_literal), evaluated again for lights L over the objects as
// they now are - moved (rt_set_transforms), hidden (rt_set_visibility) - or for new lights (rt_set_lights). The first three terms are
// the condition rt_create evaluates it under (the flag, no RT_FLAG_LITERAL from the caller or from a degenerate instance), and under
// that condition rt_create has sized h_obj_bounds: the last term holds for every caller then, rt_set_lights among them, and only
// spells out what lights_need_literal indexes.
void refresh_lights_literal(rt_context* c, const rt_light* L, uint32_t n_lights) {
    if (!(c->user_flags & RT_FLAG_DEVICE_OPENCL) || (c->user_flags & RT_FLAG_LITERAL) || c->degenerate_literal ||
        c->h_obj_bounds.size() != 4 * (size_t)c->n_objs)
        return;
    c->lights_literal = lights_need_literal(c, L, n_lights);
    const uint32_t base = c->user_flags | (c->lights_literal ? RT_FLAG_LITERAL : 0u);
    if (c->base_flags != base) c->tiles_dirty = true;  // (a table's verdict depends on the literal flag)
    c->base_flags = base;
    c->forced_literal = c->lights_literal;
    apply_ray_domain(c);
}

namespace {

// Nothing of a context is derived from a material but the words repack_objects and the ObjectRecord fill copy out of it, so new
// materials are one patch pass over those two arrays (rt_materials.hip). The host form stages its array in device memory and
// takes the same pass.
// d_src: `count` records in device memory, valid behind what `stream` holds already. Enqueues the patch there and waits for it.
// trace: begun by the caller before its upload, if any (RT_MATERIALS_TRACE=1, tools/ab/set_materials_timing.py).
int patch_materials_on(rt_context* c, const void* d_src, uint32_t first, uint32_t count, hipStream_t stream, PatchTrace& trace) {
    if (const int rc = trace.uploaded(stream)) return rc;
    const hipError_t e = rt::launch_patch_materials(static_cast<const float4*>(d_src), first, count, c->d_cold, c->d_objrec, c->d_compact, c->n_objs, stream);
    if (e != hipSuccess) return fail_hip(c, e, "material patch launch");
    if (const int rc = trace.patched(stream)) return rc;
    RT_HIP(c, hipStreamSynchronize(stream));  // synchronous like rt_set_lights: the array is the caller's again, any stream's next frame sees it
    return trace.report(count);
}

}  // namespace
}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_set_materials_device(rt_context* c, const void* d_materials, uint32_t first, uint32_t count, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_materials(c, d_materials, first, count);
    if (refused) return refused;
    if (reinterpret_cast<uintptr_t>(d_materials) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the material array must be 16-byte aligned");
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);  // NULL: the legacy default stream, as for rt_set_rays_device
    PatchTrace trace(c, "RT_MATERIALS_TRACE", "rt_set_materials", "materials");
    if (const int rc = trace.begin(stream)) return rc;
    return patch_materials_on(c, d_materials, first, count, stream, trace);
}

int rt_set_materials(rt_context* c, const void* materials, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_materials(c, materials, first, count);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    const size_t bytes = sizeof(rt_material) * (size_t)count;
    if (const int rc = ensure_patch_stage(c, bytes)) return rc;
    PatchTrace trace(c, "RT_MATERIALS_TRACE", "rt_set_materials", "materials");
    if (const int rc = trace.begin(c->stream)) return rc;
    // (the copy takes the bytes as they are: `materials` may have any alignment)
    RT_HIP(c, hipMemcpyAsync(c->d_patch_stage.p, materials, bytes, hipMemcpyHostToDevice, c->stream));
    return patch_materials_on(c, c->d_patch_stage.p, first, count, c->stream, trace);
}

int rt_read_materials(rt_context* c, void* materials, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_materials(c, materials, first, count);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    std::vector<rt::ColdObject> cold(count);
    std::vector<rt::ObjectRecord> rec(count);
    RT_HIP(c, hipMemcpy(cold.data(), c->d_cold + first, sizeof(rt::ColdObject) * (size_t)count, hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(rec.data(), c->d_objrec + first, sizeof(rt::ObjectRecord) * (size_t)count, hipMemcpyDeviceToHost));
    std::vector<rt::CompactObject> compact(c->d_compact ? count : 0u);
    if (c->d_compact) RT_HIP(c, hipMemcpy(compact.data(), c->d_compact + first, sizeof(rt::CompactObject) * (size_t)count, hipMemcpyDeviceToHost));
    uint8_t* out = static_cast<uint8_t*>(materials);  // (any alignment: the records are assembled here and copied out)
    for (uint32_t i = 0; i < count; ++i) {
        const rt::ColdObject& k = cold[i];
        if (std::memcmp(&k.amb_absorb.w, &rec[i].absorption, 4) != 0)
            return fail(c, RT_ERR_STATE, "rt_read_materials: object " + std::to_string((uint64_t)first + i) +
                                             ": ObjectRecord::absorption does not hold the bits of ColdObject::amb_absorb.w");
        if (c->d_compact && std::memcmp(&k.amb_absorb.w, &compact[i].absorption, 4) != 0)
            return fail(c, RT_ERR_STATE, "rt_read_materials: object " + std::to_string((uint64_t)first + i) +
                                             ": CompactObject::absorption does not hold the bits of ColdObject::amb_absorb.w");
        rt_material m;
        std::memset(&m, 0, sizeof(m));  // the five words no kernel reads: 0
        std::memcpy(m.ambient, &k.amb_absorb, 12);
        std::memcpy(m.diffuse, &k.dif_shine, 12);
        std::memcpy(m.specular, &k.spec_type, 12);
        std::memcpy(&m.absorption, &k.amb_absorb.w, 4);
        std::memcpy(&m.shininess, &k.dif_shine.w, 4);
        std::memcpy(out + sizeof(rt_material) * (size_t)i, &m, sizeof(m));
    }
    return RT_OK;
}

}  // extern "C"
