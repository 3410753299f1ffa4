// rt_visibility_host.cpp - replaceable visibility (hip_raytracer.h): rt_set_visibility, rt_set_visibility_device, rt_read_visibility.
// Hiding an object is writing RT_TYPE_HIDDEN into every copy of its type word, showing it is writing the create-time word back: one
// patch pass (rt_visibility.hip). No table is rebuilt - a table entry is only a candidate, and the exact test of a
// type that is none of 0, 1, 2 never hits. What the host derives from the types follows from a mirror of the mask: the NaN-ray winner
// (the last VISIBLE sphere or box) and, under RT_FLAG_DEVICE_OPENCL, the predicate on the lights, which skips hidden objects.
#include "rt_context.h"
#include "rt_device.h"

namespace rt::host {

int check_set_visibility(rt_context* c, const void* visible, uint32_t first, uint32_t count) {
    return check_object_range(c, visible, first, count, "visible");
}

namespace {

// the type word rt_create was given for an object of this kind (h_kind: min(type, 3)), or "leave it alone"
inline uint32_t created_word(uint8_t kind) { return (kind & 0x7fu) <= 2u ? (uint32_t)(kind & 0x7fu) : rt::kTypeKeep; }

// what the patch pass reads of rt_create, on the device; made by the first call
int ensure_support(rt_context* c) {
    if (c->d_vis_types && c->d_vis_slots) return RT_OK;
    const uint32_t n = c->n_objs;
    std::vector<uint32_t> types(n);
    for (uint32_t i = 0; i < n; ++i) types[i] = created_word(c->h_kind[i]);
    uint32_t *d_types = nullptr, *d_slots = nullptr;
    RT_HIP(c, hipMalloc((void**)&d_types, sizeof(uint32_t) * (size_t)n));
    hipError_t e = hipMalloc((void**)&d_slots, sizeof(uint32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(d_types, types.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_slots, c->h_shadow_slot.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {  // a failed call leaves the context as it was
        (void)hipFree(d_types);
        if (d_slots) (void)hipFree(d_slots);
        return fail_hip(c, e, "rt_set_visibility: create-time types and shadow slots");
    }
    c->d_vis_types = d_types;
    c->d_vis_slots = d_slots;
    return RT_OK;
}

// the host's side of an accepted call: `mask` is the `count` bytes the pass has read
void follow_the_types(rt_context* c, const uint8_t* mask, uint32_t first, uint32_t count) {
    if (c->h_hidden.empty()) c->h_hidden.assign(c->n_objs, 0);
    // (all of the call that grows with count: locals, since a byte store may alias the context, and no branch on the mask's bytes)
    uint8_t* const hidden = c->h_hidden.data() + first;
    const uint8_t* const kind = c->h_kind.data() + first;
    for (uint32_t m = 0; m < count; ++m) hidden[m] = (uint8_t)((mask[m] == 0) & (created_word(kind[m]) != rt::kTypeKeep));
    // the last sphere / box of the scene decides what a NaN ray ends with (rt_create): the last VISIBLE one
    c->nan_winner = -1;
    c->nan_winner_sphere = false;
    for (uint32_t i = c->n_objs; i-- > 0;) {
        const uint32_t ty = c->h_kind[i] & 0x7fu;
        if (ty <= 1u && !c->h_hidden[i]) { c->nan_winner = (int)i; c->nan_winner_sphere = (ty == 0u); break; }
    }
    refresh_lights_literal(c, c->h_lights.data(), c->n_lights);  // (the predicate on the lights, without the hidden objects)
}

// Both forms of the call. d_src: `count` bytes in device memory, valid behind what `stream` holds already - or, with the caller's host
// mask h_mask, null: the mask is staged and uploaded on `stream`. Enqueues the patch there and waits for it; the host's mirror follows
// the bytes the pass read, which the device form copies back behind the pass on the same stream (the caller's kernels have written them).
int set_visibility_from(rt_context* c, const uint8_t* d_src, hipStream_t stream, const uint8_t* h_mask, uint32_t first, uint32_t count) {
    const int refused = check_set_visibility(c, h_mask ? h_mask : d_src, first, count);
    if (refused || count == 0) return refused;
    RT_DEVICE(c);
    if (const int rc = ensure_support(c)) return rc;
    if (h_mask) {
        if (const int rc = ensure_patch_stage(c, (size_t)count)) return rc;
        d_src = static_cast<const uint8_t*>(c->d_patch_stage.p);
    }
    PatchTrace trace(c, "RT_VISIBILITY_TRACE", "rt_set_visibility", "objects");  // (tools/ab/set_visibility_timing.py)
    if (const int rc = trace.begin(stream)) return rc;
    if (h_mask) RT_HIP(c, hipMemcpyAsync(c->d_patch_stage.p, h_mask, (size_t)count, hipMemcpyHostToDevice, stream));
    if (const int rc = trace.uploaded(stream)) return rc;
    const rt::VisibilityTargets to{c->d_pairs, c->d_shadow_pairs, c->d_hot, c->d_cold, c->d_objrec, c->d_compact, c->d_vis_types, c->d_vis_slots, c->n_objs};
    const hipError_t e = rt::launch_patch_visibility(d_src, first, count, to, stream);
    if (e != hipSuccess) return fail_hip(c, e, "visibility patch launch");
    if (const int rc = trace.patched(stream)) return rc;
    std::vector<uint8_t> read_back;
    if (!h_mask) {
        read_back.resize(count);
        RT_HIP(c, hipMemcpyAsync(read_back.data(), d_src, (size_t)count, hipMemcpyDeviceToHost, stream));
        h_mask = read_back.data();
    }
    RT_HIP(c, hipStreamSynchronize(stream));  // synchronous like rt_set_materials: the mask is the caller's again, any stream's next frame sees it
    follow_the_types(c, h_mask, first, count);
    return trace.report(count);
}

}  // namespace
}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_set_visibility_device(rt_context* c, const void* d_visible, uint32_t first, uint32_t count, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // (a NULL stream: the legacy default stream, as for rt_set_materials_device)
    return set_visibility_from(c, static_cast<const uint8_t*>(d_visible), static_cast<hipStream_t>(hip_stream), nullptr, first, count);
}

int rt_set_visibility(rt_context* c, const uint8_t* visible, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    return set_visibility_from(c, nullptr, c->stream, visible, first, count);
}

int rt_read_visibility(rt_context* c, uint8_t* visible, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_visibility(c, visible, first, count);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    std::vector<rt::HotObject> hot(count);
    std::vector<rt::ColdObject> cold(count);
    std::vector<rt::ObjectRecord> rec(count);
    const uint32_t p0 = first / 2u, p1 = (first + count - 1u) / 2u;
    std::vector<rt::HotPair> pairs((size_t)p1 - p0 + 1), spairs(c->n_pairs);  // (the shadow stream whole: its slots are scattered)
    RT_HIP(c, hipMemcpy(hot.data(), c->d_hot + first, sizeof(rt::HotObject) * (size_t)count, hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(cold.data(), c->d_cold + first, sizeof(rt::ColdObject) * (size_t)count, hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(rec.data(), c->d_objrec + first, sizeof(rt::ObjectRecord) * (size_t)count, hipMemcpyDeviceToHost));
    std::vector<rt::CompactObject> compact(c->d_compact ? count : 0u);
    if (c->d_compact) RT_HIP(c, hipMemcpy(compact.data(), c->d_compact + first, sizeof(rt::CompactObject) * (size_t)count, hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(pairs.data(), c->d_pairs + p0, sizeof(rt::HotPair) * pairs.size(), hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(spairs.data(), c->d_shadow_pairs, sizeof(rt::HotPair) * spairs.size(), hipMemcpyDeviceToHost));
    for (uint32_t m = 0; m < count; ++m) {
        const uint32_t o = first + m, slot = c->h_shadow_slot[o];
        auto disagree = [&](const char* what) {
            return fail(c, RT_ERR_STATE, "rt_read_visibility: object " + std::to_string((uint64_t)o) + ": " + what);
        };
        const uint32_t word = hot[m].type;
        uint32_t bits = 0;
        std::memcpy(&bits, &cold[m].spec_type.w, 4);
        if (rec[m].type != word) return disagree("ObjectRecord::type does not hold HotObject::type");
        if (c->d_compact && compact[m].type != word) return disagree("CompactObject::type does not hold HotObject::type");
        if (bits != word) return disagree("the type bits of ColdObject::spec_type do not hold HotObject::type");
        if ((&pairs[o / 2u - p0].type_a)[o & 1u] != word) return disagree("the traversal pair stream does not hold HotObject::type");
        if ((&spairs[slot / 2u].type_a)[slot & 1u] != word) return disagree("the shadow pair stream does not hold HotObject::type");
        const uint32_t created = created_word(c->h_kind[o]);
        if (created == rt::kTypeKeep) {  // created with a type of its own: never written, reads as visible
            visible[m] = 1;
            continue;
        }
        if (word != created && word != RT_TYPE_HIDDEN) return disagree("the type word is neither the create-time type nor RT_TYPE_HIDDEN");
        visible[m] = word == created ? 1 : 0;
    }
    return RT_OK;
}

}  // extern "C"
