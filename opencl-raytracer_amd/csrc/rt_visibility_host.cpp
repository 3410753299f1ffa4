// rt_visibility_host.cpp - replaceable visibility (hip_raytracer.h): rt_set_visibility, rt_set_visibility_device, rt_read_visibility.
// Hiding an object is writing RT_TYPE_HIDDEN into every copy of its type word, showing it is writing the create-time word back: one
// patch pass (rt_visibility.hip). No table is rebuilt - a table entry is only a candidate, and the exact test of a
// type that is none of 0, 1, 2 never hits. What the host derives from the types follows from a mirror of the mask: the NaN-ray winner
// (the last VISIBLE sphere or box) and, under RT_FLAG_DEVICE_OPENCL, the predicate on the lights, which skips hidden objects.
#include "rt_context.h"
#include "rt_device.h"

namespace rt::host {

int check_set_visibility(rt_context* c, const void* visible, uint32_t first, uint32_t count) {
    if ((uint64_t)first + (uint64_t)count > (uint64_t)c->n_objs)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "first + count exceeds the context's object count");
    if (count && !visible) return fail(c, RT_ERR_INVALID_ARGUMENT, "visible is NULL with a non-zero count");
    return RT_OK;
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
    for (uint32_t m = 0; m < count; ++m)
        c->h_hidden[first + m] = (mask[m] == 0 && created_word(c->h_kind[first + m]) != rt::kTypeKeep) ? 1 : 0;
    // the last sphere / box of the scene decides what a NaN ray ends with (rt_create): the last VISIBLE one
    c->nan_winner = -1;
    c->nan_winner_sphere = false;
    for (uint32_t i = c->n_objs; i-- > 0;) {
        const uint32_t ty = c->h_kind[i] & 0x7fu;
        if (ty <= 1u && !c->h_hidden[i]) { c->nan_winner = (int)i; c->nan_winner_sphere = (ty == 0u); break; }
    }
    // RT_FLAG_DEVICE_OPENCL's predicate on the lights, without the hidden objects (as rt_set_lights evaluates it for new lights)
    if ((c->user_flags & RT_FLAG_DEVICE_OPENCL) && !(c->user_flags & RT_FLAG_LITERAL) && !c->degenerate_literal &&
        c->h_obj_bounds.size() == 4 * (size_t)c->n_objs) {
        c->lights_literal = lights_need_literal(c, c->h_lights.data(), c->n_lights);
        if (c->base_flags != (c->user_flags | (c->lights_literal ? RT_FLAG_LITERAL : 0u))) c->tiles_dirty = true;  // (a table's verdict depends on the literal flag)
        c->base_flags = c->user_flags | (c->lights_literal ? RT_FLAG_LITERAL : 0u);
        c->forced_literal = c->lights_literal;
        apply_ray_domain(c);
    }
}

struct VisibilityTrace {  // three events when RT_VISIBILITY_TRACE is set, destroyed on every exit path
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on = false;
    ~VisibilityTrace() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// d_src: `count` bytes in device memory, valid behind what `stream` holds already. Enqueues the patch there and waits for it.
// ev (or null): three events, [0] recorded by the caller before its upload, if any.
int patch_visibility_on(rt_context* c, const uint8_t* d_src, uint32_t first, uint32_t count, hipStream_t stream, hipEvent_t* ev) {
    if (ev) RT_HIP(c, hipEventRecord(ev[1], stream));
    const rt::VisibilityTargets to{c->d_pairs, c->d_shadow_pairs, c->d_hot, c->d_cold, c->d_objrec, c->d_vis_types, c->d_vis_slots, c->n_objs};
    const hipError_t e = rt::launch_patch_visibility(d_src, first, count, to, stream);
    if (e != hipSuccess) return fail_hip(c, e, "visibility patch launch");
    if (ev) RT_HIP(c, hipEventRecord(ev[2], stream));
    return RT_OK;
}

int report(rt_context* c, hipEvent_t* ev, uint32_t count) {  // engineering aid (RT_VISIBILITY_TRACE=1, tools/ab/set_visibility_timing.py)
    float copy_ms = 0.f, patch_ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&copy_ms, ev[0], ev[1]));
    RT_HIP(c, hipEventElapsedTime(&patch_ms, ev[1], ev[2]));
    std::fprintf(stderr, "[rt_set_visibility] copy %.4f ms patch %.4f ms objects %u\n", (double)copy_ms, (double)patch_ms, count);
    return RT_OK;
}

}  // namespace
}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_set_visibility_device(rt_context* c, const void* d_visible, uint32_t first, uint32_t count, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_visibility(c, d_visible, first, count);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    const int rc = ensure_support(c);
    if (rc != RT_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);  // NULL: the legacy default stream, as for rt_set_materials_device
    std::vector<uint8_t> mask(count);
    VisibilityTrace trace;
    if (std::getenv("RT_VISIBILITY_TRACE")) {
        for (hipEvent_t& e : trace.ev) RT_HIP(c, hipEventCreate(&e));
        trace.on = true;
        RT_HIP(c, hipEventRecord(trace.ev[0], stream));
    }
    const int launched = patch_visibility_on(c, static_cast<const uint8_t*>(d_visible), first, count, stream, trace.on ? trace.ev : nullptr);
    if (launched != RT_OK) return launched;
    // the bytes the pass read, for the host's mirror (behind the pass on the same stream: the caller's kernels have written them)
    RT_HIP(c, hipMemcpyAsync(mask.data(), d_visible, (size_t)count, hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));  // synchronous like rt_set_materials: the mask is the caller's again, any stream's next frame sees it
    follow_the_types(c, mask.data(), first, count);
    return trace.on ? report(c, trace.ev, count) : RT_OK;
}

int rt_set_visibility(rt_context* c, const uint8_t* visible, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_visibility(c, visible, first, count);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    const int rc = ensure_support(c);
    if (rc != RT_OK) return rc;
    if (count > c->vis_stage_capacity) {  // grow-only; a failed allocation leaves the context as it was
        void* d = nullptr;
        RT_HIP(c, hipMalloc(&d, (size_t)count));
        if (c->d_vis_stage) (void)hipFree(c->d_vis_stage);
        c->d_vis_stage = d;
        c->vis_stage_capacity = count;
    }
    VisibilityTrace trace;
    if (std::getenv("RT_VISIBILITY_TRACE")) {
        for (hipEvent_t& e : trace.ev) RT_HIP(c, hipEventCreate(&e));
        trace.on = true;
        RT_HIP(c, hipEventRecord(trace.ev[0], c->stream));
    }
    RT_HIP(c, hipMemcpyAsync(c->d_vis_stage, visible, (size_t)count, hipMemcpyHostToDevice, c->stream));
    const int launched = patch_visibility_on(c, static_cast<const uint8_t*>(c->d_vis_stage), first, count, c->stream, trace.on ? trace.ev : nullptr);
    if (launched != RT_OK) return launched;
    RT_HIP(c, hipStreamSynchronize(c->stream));  // synchronous like rt_set_materials
    follow_the_types(c, visible, first, count);
    return trace.on ? report(c, trace.ev, count) : RT_OK;
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
