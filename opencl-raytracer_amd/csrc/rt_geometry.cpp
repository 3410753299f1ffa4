// rt_geometry.cpp - replaceable transforms (hip_raytracer.h): rt_set_transforms, rt_read_transforms, rt_get_geometry_info.
//
// New matrices for objects of a live context are (1) one patch pass over every record that holds a copy of them (rt_transforms.hip)
// and (2) what the host derives from an object's bound, redone for the moved objects only: the small-scene kernel's spheres,
// RT_FLAG_DEVICE_OPENCL's bounds and its predicate on the lights, and - on a context with a grid - the registration spheres, from
// build_grid's own formula (grid_radii) with the box, cell and K2 of the grid as built. The grid's tables are NOT rebuilt: a moved
// object joins the always-list (the dynamic set) and its stale registrations stay, which can only cost exact tests (DESIGN.md 4.1,
// "dynamic objects"). The light tiles, whose lists are all a ray consults, are rebuilt by their device builder.
#include "rt_context.h"

namespace rt::host {
namespace {

rt_transform record_at(const void* transforms, size_t m) {  // (any alignment)
    rt_transform t;
    std::memcpy(&t, static_cast<const uint8_t*>(transforms) + sizeof(rt_transform) * m, sizeof(t));
    return t;
}

bool bottom_rows_affine(const rt_transform& t) { return rt::host::bottom_rows_affine(t.mv, t.mvInverse); }

// what object_bound and bounding_sphere read of an object
rt_object_data as_object(const rt_transform& t, uint32_t type) {
    rt_object_data o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(o.mv, t.mv, sizeof(o.mv));
    std::memcpy(o.mvInverse, t.mvInverse, sizeof(o.mvInverse));
    o.type = type;
    return o;
}

bool on_always_list(const rt_context* c, uint32_t object) { return std::find(c->h_always.begin(), c->h_always.end(), object) != c->h_always.end(); }

uint32_t dynamic_capacity(const rt_context* c) { return c->grid.enabled && c->n_unbounded < kMaxAlways ? kMaxAlways - c->n_unbounded : 0u; }

// Every refusal, over the whole range; the bounds of the accepted transforms for the caller that goes on (or null).
int plan_transforms(rt_context* c, const void* transforms, uint32_t first, uint32_t count, std::vector<Bound>* bounds_out) {
    const int refused = check_object_range(c, transforms, first, count, "transforms", true);
    if (refused || count == 0) return refused;
    for (uint32_t m = 0; m < count; ++m)
        if ((c->h_kind[first + m] & 0x7fu) > 1u)
            return fail(c, RT_ERR_INVALID_ARGUMENT, "object " + std::to_string((uint64_t)first + m) +
                                                        " is neither a sphere nor a box: only their records hold the two matrices (a triangle's mv holds vertices)");
    std::vector<Bound> bounds(count);
    std::atomic<uint32_t> bad_affine{0xffffffffu};
    parallel_for(count, 4096, [&](size_t m0, size_t m1) {
        for (size_t m = m0; m < m1; ++m) {
            const rt_transform t = record_at(transforms, m);
            if (c->affine_w && !bottom_rows_affine(t)) {
                uint32_t seen = bad_affine.load();
                while ((uint32_t)m < seen && !bad_affine.compare_exchange_weak(seen, (uint32_t)m)) {}
            }
            bounds[m] = object_bound(as_object(t, c->h_kind[first + m] & 0x7fu));
        }
    });
    if (bad_affine.load() != 0xffffffffu)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "object " + std::to_string((uint64_t)first + bad_affine.load()) +
                                                    ": a bottom row of mv or mvInverse is not (0,0,0,1), on a context whose instances are all affine");
    if (!c->degenerate_literal)
        for (uint32_t m = 0; m < count; ++m)
            if (!std::isfinite(bounds[m].r))
                return fail(c, RT_ERR_INVALID_ARGUMENT, "object " + std::to_string((uint64_t)first + m) +
                                                            ": the transform has no finite bound (singular or non-finite mvInverse); a fresh context renders it by the literal loops");
    if (c->grid.enabled) {
        for (uint32_t m = 0; m < count; ++m) {
            const Bound& b = bounds[m];
            const double cc[3] = {b.x, b.y, b.z}, pad = b.r * 1.01;  // (build_grid's own padding of a bound)
            bool inside = std::isfinite(b.r);
            for (int a = 0; a < 3 && inside; ++a) inside = cc[a] - pad >= c->grid_box_lo[a] && cc[a] + pad <= c->grid_box_hi[a];
            if (!inside)
                return fail(c, RT_ERR_INVALID_ARGUMENT, "object " + std::to_string((uint64_t)first + m) +
                                                            ": the new bound leaves the box the grid was built for (rt_get_rays_info: box_lo, box_hi)");
        }
        const uint32_t room = kMaxAlways - std::min<uint32_t>(kMaxAlways, (uint32_t)c->h_always.size());
        uint32_t fresh = 0;
        for (uint32_t m = 0; m < count && fresh <= room; ++m) fresh += on_always_list(c, first + m) ? 0u : 1u;
        if (fresh > room)
            return fail(c, RT_ERR_STATE, "the dynamic set is full: a context with a grid keeps at most " + std::to_string(dynamic_capacity(c)) +
                                             " moved objects (rt_get_geometry_info)");
    }
    if (bounds_out) bounds_out->swap(bounds);
    return RT_OK;
}

}  // namespace

int check_set_transforms(rt_context* c, const void* transforms, uint32_t first, uint32_t count) {
    return plan_transforms(c, transforms, first, count, nullptr);
}

}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_set_transforms(rt_context* c, const void* transforms, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    std::vector<Bound> bounds;
    const int refused = plan_transforms(c, transforms, first, count, &bounds);
    if (refused) return refused;
    if (count == 0) return RT_OK;
    RT_DEVICE(c);
    // ---- the records ----
    const size_t slots_at = sizeof(rt_transform) * (size_t)count;  // the shadow slots behind THIS call's records (a multiple of 128)
    const int staged = ensure_patch_stage(c, slots_at + sizeof(uint32_t) * (size_t)count);
    if (staged != RT_OK) return staged;
    for (hipEvent_t& e : c->ev_xf)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    std::vector<uint32_t> slots(c->h_shadow_slot.begin() + first, c->h_shadow_slot.begin() + first + count);
    uint8_t* stage = static_cast<uint8_t*>(c->d_patch_stage.p);
    RT_HIP(c, hipEventRecord(c->ev_xf[0], c->stream));
    // (the copies take the bytes as they are: `transforms` may have any alignment)
    RT_HIP(c, hipMemcpyAsync(stage, transforms, slots_at, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(stage + slots_at, slots.data(), sizeof(uint32_t) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    const rt::TransformTargets to{c->d_pairs, c->d_shadow_pairs, c->d_hot, c->d_cold, c->d_objrec, c->d_compact, c->n_objs};
    const hipError_t e = rt::launch_patch_transforms(reinterpret_cast<const float*>(stage), reinterpret_cast<const uint32_t*>(stage + slots_at), first,
                                                     count, to, c->stream);
    if (e != hipSuccess) return fail_hip(c, e, "transform patch launch");
    RT_HIP(c, hipEventRecord(c->ev_xf[1], c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));  // synchronous like rt_set_lights: the array is the caller's again, any stream's next frame sees it
    float patch_ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&patch_ms, c->ev_xf[0], c->ev_xf[1]));
    c->geo_info.patch_device_ms = (double)patch_ms;
    c->geo_info.light_tiles_rebuilt = 0;

    // ---- what the host keeps of an object's matrices ----
    for (uint32_t m = 0; m < count; ++m) {
        const rt_transform t = record_at(transforms, m);
        uint8_t& kind = c->h_kind[first + m];
        const bool was = !(kind & 0x80u), is = bottom_rows_affine(t);
        if (was != is) {
            c->n_not_affine = is ? c->n_not_affine - 1u : c->n_not_affine + 1u;
            kind = (uint8_t)((kind & 0x7fu) | (is ? 0u : 0x80u));
        }
        if (c->d_compact) {  // the scene's `diagonal` may flip either way (compact_in_use): the compact records follow every call
            uint8_t& off = c->h_not_diagonal[first + m];
            const uint8_t now = object_not_diagonal(kind & 0x7fu, t.mv, t.mvInverse) ? 1 : 0;
            c->n_not_diagonal = c->n_not_diagonal - off + now;
            off = now;
        }
        if (c->h_spheres.size() == 4 * (size_t)c->n_objs) {  // the small-scene kernel's culling rectangles follow (do_launch)
            const Sphere sp = bounding_sphere(as_object(t, kind & 0x7fu));
            double* s = &c->h_spheres[4 * (size_t)(first + m)];
            s[0] = sp.x; s[1] = sp.y; s[2] = sp.z; s[3] = sp.r;
        }
        if (c->h_obj_bounds.size() == 4 * (size_t)c->n_objs) {
            double* s = &c->h_obj_bounds[4 * (size_t)(first + m)];
            s[0] = bounds[m].x; s[1] = bounds[m].y; s[2] = bounds[m].z; s[3] = bounds[m].r;
        }
    }
    c->affine_w = c->n_not_affine == 0;
    c->rects_dirty = true;
    refresh_lights_literal(c, c->h_lights.data(), c->n_lights);  // (the predicate on the lights, for the objects where they now are)
    if (!c->grid.enabled) return RT_OK;

    // ---- the grid: registration spheres for where the objects are, the dynamic set, the light tiles ----
    GridRadii gr;
    for (int a = 0; a < 3; ++a) { gr.lo[a] = c->grid_box_lo[a]; gr.hi[a] = c->grid_box_hi[a]; }
    gr.cell = c->grid_cell;
    gr.diag = c->grid_diag;
    gr.S_max = c->grid_s_max;
    const size_t n_before = c->h_always.size();
    for (uint32_t m = 0; m < count; ++m) {
        const uint32_t i = first + m;
        const ObjectRadii r = grid_radii(gr, bounds[m], c->h_kind[i] & 0x7fu, c->grid_k2);
        double* s = &c->h_grid_spheres[4 * (size_t)i];
        s[0] = bounds[m].x; s[1] = bounds[m].y; s[2] = bounds[m].z; s[3] = r.rg;
        c->h_grid_pre[i] = pretest_as_stored(r.rpre);
        if (!on_always_list(c, i)) c->h_always.push_back(i);  // (plan_transforms made sure of the room)
        if (c->h_obj_bound6.size() == rt::kBoundDoubles * (size_t)c->n_objs) {  // the bound a pose outside the box makes its sphere from
            double* b = &c->h_obj_bound6[rt::kBoundDoubles * (size_t)i];
            b[0] = bounds[m].x; b[1] = bounds[m].y; b[2] = bounds[m].z; b[3] = bounds[m].r; b[4] = bounds[m].kappa2;
        }
    }
    if (c->d_obj_bound6 && c->h_obj_bound6.size() == rt::kBoundDoubles * (size_t)c->n_objs)
        RT_HIP(c, hipMemcpy(c->d_obj_bound6 + rt::kBoundDoubles * (size_t)first, &c->h_obj_bound6[rt::kBoundDoubles * (size_t)first],
                            sizeof(double) * rt::kBoundDoubles * (size_t)count, hipMemcpyHostToDevice));
    if (c->d_pose_spheres)
        RT_HIP(c, hipMemcpy(c->d_pose_spheres + 4 * (size_t)first, &c->h_grid_spheres[4 * (size_t)first], sizeof(double) * 4 * (size_t)count, hipMemcpyHostToDevice));
    if (c->d_lt_pre)
        RT_HIP(c, hipMemcpy(c->d_lt_pre + first, &c->h_grid_pre[first], sizeof(float) * (size_t)count, hipMemcpyHostToDevice));
    if (c->h_always.size() != n_before) {
        RT_HIP(c, hipMemcpy(c->d_grid_always + n_before, c->h_always.data() + n_before, sizeof(uint32_t) * (c->h_always.size() - n_before), hipMemcpyHostToDevice));
        c->grid.n_always = (uint32_t)c->h_always.size();  // (do_launch hands c->grid to the round machine every frame)
    }
    // The current screen tiles stay: wf_trace_primary_tiles tests the always-list for every wave, and a stale entry keeps its place in
    // the depth order. The light tiles do not: their lists are all last_light_blocked consults.
    const int rc = build_light_tiles_device(c, c->h_lights.data());
    if (rc != RT_OK) return rc;
    c->geo_info.light_tiles_rebuilt = c->lt_info.enabled ? 1u : 0u;
    return RT_OK;
}

int rt_read_transforms(rt_context* c, void* transforms, uint32_t first, uint32_t count) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_object_range(c, transforms, first, count, "transforms", true);
    if (refused || count == 0) return refused;
    for (uint32_t m = 0; m < count; ++m)
        if ((c->h_kind[first + m] & 0x7fu) > 1u)
            return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_read_transforms: object " + std::to_string((uint64_t)first + m) + " is neither a sphere nor a box");
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
    uint8_t* out = static_cast<uint8_t*>(transforms);  // (any alignment: the records are assembled here and copied out)
    auto word = [](const float4& v, int k) { return (&v.x)[k]; };
    auto same = [](float a, float b) { return std::memcmp(&a, &b, 4) == 0; };
    for (uint32_t m = 0; m < count; ++m) {
        const uint32_t o = first + m, slot = c->h_shadow_slot[o];
        const rt::HotPair& hp = pairs[o / 2u - p0];
        const rt::HotPair& sp = spairs[slot / 2u];
        const float4* hrow = &hot[m].row0;
        auto disagree = [&](const char* what) {
            return fail(c, RT_ERR_STATE, "rt_read_transforms: object " + std::to_string((uint64_t)o) + ": " + what);
        };
        rt_transform t;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) {
                const float v = word(hrow[r], k);
                if (!same(v, word(rec[m].inv_row[r], k))) return disagree("ObjectRecord::inv_row does not hold the bits of HotObject's rows");
                if (!same(v, hp.m[4 * r + k][o & 1u])) return disagree("the traversal pair stream does not hold the bits of HotObject's rows");
                if (!same(v, sp.m[4 * r + k][slot & 1u])) return disagree("the shadow pair stream does not hold the bits of HotObject's rows");
                if (!same(word(cold[m].mv_row[r], k), word(rec[m].mv_row[r], k))) return disagree("ObjectRecord::mv_row does not hold the bits of ColdObject::mv_row");
                t.mvInverse[4 * k + r] = v;
            }
        for (int k = 0; k < 4; ++k) {
            t.mvInverse[4 * k + 3] = word(cold[m].inv_row3, k);
            for (int r = 0; r < 4; ++r) t.mv[4 * k + r] = word(cold[m].mv_row[r], k);
        }
        if (c->d_compact) {  // the twelve matrix words of the compact record: what pack_compact takes of the two matrices
            const rt::CompactObject want = pack_compact(t.mv, t.mvInverse, compact[m].type, compact[m].absorption);
            if (std::memcmp(&want, &compact[m], 12) != 0 || std::memcmp(&want.b0, &compact[m].b0, 12) != 0 || std::memcmp(&want.s0, &compact[m].s0, 12) != 0 ||
                std::memcmp(&want.x, &compact[m].x, 12) != 0)
                return disagree("the CompactObject does not hold the diagonal and the translation of the two matrices");
        }
        std::memcpy(out + sizeof(rt_transform) * (size_t)m, &t, sizeof(t));
    }
    return RT_OK;
}

int rt_get_compact_info(const rt_context* c, rt_compact_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    *info = rt_compact_info_t{};
    info->table_built = c->d_compact ? 1u : 0u;
    info->n_not_diagonal = c->n_not_diagonal;
    info->allowed = c->compact_allowed ? 1u : 0u;
    info->in_use = compact_in_use(c);
    return RT_OK;
}

int rt_get_block_range(const rt_context* c, rt_block_range_t* range) {
    if (!c || !range) return RT_ERR_INVALID_ARGUMENT;
    *range = rt_block_range_t{};
    const rt::BlockGrid& b = c->blocks;
    if (!b.enabled) return RT_OK;
    range->built = 1u;
    const int32_t cells[3] = {b.nx, b.ny, b.nz};
    bool whole = true;
    for (int a = 0; a < 3; ++a) {
        range->cells[a] = cells[a];
        range->lo[a] = c->block_occ[a];
        range->hi[a] = c->block_occ[3 + a];
        whole = whole && range->lo[a] == 0 && range->hi[a] == cells[a] - 1;
    }
    range->whole_grid = whole ? 1u : 0u;
    range->cell = b.cell;
    range->face_lo[0] = b.occ.lox; range->face_lo[1] = b.occ.loy; range->face_lo[2] = b.occ.loz;
    range->face_hi[0] = b.occ.hix; range->face_hi[1] = b.occ.hiy; range->face_hi[2] = b.occ.hiz;
    return RT_OK;
}

int rt_get_geometry_info(const rt_context* c, rt_geometry_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    *info = c->geo_info;
    info->grid_built = c->grid.enabled ? 1u : 0u;
    if (!c->grid.enabled) return RT_OK;
    info->n_unbounded = c->n_unbounded;
    info->dynamic_capacity = dynamic_capacity(c);
    info->n_dynamic = (uint32_t)c->h_always.size() - c->n_unbounded;
    for (uint32_t k = 0; k < info->n_dynamic && k < kMaxAlways; ++k) info->dynamic_ids[k] = c->h_always[c->n_unbounded + k];
    return RT_OK;
}

}  // extern "C"
