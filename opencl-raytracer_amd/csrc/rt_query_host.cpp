// rt_query_host.cpp - ray queries (hip_raytracer.h): rt_query_closest_device, rt_query_occluded_device, their host twins
// rt_query_closest / rt_query_occluded, rt_query_primary, the hit-record queries rt_query_hits_device / rt_query_hits /
// rt_query_primary_hits, the shaded queries rt_query_shade_device / rt_query_shade / rt_query_primary_shade with their own
// rt_get_query_shade_info, and rt_get_query_info. A query reads the context's object records and grid as
// the setters have left them and writes the caller's outputs and the context's counter block - nothing of the frame: not its rays,
// camera, pose, shard, supersampling factor, aux buffers or state buffers. The device forms enqueue a memset, two event records and one
// kernel (rt_query.hip) and return; after the first call, which makes the counter block and the events, nothing is allocated.
#include "rt_context.h"

namespace rt::host {

// shared with the G-buffer pass (rt_render.cpp), declared in rt_context.h
// the records as do_launch hands them to a frame (rt_api.cpp); a query reads the traversal's part of them
rt::Scene query_scene(const rt_context* c) {
    rt::Scene s = {};
    s.pairs = c->d_pairs;
    s.n_pairs = c->n_pairs;
    s.hot = c->d_hot;
    s.bounds = c->d_bounds;
    s.cold = c->d_cold;
    s.objrec = c->d_objrec;
    s.lights = c->d_lights;
    s.n_objs = c->n_objs;
    s.n_lights = c->n_lights;
    s.affine = (c->affine_w && !c->has_triangles) ? 1u : 0u;
    s.nan_winner = c->nan_winner;
    s.nan_winner_sphere = c->nan_winner_sphere ? 1u : 0u;
    return s;
}

// RT_FLAG_FAST_PHONG does not touch t: the mode is the two arithmetic flags'
int query_arith(const rt_context* c) {
    return (c->flags & RT_FLAG_DEVICE_OPENCL) ? rt::kDeviceCL : ((c->flags & RT_FLAG_UNFUSED) ? rt::kUnfused : rt::kFused);
}

// the context's own primary rays, for rt_query_primary / rt_query_primary_hits
rt::QueryCamera query_camera(const rt_context* c) {
    rt::QueryCamera cam = {};
    cam.rays = c->pinhole ? nullptr : c->d_rays;
    cam.pinhole = c->pinhole ? 1u : 0u;
    cam.width = c->width ? c->width : 1;
    cam.half_w = (float)c->width / 2.0f;
    cam.half_h = (float)c->height / 2.0f;
    cam.height_f = (float)c->height;
    cam.z = c->z;
    return cam;
}

namespace {

// rt_context::grid_box_lo / hi as floats that lie INSIDE the double box: lo rounded up, hi rounded down
float round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return f;
}
float round_down(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
    return f;
}

// The grid serves queries unless the context is literal by its OBJECTS or by the caller's wish: a degenerate instance (singular or
// non-finite mvInverse: NaN times for finite rays, so the result depends on the order of the loop - rt_create, "instance checks")
// or RT_FLAG_LITERAL itself. build_grid builds a grid for such a context all the same (the frames leave it alone: use_grid =
// grid.enabled && !literal); the order-free walks must not answer there. The frame-level reasons for RT_FLAG_LITERAL - the rays in
// use left the domain, RT_FLAG_DEVICE_OPENCL's predicate on the lights - concern the frame's rays and zero-direction shadow rays, not
// a query's: they play no part.
bool grid_serves_queries(const rt_context* c) {
    return c->grid.enabled && !(c->user_flags & RT_FLAG_LITERAL) && !c->degenerate_literal;
}

rt::QueryBox query_box(const rt_context* c) {
    rt::QueryBox b = {};
    b.grid = grid_serves_queries(c) ? 1u : 0u;
    if (!b.grid) return b;
    b.lox = round_up(c->grid_box_lo[0]); b.loy = round_up(c->grid_box_lo[1]); b.loz = round_up(c->grid_box_lo[2]);
    b.hix = round_down(c->grid_box_hi[0]); b.hiy = round_down(c->grid_box_hi[1]); b.hiz = round_down(c->grid_box_hi[2]);
    return b;
}

int refuse_triangles(rt_context* c) {
    if (c->has_triangles)
        return fail(c, RT_ERR_STATE, "ray queries on a context with triangle records: the ordered loop over the pair stream does not know type 2, "
                                     "so no ray could be guaranteed a route");
    return RT_OK;
}

// what the device forms and the host twins refuse of (rays, n); nothing is touched
int check_query_rays(rt_context* c, const void* rays, uint64_t n, bool device) {
    if (n != 0 && !rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "the ray array is NULL with a non-zero count");
    if (device && (reinterpret_cast<uintptr_t>(rays) & 15u)) return fail(c, RT_ERR_INVALID_ARGUMENT, "the ray array must be 16-byte aligned");
    if (n > (std::numeric_limits<uint64_t>::max)() / sizeof(rt_ray)) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many rays");
    return RT_OK;
}

// the counter block and the event pair: made by the first query
int ensure_query_support(rt_context* c) {
    if (!c->d_query_counters) RT_HIP(c, hipMalloc((void**)&c->d_query_counters, sizeof(rt::QueryCounters)));
    for (hipEvent_t& e : c->ev_query)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    return RT_OK;
}

enum class Kind { Closest, Occluded, Primary };

// One query on `stream`: counters zeroed, event, kernel, event. All pointers are device memory; `d_in` the rays or, for Kind::Primary, the
// work-items. Asynchronous.
int enqueue_query(rt_context* c, Kind kind, const void* d_in, uint64_t n, float* d_t, int32_t* d_index, uint8_t* d_occluded, hipStream_t stream) {
    if (const int rc = ensure_query_support(c)) return rc;
    const rt::Scene scene = query_scene(c);
    const rt::QueryBox box = query_box(c);
    const rt::GridDesc grid = box.grid ? c->grid : rt::GridDesc{};
    const int arith = query_arith(c);
    RT_HIP(c, hipMemsetAsync(c->d_query_counters, 0, sizeof(rt::QueryCounters), stream));
    RT_HIP(c, hipEventRecord(c->ev_query[0], stream));
    hipError_t e = hipSuccess;
    if (kind == Kind::Closest) {
        e = rt::launch_query_closest(scene, grid, box, arith, static_cast<const float4*>(d_in), n, d_t, d_index, c->d_query_counters, stream);
    } else if (kind == Kind::Occluded) {
        e = rt::launch_query_occluded(scene, grid, box, arith, static_cast<const float4*>(d_in), n, d_occluded, c->d_query_counters, stream);
    } else {
        e = rt::launch_query_primary(scene, grid, box, arith, query_camera(c), static_cast<const uint64_t*>(d_in), n, d_t, d_index, c->d_query_counters, stream);
    }
    if (e != hipSuccess) return fail_hip(c, e, "query launch");
    RT_HIP(c, hipEventRecord(c->ev_query[1], stream));
    c->query_made = true;
    return RT_OK;
}

size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// The host twins and rt_query_primary: input and results staged in the context's patch buffer (rt_object_patch.cpp), on the context's
// stream; synchronous. `in_bytes` bytes of input per element.
int query_from_host(rt_context* c, Kind kind, const void* in, size_t in_bytes, uint64_t n, float* t, int32_t* index, uint8_t* occluded) {
    RT_DEVICE(c);
    const size_t off_t = align16(in_bytes * (size_t)n);
    const size_t off_index = off_t + align16(sizeof(float) * (size_t)n);
    const size_t off_occ = off_index + align16(sizeof(int32_t) * (size_t)n);
    if (const int rc = ensure_patch_stage(c, off_occ + align16((size_t)n))) return rc;
    char* const stage = static_cast<char*>(c->d_patch_stage.p);
    float* const d_t = t ? reinterpret_cast<float*>(stage + off_t) : nullptr;
    int32_t* const d_index = index ? reinterpret_cast<int32_t*>(stage + off_index) : nullptr;
    uint8_t* const d_occ = occluded ? reinterpret_cast<uint8_t*>(stage + off_occ) : nullptr;
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(stage, in, in_bytes * (size_t)n, hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_query(c, kind, stage, n, d_t, d_index, d_occ, stream)) return rc;
    if (t) RT_HIP(c, hipMemcpyAsync(t, d_t, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, stream));
    if (index) RT_HIP(c, hipMemcpyAsync(index, d_index, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    if (occluded) RT_HIP(c, hipMemcpyAsync(occluded, d_occ, (size_t)n, hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- hit records ---------------------------------------------------------------------------------------------------------------------
// One hit-record query on `stream`, as enqueue_query: `d_in` the rays or, with `primary`, the work-items; `hits` device pointers.
int enqueue_hits(rt_context* c, bool primary, const void* d_in, uint64_t n, const int32_t* d_mask, const rt::QueryHits& hits, hipStream_t stream) {
    if (const int rc = ensure_query_support(c)) return rc;
    const rt::Scene scene = query_scene(c);
    const rt::QueryBox box = query_box(c);
    const rt::GridDesc grid = box.grid ? c->grid : rt::GridDesc{};
    const int arith = query_arith(c);
    RT_HIP(c, hipMemsetAsync(c->d_query_counters, 0, sizeof(rt::QueryCounters), stream));
    RT_HIP(c, hipEventRecord(c->ev_query[0], stream));
    const hipError_t e = primary ? rt::launch_query_primary_hits(scene, grid, box, arith, query_camera(c), static_cast<const uint64_t*>(d_in), n, hits,
                                                                 c->d_query_counters, stream)
                                 : rt::launch_query_hits(scene, grid, box, arith, static_cast<const float4*>(d_in), n, d_mask, hits,
                                                         c->d_query_counters, stream);
    if (e != hipSuccess) return fail_hip(c, e, "hit-record query launch");
    RT_HIP(c, hipEventRecord(c->ev_query[1], stream));
    c->query_made = true;
    return RT_OK;
}

rt::QueryHits device_hits(const rt_hits_t& o) {
    return rt::QueryHits{o.t, o.index, reinterpret_cast<float4*>(o.point), reinterpret_cast<float4*>(o.normal), static_cast<float4*>(o.reflected)};
}

// what every form refuses of the output struct; `device`: its members are device pointers, whose alignment the kernel's stores need
int check_hits(rt_context* c, const rt_hits_t* o, bool device) {
    if (!o) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output struct is NULL");
    if (!o->t && !o->index && !o->point && !o->normal && !o->reflected) return fail(c, RT_ERR_INVALID_ARGUMENT, "all outputs are NULL");
    if (!device) return RT_OK;
    if ((reinterpret_cast<uintptr_t>(o->t) | reinterpret_cast<uintptr_t>(o->index)) & 3u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "t and index must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(o->point) | reinterpret_cast<uintptr_t>(o->normal) | reinterpret_cast<uintptr_t>(o->reflected)) & 15u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "point, normal and reflected must be 16-byte aligned");
    return RT_OK;
}

// What hits_from_host stages per element, at most: the input (a 32-byte ray or an 8-byte work-item), the mask, t, index, point, normal
// and the reflected ray; each of the first four arrays is padded to 16 bytes once.
constexpr size_t kHitsStageBytesPerElement = sizeof(rt_ray) + 3 * 4 + 16 + 16 + sizeof(rt_ray);
constexpr size_t kHitsStagePadding = 4 * 16;
int check_hits_count(rt_context* c, uint64_t n) {
    if (n > ((std::numeric_limits<size_t>::max)() - kHitsStagePadding) / kHitsStageBytesPerElement)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "too many elements: the staged records would not fit an address");
    return RT_OK;
}

// The host forms: input, mask and the requested records staged in the context's patch buffer on the context's stream; synchronous.
int hits_from_host(rt_context* c, bool primary, const void* in, size_t in_bytes, uint64_t n, const int32_t* mask, const rt_hits_t& out) {
    RT_DEVICE(c);
    const size_t count = (size_t)n;
    const size_t off_mask = align16(in_bytes * count);
    const size_t off_t = off_mask + align16(sizeof(int32_t) * count);
    const size_t off_index = off_t + align16(sizeof(float) * count);
    const size_t off_point = off_index + align16(sizeof(int32_t) * count);
    const size_t off_normal = off_point + 16 * count;
    const size_t off_refl = off_normal + 16 * count;
    if (const int rc = ensure_patch_stage(c, off_refl + sizeof(rt_ray) * count)) return rc;
    char* const stage = static_cast<char*>(c->d_patch_stage.p);
    rt::QueryHits d = {};
    d.t = out.t ? reinterpret_cast<float*>(stage + off_t) : nullptr;
    d.index = out.index ? reinterpret_cast<int32_t*>(stage + off_index) : nullptr;
    d.point = out.point ? reinterpret_cast<float4*>(stage + off_point) : nullptr;
    d.normal = out.normal ? reinterpret_cast<float4*>(stage + off_normal) : nullptr;
    d.reflected = out.reflected ? reinterpret_cast<float4*>(stage + off_refl) : nullptr;
    int32_t* const d_mask = mask ? reinterpret_cast<int32_t*>(stage + off_mask) : nullptr;
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(stage, in, in_bytes * count, hipMemcpyHostToDevice, stream));
    if (mask) RT_HIP(c, hipMemcpyAsync(d_mask, mask, sizeof(int32_t) * count, hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_hits(c, primary, stage, n, d_mask, d, stream)) return rc;
    if (out.t) RT_HIP(c, hipMemcpyAsync(out.t, d.t, sizeof(float) * count, hipMemcpyDeviceToHost, stream));
    if (out.index) RT_HIP(c, hipMemcpyAsync(out.index, d.index, sizeof(int32_t) * count, hipMemcpyDeviceToHost, stream));
    if (out.point) RT_HIP(c, hipMemcpyAsync(out.point, d.point, 16 * count, hipMemcpyDeviceToHost, stream));
    if (out.normal) RT_HIP(c, hipMemcpyAsync(out.normal, d.normal, 16 * count, hipMemcpyDeviceToHost, stream));
    if (out.reflected) RT_HIP(c, hipMemcpyAsync(out.reflected, d.reflected, sizeof(rt_ray) * count, hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- shaded queries ------------------------------------------------------------------------------------------------------------------
// Every path of a shaded query is literal on a context that is literal by its OBJECTS, by the caller's wish or by its LIGHTS
// (RT_FLAG_DEVICE_OPENCL's predicate, rt_light_setup.cpp: a zero-direction shadow ray has no order-free answer) - the reasons that do
// not depend on the frame's rays. The first two also keep the grid from answering (grid_serves_queries); the third does not.
bool shade_context_literal(const rt_context* c) {
    return (c->user_flags & RT_FLAG_LITERAL) || c->degenerate_literal || c->lights_literal;
}

int refuse_shade_context(rt_context* c) {
    if (c->kernel == RT_KERNEL_HITTEST)
        return fail(c, RT_ERR_STATE, "shaded queries on an RT_KERNEL_HITTEST context: a time is not a colour (rt_query_closest answers there)");
    return refuse_triangles(c);
}

int check_shade(rt_context* c, const rt_shade_t* o, bool device) {
    if (!o) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output struct is NULL");
    if (!o->rgba && !o->t && !o->index) return fail(c, RT_ERR_INVALID_ARGUMENT, "all outputs are NULL");
    if (!device) return RT_OK;
    if ((reinterpret_cast<uintptr_t>(o->t) | reinterpret_cast<uintptr_t>(o->index)) & 3u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "t and index must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(o->rgba) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "rgba must be 16-byte aligned");
    return RT_OK;
}

int ensure_shade_support(rt_context* c) {
    if (!c->d_query_shade_counters) RT_HIP(c, hipMalloc((void**)&c->d_query_shade_counters, sizeof(rt::QueryShadeCounters)));
    for (hipEvent_t& e : c->ev_query_shade)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    return RT_OK;
}

// One shaded query on `stream`, as enqueue_hits: `d_in` the rays or, with `primary`, the work-items; `out` device pointers.
int enqueue_shade(rt_context* c, bool primary, const void* d_in, uint64_t n, const int32_t* d_mask, const rt::QueryShade& out, hipStream_t stream) {
    if (const int rc = ensure_shade_support(c)) return rc;
    rt::Scene scene = query_scene(c);
    scene.literal = shade_context_literal(c) ? 1u : 0u;
    scene.fast_phong = (c->flags & RT_FLAG_FAST_PHONG) ? 1u : 0u;
    const rt::QueryBox box = query_box(c);
    const rt::GridDesc grid = box.grid ? c->grid : rt::GridDesc{};
    RT_HIP(c, hipMemsetAsync(c->d_query_shade_counters, 0, sizeof(rt::QueryShadeCounters), stream));
    RT_HIP(c, hipEventRecord(c->ev_query_shade[0], stream));
    const hipError_t e = rt::launch_query_shade(scene, grid, box, c->kernel, query_arith(c), c->max_bounces,
                                                primary ? nullptr : static_cast<const float4*>(d_in), primary ? query_camera(c) : rt::QueryCamera{},
                                                primary ? static_cast<const uint64_t*>(d_in) : nullptr, n, d_mask, out, c->d_query_shade_counters, stream);
    if (e != hipSuccess) return fail_hip(c, e, "shaded query launch");
    RT_HIP(c, hipEventRecord(c->ev_query_shade[1], stream));
    c->query_shade_made = true;
    return RT_OK;
}

// What shade_from_host stages per element, at most: the input (a 32-byte ray or an 8-byte work-item), the mask, rgba, t, index; each
// array but the last is padded to 16 bytes once.
constexpr size_t kShadeStageBytesPerElement = sizeof(rt_ray) + 4 + 16 + 4 + 4;
constexpr size_t kShadeStagePadding = 4 * 16;
int check_shade_count(rt_context* c, uint64_t n) {
    if (n > ((std::numeric_limits<size_t>::max)() - kShadeStagePadding) / kShadeStageBytesPerElement)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "too many elements: the staged records would not fit an address");
    return RT_OK;
}

// The host forms: input, mask and the requested outputs staged in the context's patch buffer on the context's stream; synchronous.
int shade_from_host(rt_context* c, bool primary, const void* in, size_t in_bytes, uint64_t n, const int32_t* mask, const rt_shade_t& out) {
    RT_DEVICE(c);
    const size_t count = (size_t)n;
    const size_t off_mask = align16(in_bytes * count);
    const size_t off_rgba = off_mask + align16(sizeof(int32_t) * count);
    const size_t off_t = off_rgba + 16 * count;
    const size_t off_index = off_t + align16(sizeof(float) * count);
    if (const int rc = ensure_patch_stage(c, off_index + align16(sizeof(int32_t) * count))) return rc;
    char* const stage = static_cast<char*>(c->d_patch_stage.p);
    rt::QueryShade d = {};
    d.rgba = out.rgba ? reinterpret_cast<float4*>(stage + off_rgba) : nullptr;
    d.t = out.t ? reinterpret_cast<float*>(stage + off_t) : nullptr;
    d.index = out.index ? reinterpret_cast<int32_t*>(stage + off_index) : nullptr;
    int32_t* const d_mask = mask ? reinterpret_cast<int32_t*>(stage + off_mask) : nullptr;
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(stage, in, in_bytes * count, hipMemcpyHostToDevice, stream));
    if (mask) RT_HIP(c, hipMemcpyAsync(d_mask, mask, sizeof(int32_t) * count, hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_shade(c, primary, stage, n, d_mask, d, stream)) return rc;
    if (out.rgba) RT_HIP(c, hipMemcpyAsync(out.rgba, d.rgba, 16 * count, hipMemcpyDeviceToHost, stream));
    if (out.t) RT_HIP(c, hipMemcpyAsync(out.t, d.t, sizeof(float) * count, hipMemcpyDeviceToHost, stream));
    if (out.index) RT_HIP(c, hipMemcpyAsync(out.index, d.index, sizeof(int32_t) * count, hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    return RT_OK;
}

}  // namespace
}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_query_closest_device(rt_context* c, const void* d_rays, uint64_t n, float* d_t, int32_t* d_index, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, d_rays, n, true)) return rc;
    if (!d_t && !d_index) return fail(c, RT_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    if ((reinterpret_cast<uintptr_t>(d_t) | reinterpret_cast<uintptr_t>(d_index)) & 3u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "the outputs must be 4-byte aligned");
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    return enqueue_query(c, Kind::Closest, d_rays, n, d_t, d_index, nullptr, static_cast<hipStream_t>(hip_stream));
}

int rt_query_occluded_device(rt_context* c, const void* d_rays, uint64_t n, uint8_t* d_occluded, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, d_rays, n, true)) return rc;
    if (!d_occluded) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output is NULL");
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    return enqueue_query(c, Kind::Occluded, d_rays, n, nullptr, nullptr, d_occluded, static_cast<hipStream_t>(hip_stream));
}

int rt_query_closest(rt_context* c, const void* rays, uint64_t n, float* t, int32_t* index) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, rays, n, false)) return rc;
    if (!t && !index) return fail(c, RT_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    return query_from_host(c, Kind::Closest, rays, sizeof(rt_ray), n, t, index, nullptr);
}

int rt_query_occluded(rt_context* c, const void* rays, uint64_t n, uint8_t* occluded) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, rays, n, false)) return rc;
    if (!occluded) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output is NULL");
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    return query_from_host(c, Kind::Occluded, rays, sizeof(rt_ray), n, nullptr, nullptr, occluded);
}

int rt_query_primary(rt_context* c, const uint64_t* work_items, uint64_t n, float* t, int32_t* index) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (n != 0 && !work_items) return fail(c, RT_ERR_INVALID_ARGUMENT, "the work-item array is NULL with a non-zero count");
    if (n > (std::numeric_limits<uint64_t>::max)() / sizeof(rt_ray)) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many work-items");
    if (!t && !index) return fail(c, RT_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    for (uint64_t k = 0; k < n; ++k)
        if (work_items[k] >= c->n_rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "a work-item is not below the context's ray count");
    if (const int rc = refuse_triangles(c)) return rc;
    if (!c->pinhole && !c->have_rays)
        return fail(c, RT_ERR_STATE, "no primary rays: rt_create got rays == NULL and rt_set_camera was not called");
    if (n == 0) return RT_OK;
    return query_from_host(c, Kind::Primary, work_items, sizeof(uint64_t), n, t, index, nullptr);
}

int rt_query_hits_device(rt_context* c, const void* d_rays, uint64_t n, const int32_t* d_mask, const rt_hits_t* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, d_rays, n, true)) return rc;
    if (reinterpret_cast<uintptr_t>(d_mask) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the mask must be 4-byte aligned");
    if (const int rc = check_hits(c, d_out, true)) return rc;
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    return enqueue_hits(c, false, d_rays, n, d_mask, device_hits(*d_out), static_cast<hipStream_t>(hip_stream));
}

int rt_query_hits(rt_context* c, const void* rays, uint64_t n, const int32_t* mask, const rt_hits_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, rays, n, false)) return rc;
    if (const int rc = check_hits_count(c, n)) return rc;
    if (const int rc = check_hits(c, out, false)) return rc;
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    return hits_from_host(c, false, rays, sizeof(rt_ray), n, mask, *out);
}

int rt_query_primary_hits(rt_context* c, const uint64_t* work_items, uint64_t n, const rt_hits_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (n != 0 && !work_items) return fail(c, RT_ERR_INVALID_ARGUMENT, "the work-item array is NULL with a non-zero count");
    if (const int rc = check_hits_count(c, n)) return rc;
    if (const int rc = check_hits(c, out, false)) return rc;
    for (uint64_t k = 0; k < n; ++k)
        if (work_items[k] >= c->n_rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "a work-item is not below the context's ray count");
    if (const int rc = refuse_triangles(c)) return rc;
    if (!c->pinhole && !c->have_rays)
        return fail(c, RT_ERR_STATE, "no primary rays: rt_create got rays == NULL and rt_set_camera was not called");
    if (n == 0) return RT_OK;
    return hits_from_host(c, true, work_items, sizeof(uint64_t), n, nullptr, *out);
}

int rt_query_shade_device(rt_context* c, const void* d_rays, uint64_t n, const int32_t* d_mask, const rt_shade_t* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, d_rays, n, true)) return rc;
    if (reinterpret_cast<uintptr_t>(d_mask) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the mask must be 4-byte aligned");
    if (const int rc = check_shade(c, d_out, true)) return rc;
    if (const int rc = refuse_shade_context(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    return enqueue_shade(c, false, d_rays, n, d_mask, rt::QueryShade{reinterpret_cast<float4*>(d_out->rgba), d_out->t, d_out->index},
                         static_cast<hipStream_t>(hip_stream));
}

int rt_query_shade(rt_context* c, const void* rays, uint64_t n, const int32_t* mask, const rt_shade_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_query_rays(c, rays, n, false)) return rc;
    if (const int rc = check_shade_count(c, n)) return rc;
    if (const int rc = check_shade(c, out, false)) return rc;
    if (const int rc = refuse_shade_context(c)) return rc;
    if (n == 0) return RT_OK;
    return shade_from_host(c, false, rays, sizeof(rt_ray), n, mask, *out);
}

int rt_query_primary_shade(rt_context* c, const uint64_t* work_items, uint64_t n, const rt_shade_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (n != 0 && !work_items) return fail(c, RT_ERR_INVALID_ARGUMENT, "the work-item array is NULL with a non-zero count");
    if (const int rc = check_shade_count(c, n)) return rc;
    if (const int rc = check_shade(c, out, false)) return rc;
    for (uint64_t k = 0; k < n; ++k)
        if (work_items[k] >= c->n_rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "a work-item is not below the context's ray count");
    if (const int rc = refuse_shade_context(c)) return rc;
    if (!c->pinhole && !c->have_rays)
        return fail(c, RT_ERR_STATE, "no primary rays: rt_create got rays == NULL and rt_set_camera was not called");
    if (n == 0) return RT_OK;
    return shade_from_host(c, true, work_items, sizeof(uint64_t), n, nullptr, *out);
}

int rt_get_query_shade_info(rt_context* c, rt_query_shade_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->query_shade_made) return fail(c, RT_ERR_STATE, "rt_get_query_shade_info: no shaded query has been made on this context");
    RT_DEVICE(c);
    RT_HIP(c, hipEventSynchronize(c->ev_query_shade[1]));  // the last shaded query's stream, up to the query
    rt::QueryShadeCounters ctr = {};
    RT_HIP(c, hipMemcpy(&ctr, c->d_query_shade_counters, sizeof(ctr), hipMemcpyDeviceToHost));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev_query_shade[0], c->ev_query_shade[1]));
    info->n_rays = ctr.q.n_rays;
    info->n_grid = ctr.q.n_grid;
    info->n_brute = ctr.q.n_brute;
    info->n_literal = ctr.n_literal;
    info->hit_rays = ctr.hits;
    info->rays_traced = ctr.traced;
    info->rays_reference = ctr.reference;
    info->object_tests = ctr.q.tests;
    info->device_ms = (double)ms;
    return RT_OK;
}

int rt_get_query_info(rt_context* c, rt_query_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->query_made) return fail(c, RT_ERR_STATE, "rt_get_query_info: no query has been made on this context");
    RT_DEVICE(c);
    RT_HIP(c, hipEventSynchronize(c->ev_query[1]));  // the last query's stream, up to the query
    rt::QueryCounters ctr = {};
    RT_HIP(c, hipMemcpy(&ctr, c->d_query_counters, sizeof(ctr), hipMemcpyDeviceToHost));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev_query[0], c->ev_query[1]));
    info->n_rays = ctr.n_rays;
    info->n_grid = ctr.n_grid;
    info->n_brute = ctr.n_brute;
    info->object_tests = ctr.tests;
    info->device_ms = (double)ms;
    return RT_OK;
}

}  // extern "C"
