// rt_query_host.cpp - ray queries (hip_raytracer.h): rt_query_closest_device, rt_query_occluded_device, their host twins
// rt_query_closest / rt_query_occluded, rt_query_primary, the hit-record queries rt_query_hits_device / rt_query_hits /
// rt_query_primary_hits, the shaded queries rt_query_shade_device / rt_query_shade / rt_query_primary_shade with their own
// rt_get_query_shade_info, and rt_get_query_info; and the ambient-occlusion pass on items of the caller's, rt_ao_device / rt_ao with
// rt_get_ao_info, and the filter of its counts, rt_ao_filter_device / rt_ao_filter with rt_get_ao_filter_info (the frame forms of both are
// rt_render.cpp's). A query reads the context's object records and grid as
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

// What the three primary forms refuse of (work_items, n) and of the context, in their order: the array, then `arguments()` - the
// form's own count bound and outputs -, the range of every work-item, `refuse_context`, and a context without primary rays (which
// comes before the n == 0 return). Nothing is touched.
template <class Arguments>
int check_primary(rt_context* c, const uint64_t* work_items, uint64_t n, Arguments arguments, int (*refuse_context)(rt_context*)) {
    if (n != 0 && !work_items) return fail(c, RT_ERR_INVALID_ARGUMENT, "the work-item array is NULL with a non-zero count");
    if (const int rc = arguments()) return rc;
    for (uint64_t k = 0; k < n; ++k)
        if (work_items[k] >= c->n_rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "a work-item is not below the context's ray count");
    if (const int rc = refuse_context(c)) return rc;
    return refuse_no_primary_rays(c);
}

// what every query launch reads of the context
struct QueryInputs {
    rt::Scene scene;
    rt::QueryBox box;
    rt::GridDesc grid;
    int arith;
    explicit QueryInputs(const rt_context* c)
        : scene(query_scene(c)), box(query_box(c)), grid(box.grid ? c->grid : rt::GridDesc{}), arith(query_arith(c)) {}
};

// ---- staging in the patch buffer -----------------------------------------------------------------------------------------------------
// A host form stages its arrays behind one another in the context's patch buffer (rt_object_patch.cpp). One row per array, in that
// order: its bytes per element and whether the array is padded to 16 bytes. Row 0 is the input at its largest, a 32-byte ray (an
// 8-byte work-item for the primary forms); then, where the family has one, the mask; then the outputs in the order they are copied back.
struct StageField { size_t elem; bool padded; };
enum { qIn, qT, qIndex, qOccluded };
constexpr StageField kQueryStage[] = {{sizeof(rt_ray), true}, {sizeof(float), true}, {sizeof(int32_t), true}, {1, true}};
enum { hIn, hMask, hT, hIndex, hPoint, hNormal, hReflected };
constexpr StageField kHitsStage[] = {{sizeof(rt_ray), true}, {sizeof(int32_t), true}, {sizeof(float), true}, {sizeof(int32_t), true},
                                     {16, false},            {16, false},             {sizeof(rt_ray), false}};
enum { sIn, sMask, sRgba, sT, sIndex };
constexpr StageField kShadeStage[] = {{sizeof(rt_ray), true}, {sizeof(int32_t), true}, {16, false}, {sizeof(float), true}, {sizeof(int32_t), true}};

size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// The count bound of a table: what it stages per element, at most, and what its padded arrays add, at most, must fit an address.
template <size_t N>
constexpr size_t stage_max_count(const StageField (&fields)[N]) {
    size_t per_element = 0, padding = 0;
    for (const StageField& f : fields) {
        per_element += f.elem;
        padding += f.padded ? 16 : 0;
    }
    return ((std::numeric_limits<size_t>::max)() - padding) / per_element;
}
static_assert(stage_max_count(kHitsStage) == ((std::numeric_limits<size_t>::max)() - 64) / 108, "rt_query_hits' bound: 108 bytes, four pads");
static_assert(stage_max_count(kShadeStage) == ((std::numeric_limits<size_t>::max)() - 64) / 60, "rt_query_shade's bound: 60 bytes, four pads");

template <size_t N>
int check_stage_count(rt_context* c, const StageField (&fields)[N], uint64_t n) {
    if (n > stage_max_count(fields)) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many elements: the staged records would not fit an address");
    return RT_OK;
}

// The layout of one call: n elements per row, `in_bytes` per element of the input.
template <size_t N>
struct Stage {
    const StageField (&fields)[N];
    const size_t in_bytes, n;
    size_t off[N];
    size_t total = 0;
    char* base = nullptr;
    CopyBack back;
    Stage(const StageField (&f)[N], size_t in_bytes_, uint64_t n_) : fields(f), in_bytes(in_bytes_), n((size_t)n_) {
        for (size_t k = 0; k < N; ++k) {
            off[k] = total;
            total += fields[k].padded ? align16(bytes(k)) : bytes(k);
        }
    }
    size_t bytes(size_t k) const { return (k ? fields[k].elem : in_bytes) * n; }
    int bind(rt_context* c) {  // the patch buffer holds the layout
        if (const int rc = ensure_patch_stage(c, total)) return rc;
        base = static_cast<char*>(c->d_patch_stage.p);
        return RT_OK;
    }
    template <class T>
    T* at(size_t k) const { return reinterpret_cast<T*>(base + off[k]); }
    // row k as the device array of the output `host` (null: not wanted), to be copied back
    template <class T>
    T* out(size_t k, void* host) { return back.select<T>(host, base + off[k], bytes(k)); }
};

enum class Kind { Closest, Occluded, Primary };

// One query on `stream` (enqueue_counted). All pointers are device memory; `d_in` the rays or, for Kind::Primary, the work-items.
int enqueue_query(rt_context* c, Kind kind, const void* d_in, uint64_t n, float* d_t, int32_t* d_index, uint8_t* d_occluded, hipStream_t stream) {
    return enqueue_counted(c, c->query, stream, "query launch", [&] {
        const QueryInputs q(c);
        rt::QueryCounters* const counters = static_cast<rt::QueryCounters*>(c->query.d_counters);
        if (kind == Kind::Closest)
            return rt::launch_query_closest(q.scene, q.grid, q.box, q.arith, static_cast<const float4*>(d_in), n, d_t, d_index, counters, stream);
        if (kind == Kind::Occluded)
            return rt::launch_query_occluded(q.scene, q.grid, q.box, q.arith, static_cast<const float4*>(d_in), n, d_occluded, counters, stream);
        return rt::launch_query_primary(q.scene, q.grid, q.box, q.arith, query_camera(c), static_cast<const uint64_t*>(d_in), n, d_t, d_index, counters, stream);
    });
}

// The host twins and rt_query_primary: input and results staged on the context's stream; synchronous. `in_bytes` bytes of input per element.
int query_from_host(rt_context* c, Kind kind, const void* in, size_t in_bytes, uint64_t n, float* t, int32_t* index, uint8_t* occluded) {
    RT_DEVICE(c);
    Stage st(kQueryStage, in_bytes, n);
    if (const int rc = st.bind(c)) return rc;
    float* const d_t = st.out<float>(qT, t);
    int32_t* const d_index = st.out<int32_t>(qIndex, index);
    uint8_t* const d_occ = st.out<uint8_t>(qOccluded, occluded);
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(st.base, in, st.bytes(qIn), hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_query(c, kind, st.base, n, d_t, d_index, d_occ, stream)) return rc;
    return st.back.finish(c, stream);
}

// ---- hit records ---------------------------------------------------------------------------------------------------------------------
// One hit-record query on `stream`, as enqueue_query: `d_in` the rays or, with `primary`, the work-items; `hits` device pointers.
int enqueue_hits(rt_context* c, bool primary, const void* d_in, uint64_t n, const int32_t* d_mask, const rt::QueryHits& hits, hipStream_t stream) {
    return enqueue_counted(c, c->query, stream, "hit-record query launch", [&] {
        const QueryInputs q(c);
        rt::QueryCounters* const counters = static_cast<rt::QueryCounters*>(c->query.d_counters);
        return primary ? rt::launch_query_primary_hits(q.scene, q.grid, q.box, q.arith, query_camera(c), static_cast<const uint64_t*>(d_in), n, hits,
                                                       counters, stream)
                       : rt::launch_query_hits(q.scene, q.grid, q.box, q.arith, static_cast<const float4*>(d_in), n, d_mask, hits, counters, stream);
    });
}

rt::QueryHits device_hits(const rt_hits_t& o) {
    return rt::QueryHits{o.t, o.index, reinterpret_cast<float4*>(o.point), reinterpret_cast<float4*>(o.normal), static_cast<float4*>(o.reflected)};
}

int check_hits(rt_context* c, const rt_hits_t* o, bool device) {
    const rt_hits_t m = o ? *o : rt_hits_t{};
    return check_outputs(c, o, {{m.t, 4}, {m.index, 4}, {m.point, 16}, {m.normal, 16}, {m.reflected, 16}}, device,
                         "t and index must be 4-byte aligned", "point, normal and reflected must be 16-byte aligned");
}

// The host forms: input, mask and the wanted records staged on the context's stream; synchronous.
int hits_from_host(rt_context* c, bool primary, const void* in, size_t in_bytes, uint64_t n, const int32_t* mask, const rt_hits_t& out) {
    RT_DEVICE(c);
    Stage st(kHitsStage, in_bytes, n);
    if (const int rc = st.bind(c)) return rc;
    const rt::QueryHits d{st.out<float>(hT, out.t), st.out<int32_t>(hIndex, out.index), st.out<float4>(hPoint, out.point),
                          st.out<float4>(hNormal, out.normal), st.out<float4>(hReflected, out.reflected)};
    int32_t* const d_mask = mask ? st.at<int32_t>(hMask) : nullptr;
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(st.base, in, st.bytes(hIn), hipMemcpyHostToDevice, stream));
    if (mask) RT_HIP(c, hipMemcpyAsync(d_mask, mask, st.bytes(hMask), hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_hits(c, primary, st.base, n, d_mask, d, stream)) return rc;
    return st.back.finish(c, stream);
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
    const rt_shade_t m = o ? *o : rt_shade_t{};
    return check_outputs(c, o, {{m.rgba, 16}, {m.t, 4}, {m.index, 4}}, device, "t and index must be 4-byte aligned", "rgba must be 16-byte aligned");
}

// One shaded query on `stream`, as enqueue_hits: `d_in` the rays or, with `primary`, the work-items; `out` device pointers.
int enqueue_shade(rt_context* c, bool primary, const void* d_in, uint64_t n, const int32_t* d_mask, const rt::QueryShade& out, hipStream_t stream) {
    return enqueue_counted(c, c->query_shade, stream, "shaded query launch", [&] {
        QueryInputs q(c);
        q.scene.literal = shade_context_literal(c) ? 1u : 0u;
        q.scene.fast_phong = (c->flags & RT_FLAG_FAST_PHONG) ? 1u : 0u;
        return rt::launch_query_shade(q.scene, q.grid, q.box, c->kernel, q.arith, c->max_bounces, primary ? nullptr : static_cast<const float4*>(d_in),
                                      primary ? query_camera(c) : rt::QueryCamera{}, primary ? static_cast<const uint64_t*>(d_in) : nullptr, n, d_mask,
                                      out, static_cast<rt::QueryShadeCounters*>(c->query_shade.d_counters), stream);
    });
}

// The host forms, as hits_from_host.
int shade_from_host(rt_context* c, bool primary, const void* in, size_t in_bytes, uint64_t n, const int32_t* mask, const rt_shade_t& out) {
    RT_DEVICE(c);
    Stage st(kShadeStage, in_bytes, n);
    if (const int rc = st.bind(c)) return rc;
    const rt::QueryShade d{st.out<float4>(sRgba, out.rgba), st.out<float>(sT, out.t), st.out<int32_t>(sIndex, out.index)};
    int32_t* const d_mask = mask ? st.at<int32_t>(sMask) : nullptr;
    hipStream_t stream = c->stream;
    RT_HIP(c, hipMemcpyAsync(st.base, in, st.bytes(sIn), hipMemcpyHostToDevice, stream));
    if (mask) RT_HIP(c, hipMemcpyAsync(d_mask, mask, st.bytes(sMask), hipMemcpyHostToDevice, stream));
    if (const int rc = enqueue_shade(c, primary, st.base, n, d_mask, d, stream)) return rc;
    return st.back.finish(c, stream);
}

}  // namespace

// ---- what the families share, the G-buffer pass (rt_render.cpp) among them; declared in rt_context.h ----------------------------------
int ensure_counted(rt_context* c, CountedSlot& s) {
    if (!s.d_counters) RT_HIP(c, hipMalloc(&s.d_counters, s.counter_bytes));
    for (hipEvent_t& e : s.ev)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    return RT_OK;
}

int read_counted(rt_context* c, const CountedSlot& s, void* counters, double* ms) {
    RT_HIP(c, hipEventSynchronize(s.ev[1]));  // the last call's stream, up to its kernel
    RT_HIP(c, hipMemcpy(counters, s.d_counters, s.counter_bytes, hipMemcpyDeviceToHost));
    float elapsed = 0.f;
    RT_HIP(c, hipEventElapsedTime(&elapsed, s.ev[0], s.ev[1]));
    *ms = (double)elapsed;
    return RT_OK;
}

int check_outputs(rt_context* c, const void* o, std::initializer_list<OutputMember> members, bool device, const char* scalars_misaligned,
                  const char* vectors_misaligned) {
    if (!o) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output struct is NULL");
    uintptr_t any = 0, scalars = 0, vectors = 0;
    for (const OutputMember& m : members) {
        any |= reinterpret_cast<uintptr_t>(m.p);
        (m.align == 4 ? scalars : vectors) |= reinterpret_cast<uintptr_t>(m.p);
    }
    if (!any) return fail(c, RT_ERR_INVALID_ARGUMENT, "all outputs are NULL");
    if (!device) return RT_OK;
    if (scalars & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, scalars_misaligned);
    if (vectors & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, vectors_misaligned);
    return RT_OK;
}

// ---- ambient occlusion (hip_raytracer.h, "ambient-occlusion frames"; the frame form is rt_render.cpp's) ---------------------------------
int check_ao(rt_context* c, const rt_ao_params_t* p, const rt_ao_t* o, bool device) {
    if (!p) return fail(c, RT_ERR_INVALID_ARGUMENT, "the parameter struct is NULL");
    if (!o) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output struct is NULL");
    if (!o->unoccluded && !o->ao) return fail(c, RT_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    if (p->samples == 0 || p->samples > 64 || (p->samples & (p->samples - 1u)))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "samples is one of 1, 2, 4, 8, 16, 32, 64");
    if (p->n_sets < 1 || p->n_sets > 4096) return fail(c, RT_ERR_INVALID_ARGUMENT, "n_sets is 1 .. 4096");
    if (!(p->bias >= 0.f) || !std::isfinite(p->bias)) return fail(c, RT_ERR_INVALID_ARGUMENT, "bias must be finite and not negative");
    if (p->reserved != 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "reserved must be 0");
    if (!p->dirs) return fail(c, RT_ERR_INVALID_ARGUMENT, "the direction table is NULL");
    if (!device) return RT_OK;
    if (reinterpret_cast<uintptr_t>(p->dirs) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the direction table must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(o->ao) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "ao must be 4-byte aligned");
    return RT_OK;
}

int refuse_ao_context(rt_context* c) {
    if (c->has_triangles)
        return fail(c, RT_ERR_STATE, "ambient occlusion on a context with triangle records: its rays are occlusion queries, and the ordered "
                                     "loop over the pair stream does not know type 2");
    return RT_OK;
}

int enqueue_ao(rt_context* c, const rt::GBufferShard& shard, const float* d_point, const float* d_normal, const int32_t* d_index,
               const rt_ao_params_t& p, const rt_ao_t& d_out, hipStream_t stream) {
    const int rc = enqueue_counted(c, c->ao, stream, "ambient-occlusion launch", [&] {
        const QueryInputs q(c);
        const rt::AoInputs in{reinterpret_cast<const float4*>(d_point), reinterpret_cast<const float4*>(d_normal), d_index,
                              static_cast<const float4*>(p.dirs),      p.samples, p.n_sets, p.bias, 1.0f / (float)p.samples};
        return rt::launch_ao(q.scene, q.grid, q.box, q.arith, shard, in, rt::AoOutputs{d_out.unoccluded, d_out.ao},
                             static_cast<rt::AoCounters*>(c->ao.d_counters), stream);
    });
    if (rc) return rc;
    c->ao_items = shard.n_local;
    return RT_OK;
}

int stage_ao_host(rt_context* c, const rt_ao_params_t& p, const rt_ao_t& out, uint64_t n, size_t extra, hipStream_t stream,
                  rt_ao_params_t& d_p, rt_ao_t& d_out, CopyBack& back, char*& d_extra) {
    const size_t dirs_bytes = (size_t)p.n_sets * p.samples * 16u;
    const size_t off_unoccluded = dirs_bytes, off_ao = off_unoccluded + align16((size_t)n), off_extra = off_ao + align16((size_t)n * sizeof(float));
    if (const int rc = ensure_patch_stage(c, off_extra + extra)) return rc;
    char* const base = static_cast<char*>(c->d_patch_stage.p);
    RT_HIP(c, hipMemcpyAsync(base, p.dirs, dirs_bytes, hipMemcpyHostToDevice, stream));
    d_p = p;
    d_p.dirs = base;
    d_out.unoccluded = back.select<uint8_t>(out.unoccluded, base + off_unoccluded, (size_t)n);
    d_out.ao = back.select<float>(out.ao, base + off_ao, (size_t)n * sizeof(float));
    d_extra = base + off_extra;
    return RT_OK;
}

namespace {

// what rt_ao_device and rt_ao refuse of (point, normal, index, n); nothing is touched
int check_ao_items(rt_context* c, const float* point, const float* normal, const int32_t* index, uint64_t n, bool device) {
    if (n != 0 && (!point || !normal)) return fail(c, RT_ERR_INVALID_ARGUMENT, "point or normal is NULL with a non-zero count");
    if (n > (std::numeric_limits<size_t>::max)() / 64u) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many items");
    if (!device) return RT_OK;
    if ((reinterpret_cast<uintptr_t>(point) | reinterpret_cast<uintptr_t>(normal)) & 15u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "point and normal must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(index) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "index must be 4-byte aligned");
    return RT_OK;
}

}  // namespace

// ---- filtered ambient occlusion (hip_raytracer.h, "filtered ambient occlusion"; the frame forms are rt_render.cpp's) ------------------
int check_ao_filter(rt_context* c, const rt_ao_filter_params_t* f, const rt_ao_filtered_t* o, uint32_t samples, bool device) {
    if (!f) return fail(c, RT_ERR_INVALID_ARGUMENT, "the filter's parameter struct is NULL");
    if (!o) return fail(c, RT_ERR_INVALID_ARGUMENT, "the output struct is NULL");
    if (!o->ao && !o->grey && !o->taps) return fail(c, RT_ERR_INVALID_ARGUMENT, "all outputs are NULL");
    if (f->radius < 1 || f->radius > 4) return fail(c, RT_ERR_INVALID_ARGUMENT, "radius is 1 .. 4");
    if (!(f->plane_max >= 0.f) || !std::isfinite(f->plane_max)) return fail(c, RT_ERR_INVALID_ARGUMENT, "plane_max must be finite and not negative");
    if (f->reserved != 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "reserved must be 0");
    if (samples == 0 || samples > 64 || (samples & (samples - 1u))) return fail(c, RT_ERR_INVALID_ARGUMENT, "samples is one of 1, 2, 4, 8, 16, 32, 64");
    if (device && (reinterpret_cast<uintptr_t>(o->ao) & 3u)) return fail(c, RT_ERR_INVALID_ARGUMENT, "ao must be 4-byte aligned");
    return RT_OK;
}

int enqueue_ao_filter(rt_context* c, const uint8_t* d_unoccluded, const float* d_point, const float* d_normal, const int32_t* d_index,
                      uint64_t width, uint64_t rows, uint32_t samples, const rt_ao_filter_params_t& f, const rt_ao_filtered_t& d_out,
                      hipStream_t stream) {
    const int rc = enqueue_counted(c, c->ao_filter, stream, "ambient-occlusion filter launch", [&] {
        const rt::AoFilterInputs in{d_unoccluded, reinterpret_cast<const float4*>(d_point), reinterpret_cast<const float4*>(d_normal), d_index,
                                    width,        rows, samples, f.radius, f.normal_min, f.plane_max};
        return rt::launch_ao_filter(in, rt::AoFilterOutputs{d_out.ao, d_out.grey, d_out.taps},
                                    static_cast<rt::AoFilterCounters*>(c->ao_filter.d_counters), stream);
    });
    if (rc) return rc;
    c->ao_filter_items = width * rows;
    return RT_OK;
}

size_t ao_filter_output_bytes(uint64_t n) { return align16((size_t)n * sizeof(float)) + 2 * align16((size_t)n); }

size_t stage_ao_filter_outputs(char* base, size_t offset, const rt_ao_filtered_t& out, uint64_t n, rt_ao_filtered_t& d_out, CopyBack& back) {
    const size_t off_grey = offset + align16((size_t)n * sizeof(float)), off_taps = off_grey + align16((size_t)n);
    d_out.ao = back.select<float>(out.ao, base + offset, (size_t)n * sizeof(float));
    d_out.grey = back.select<uint8_t>(out.grey, base + off_grey, (size_t)n);
    d_out.taps = back.select<uint8_t>(out.taps, base + off_taps, (size_t)n);
    return off_taps + align16((size_t)n);
}

namespace {

// what rt_ao_filter_device and rt_ao_filter refuse of (unoccluded, point, normal, index, width, rows); nothing is touched
int check_ao_filter_items(rt_context* c, const uint8_t* unoccluded, const float* point, const float* normal, const int32_t* index, uint64_t width,
                          uint64_t rows, bool device) {
    if (width != 0 && rows > ((std::numeric_limits<size_t>::max)() / 64u) / width) return fail(c, RT_ERR_INVALID_ARGUMENT, "width * rows overflows");
    if (width * rows != 0 && (!unoccluded || !point || !normal))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "unoccluded, point or normal is NULL with a non-zero count");
    if (!device) return RT_OK;
    if ((reinterpret_cast<uintptr_t>(point) | reinterpret_cast<uintptr_t>(normal)) & 15u)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "point and normal must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(index) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "index must be 4-byte aligned");
    return RT_OK;
}

}  // namespace

int refuse_no_primary_rays(rt_context* c) {
    if (!c->pinhole && !c->have_rays)
        return fail(c, RT_ERR_STATE, "no primary rays: rt_create got rays == NULL and rt_set_camera was not called");
    return RT_OK;
}

int CopyBack::finish(rt_context* c, hipStream_t stream) const {
    for (int k = 0; k < count; ++k) RT_HIP(c, hipMemcpyAsync(items[k].host, items[k].dev, items[k].bytes, hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    return RT_OK;
}

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
    const auto arguments = [&] {
        if (n > (std::numeric_limits<uint64_t>::max)() / sizeof(rt_ray)) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many work-items");
        if (!t && !index) return fail(c, RT_ERR_INVALID_ARGUMENT, "both outputs are NULL");
        return (int)RT_OK;
    };
    if (const int rc = check_primary(c, work_items, n, arguments, refuse_triangles)) return rc;
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
    if (const int rc = check_stage_count(c, kHitsStage, n)) return rc;
    if (const int rc = check_hits(c, out, false)) return rc;
    if (const int rc = refuse_triangles(c)) return rc;
    if (n == 0) return RT_OK;
    return hits_from_host(c, false, rays, sizeof(rt_ray), n, mask, *out);
}

int rt_query_primary_hits(rt_context* c, const uint64_t* work_items, uint64_t n, const rt_hits_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const auto arguments = [&] {
        const int rc = check_stage_count(c, kHitsStage, n);
        return rc ? rc : check_hits(c, out, false);
    };
    if (const int rc = check_primary(c, work_items, n, arguments, refuse_triangles)) return rc;
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
    if (const int rc = check_stage_count(c, kShadeStage, n)) return rc;
    if (const int rc = check_shade(c, out, false)) return rc;
    if (const int rc = refuse_shade_context(c)) return rc;
    if (n == 0) return RT_OK;
    return shade_from_host(c, false, rays, sizeof(rt_ray), n, mask, *out);
}

int rt_query_primary_shade(rt_context* c, const uint64_t* work_items, uint64_t n, const rt_shade_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const auto arguments = [&] {
        const int rc = check_stage_count(c, kShadeStage, n);
        return rc ? rc : check_shade(c, out, false);
    };
    if (const int rc = check_primary(c, work_items, n, arguments, refuse_shade_context)) return rc;
    if (n == 0) return RT_OK;
    return shade_from_host(c, true, work_items, sizeof(uint64_t), n, nullptr, *out);
}

int rt_get_query_shade_info(rt_context* c, rt_query_shade_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->query_shade.made) return fail(c, RT_ERR_STATE, "rt_get_query_shade_info: no shaded query has been made on this context");
    RT_DEVICE(c);
    rt::QueryShadeCounters ctr = {};
    if (const int rc = read_counted(c, c->query_shade, &ctr, &info->device_ms)) return rc;
    info->n_rays = ctr.q.n_rays;
    info->n_grid = ctr.q.n_grid;
    info->n_brute = ctr.q.n_brute;
    info->n_literal = ctr.n_literal;
    info->hit_rays = ctr.hits;
    info->rays_traced = ctr.traced;
    info->rays_reference = ctr.reference;
    info->object_tests = ctr.q.tests;
    return RT_OK;
}

int rt_ao_device(rt_context* c, const float* d_point, const float* d_normal, const int32_t* d_index, uint64_t n, const rt_ao_params_t* params,
                 const rt_ao_t* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_ao(c, params, d_out, true)) return rc;
    if (const int rc = check_ao_items(c, d_point, d_normal, d_index, n, true)) return rc;
    if (const int rc = refuse_ao_context(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    c->ao_frame = false;
    return enqueue_ao(c, rt::GBufferShard{n, n, 1, 0, 1}, d_point, d_normal, d_index, *params, *d_out, static_cast<hipStream_t>(hip_stream));
}

// the host twin: items, table and results staged in the patch buffer on the context's stream; synchronous
int rt_ao(rt_context* c, const float* point, const float* normal, const int32_t* index, uint64_t n, const rt_ao_params_t* params, const rt_ao_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_ao(c, params, out, false)) return rc;
    if (const int rc = check_ao_items(c, point, normal, index, n, false)) return rc;
    if (const int rc = refuse_ao_context(c)) return rc;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    hipStream_t stream = c->stream;
    const size_t vec_bytes = (size_t)n * 16u, index_bytes = (size_t)n * sizeof(int32_t);
    rt_ao_params_t d_params;
    rt_ao_t d_out;
    CopyBack back;
    char* d_items = nullptr;
    if (const int rc = stage_ao_host(c, *params, *out, n, 2 * vec_bytes + index_bytes, stream, d_params, d_out, back, d_items)) return rc;
    RT_HIP(c, hipMemcpyAsync(d_items, point, vec_bytes, hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipMemcpyAsync(d_items + vec_bytes, normal, vec_bytes, hipMemcpyHostToDevice, stream));
    if (index) RT_HIP(c, hipMemcpyAsync(d_items + 2 * vec_bytes, index, index_bytes, hipMemcpyHostToDevice, stream));
    c->ao_frame = false;
    if (const int rc = enqueue_ao(c, rt::GBufferShard{n, n, 1, 0, 1}, reinterpret_cast<const float*>(d_items),
                                  reinterpret_cast<const float*>(d_items + vec_bytes),
                                  index ? reinterpret_cast<const int32_t*>(d_items + 2 * vec_bytes) : nullptr, d_params, d_out, stream))
        return rc;
    return back.finish(c, stream);
}

int rt_get_ao_info(rt_context* c, rt_ao_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->ao.made) return fail(c, RT_ERR_STATE, "rt_get_ao_info: no ambient-occlusion pass has been made on this context");
    RT_DEVICE(c);
    rt::AoCounters ctr = {};
    if (const int rc = read_counted(c, c->ao, &ctr, &info->ao_ms)) return rc;
    float gbuffer = 0.f;
    if (c->ao_frame) RT_HIP(c, hipEventElapsedTime(&gbuffer, c->ev_ao_gbuffer[0], c->ev_ao_gbuffer[1]));  // (before the kernel: it has ended)
    info->n_items = c->ao_items;
    info->n_live = ctr.n_live;
    info->n_rays = ctr.q.n_rays;
    info->n_grid = ctr.q.n_grid;
    info->n_brute = ctr.q.n_brute;
    info->object_tests = ctr.q.tests;
    info->gbuffer_ms = (double)gbuffer;
    return RT_OK;
}

int rt_ao_filter_device(rt_context* c, const uint8_t* d_unoccluded, const float* d_point, const float* d_normal, const int32_t* d_index,
                        uint64_t width, uint64_t rows, uint32_t samples, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* d_out,
                        void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_ao_filter(c, filter, d_out, samples, true)) return rc;
    if (const int rc = check_ao_filter_items(c, d_unoccluded, d_point, d_normal, d_index, width, rows, true)) return rc;
    if (width * rows == 0) return RT_OK;
    RT_DEVICE(c);
    c->ao_filter_frame = false;
    return enqueue_ao_filter(c, d_unoccluded, d_point, d_normal, d_index, width, rows, samples, *filter, *d_out, static_cast<hipStream_t>(hip_stream));
}

// the host twin: items and results staged in the patch buffer on the context's stream; synchronous
int rt_ao_filter(rt_context* c, const uint8_t* unoccluded, const float* point, const float* normal, const int32_t* index, uint64_t width,
                 uint64_t rows, uint32_t samples, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_ao_filter(c, filter, out, samples, false)) return rc;
    if (const int rc = check_ao_filter_items(c, unoccluded, point, normal, index, width, rows, false)) return rc;
    const uint64_t n = width * rows;
    if (n == 0) return RT_OK;
    RT_DEVICE(c);
    hipStream_t stream = c->stream;
    const size_t vec_bytes = (size_t)n * 16u, index_bytes = (size_t)n * sizeof(int32_t);
    const size_t off_normal = vec_bytes, off_index = 2 * vec_bytes, off_counts = off_index + align16(index_bytes), off_out = off_counts + align16((size_t)n);
    if (const int rc = ensure_patch_stage(c, off_out + ao_filter_output_bytes(n))) return rc;
    char* const base = static_cast<char*>(c->d_patch_stage.p);
    rt_ao_filtered_t d_out;
    CopyBack back;
    stage_ao_filter_outputs(base, off_out, *out, n, d_out, back);
    RT_HIP(c, hipMemcpyAsync(base, point, vec_bytes, hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipMemcpyAsync(base + off_normal, normal, vec_bytes, hipMemcpyHostToDevice, stream));
    if (index) RT_HIP(c, hipMemcpyAsync(base + off_index, index, index_bytes, hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipMemcpyAsync(base + off_counts, unoccluded, (size_t)n, hipMemcpyHostToDevice, stream));
    c->ao_filter_frame = false;
    if (const int rc = enqueue_ao_filter(c, reinterpret_cast<const uint8_t*>(base + off_counts), reinterpret_cast<const float*>(base),
                                         reinterpret_cast<const float*>(base + off_normal),
                                         index ? reinterpret_cast<const int32_t*>(base + off_index) : nullptr, width, rows, samples, *filter, d_out,
                                         stream))
        return rc;
    return back.finish(c, stream);
}

int rt_get_ao_filter_info(rt_context* c, rt_ao_filter_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->ao_filter.made) return fail(c, RT_ERR_STATE, "rt_get_ao_filter_info: no filtered ambient-occlusion pass has been made on this context");
    RT_DEVICE(c);
    rt::AoFilterCounters slots[rt::kAoFilterCounterSlots] = {};
    if (const int rc = read_counted(c, c->ao_filter, slots, &info->filter_ms)) return rc;
    rt::AoFilterCounters ctr = {};
    for (const rt::AoFilterCounters& s : slots) {
        ctr.n_live += s.n_live;
        ctr.accepted += s.accepted;
    }
    float gbuffer = 0.f, ao = 0.f;
    if (c->ao_filter_frame) {  // (this form's own marks, recorded before the filter kernel on its stream: they have ended)
        RT_HIP(c, hipEventElapsedTime(&gbuffer, c->ev_ao_filter_frame[0], c->ev_ao_filter_frame[1]));
        RT_HIP(c, hipEventElapsedTime(&ao, c->ev_ao_filter_frame[1], c->ev_ao_filter_frame[2]));
    }
    info->n_items = c->ao_filter_items;
    info->n_live = ctr.n_live;
    info->accepted = ctr.accepted;
    info->gbuffer_ms = (double)gbuffer;
    info->ao_ms = (double)ao;
    return RT_OK;
}

int rt_get_query_info(rt_context* c, rt_query_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->query.made) return fail(c, RT_ERR_STATE, "rt_get_query_info: no query has been made on this context");
    RT_DEVICE(c);
    rt::QueryCounters ctr = {};
    if (const int rc = read_counted(c, c->query, &ctr, &info->device_ms)) return rc;
    info->n_rays = ctr.n_rays;
    info->n_grid = ctr.n_grid;
    info->n_brute = ctr.n_brute;
    info->object_tests = ctr.tests;
    return RT_OK;
}

}  // extern "C"
