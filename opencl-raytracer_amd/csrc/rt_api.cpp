// rt_api.cpp - the C ABI of include/hip_raytracer.h: context life cycle, scene re-pack + upload, rays / camera / pose,
// the shard and supersampling setters, the tile / grid / light readers, stats and timing. What produces a frame is rt_render.cpp.
//
// Plays the role of the reference's OpenCLRaytracer ctor/Render()/dtor (OpenCLRaytracer.cpp:13-105) for one
// MI355X. There is deliberately no CPU path here: every failure to reach the GPU is an error.
#include "rt_context.h"

namespace rt::host {

static thread_local std::string g_create_error;

int fail(rt_context* ctx, int code, const std::string& msg) {
    if (ctx) ctx->error = msg;
    else g_create_error = msg;
    return code;
}

int fail_hip(rt_context* ctx, hipError_t e, const char* what) {
    return fail(ctx, e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

// a context-owned buffer that only ever grows: device memory, or pinned host memory
int grow_buffer(rt_context* c, void*& p, size_t& have, size_t need, bool pinned_host) {
    if (p && need <= have) return RT_OK;
    if (p) (void)(pinned_host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    have = 0;
    if (pinned_host) RT_HIP(c, hipHostMalloc(&p, need ? need : 16, hipHostMallocDefault));
    else RT_HIP(c, hipMalloc(&p, need ? need : 16));
    have = need;
    return RT_OK;
}

// what rt_set_supersampling, rt_set_camera and rt_set_shard hold a (factor, camera, shard) combination to; nothing is changed here
static int check_supersampling(rt_context* c, uint32_t s, bool pinhole, uint32_t width, uint32_t height, uint64_t tile_rays, uint32_t world) {
    if (s < 1 || s > 4) return fail(c, RT_ERR_INVALID_ARGUMENT, "the supersampling factor is 1, 2, 3 or 4");
    if (s == 1) return RT_OK;
    if (c->kernel == RT_KERNEL_HITTEST)
        return fail(c, RT_ERR_STATE, "an RT_KERNEL_HITTEST context renders the nearest t per ray: a time is not a colour, there is nothing to filter");
    if (c->aux_t || c->aux_index) return fail(c, RT_ERR_STATE, "aux buffers are per work-item: not together with a supersampling factor > 1");
    if (!pinhole || !width || !height)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "supersampling needs a pinhole camera (rt_set_camera, rt_set_pose): the samples are the sub-pixel rays of its grid");
    if (width % s || height % s) return fail(c, RT_ERR_INVALID_ARGUMENT, "width and height of the sample grid must be multiples of the supersampling factor");
    if (world > 1 && tile_rays % ((uint64_t)s * width))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "with supersampling a tile must hold whole pixel rows: tile_rays % (s * width) == 0");
    return RT_OK;
}

// a pinhole grid's directions are (col - W/2, (H - row) - H/2, z): the shortest belongs to the centre pixel, the longest to a corner
static bool camera_in_domain(uint32_t W, uint32_t H, float z) {
    const double zz = (double)z * (double)z;
    const double lo = zz + ((W & 1u) ? 0.25 : 0.0) + ((H & 1u) ? 0.25 : 0.0);
    const double hi = zz + 0.25 * (double)W * (double)W + 0.25 * (double)H * (double)H;
    return std::isfinite(zz) && lo > 1.0e-29 && hi < 1.0e29;  // (a decade inside the walks' window: fp32 rounding of the sum)
}
void apply_ray_domain(rt_context* c) {
    const bool out = c->pinhole ? c->camera_out_of_domain : c->rays_out_of_domain;
    c->flags = c->base_flags | (out ? RT_FLAG_LITERAL : 0u);
}

// ---- posed cameras (hip_raytracer.h) ----
// The ray buffer of a live context written by the generator (rt_raygen.hip) instead of copied into it: the verdict pass stores no
// ray, the refusals follow, and only then the context's own buffer is overwritten. pose_check changes nothing of the context's
// state (it may allocate the scan record); pose_commit cannot be refused any more. rt_set_pose_multi runs the first on every shard
// before the second on any.
static bool pose_trace() { return std::getenv("RT_RAYS_TRACE") != nullptr; }  // (set_rays_from_device's aid, for the two passes here)

int pose_grid(rt_context* c, uint32_t width, uint32_t height, float z, const float* m, const float* origin, rt::PoseGrid& g) {
    if (!m || !origin) return fail(c, RT_ERR_INVALID_ARGUMENT, "the pose's matrix or origin is NULL");
    if (width > 0x1000000u || height > 0x1000000u) return fail(c, RT_ERR_INVALID_ARGUMENT, "grid too large");
    g.width = width;
    g.height = height;
    g.z = z;
    std::memcpy(g.m, m, sizeof(g.m));
    std::memcpy(g.origin, origin, sizeof(g.origin));
    return RT_OK;
}

int pose_check(rt_context* c, const rt::PoseGrid& g, hipStream_t stream, PoseVerdict& v) {
    if (g.width == 0 || g.height == 0 || (uint64_t)g.width * g.height != c->n_rays)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "width*height must equal n_rays");
    if (c->ss > 1) {
        const int rc = check_supersampling(c, c->ss, true, g.width, g.height, c->shard.tile_rays, c->shard.world);
        if (rc) return rc;
    }
    RT_DEVICE(c);
    if (!c->d_scan) RT_HIP(c, hipMalloc((void**)&c->d_scan, sizeof(rt::RayScan)));
    if (!c->h_scan) RT_HIP(c, hipHostMalloc((void**)&c->h_scan, sizeof(rt::RayScan), hipHostMallocDefault));
    const bool trace = pose_trace();
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventPair { hipEvent_t* e; ~EventPair() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    if (trace) { RT_HIP(c, hipEventCreate(&ev[0])); RT_HIP(c, hipEventCreate(&ev[1])); }
    if (trace) RT_HIP(c, hipEventRecord(ev[0], stream));
    const hipError_t e = rt::launch_pose_verdict(g, c->d_scan, stream);
    if (e != hipSuccess) return fail_hip(c, e, "pose verdict launch");
    if (trace) RT_HIP(c, hipEventRecord(ev[1], stream));
    RT_HIP(c, hipMemcpyAsync(c->h_scan, c->d_scan, sizeof(rt::RayScan), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (trace) RT_HIP(c, hipEventElapsedTime(&v.verdict_ms, ev[0], ev[1]));
    v.in_domain = !(c->h_scan->flags & rt::kRayDomain);
    // the starts are one point: the scan's predicate and box on it, in fp32 with every sum rounded (start.w is 1)
    const volatile float s1 = g.origin[0] + g.origin[1];
    const volatile float s2 = s1 + g.origin[2];
    v.starts_ok = std::isfinite((float)s2);
    bool inside = v.starts_ok;
    for (int a = 0; a < 3; ++a) {
        v.origin[a] = v.starts_ok ? (double)g.origin[a] : 0.0;
        inside = inside && v.origin[a] >= c->grid_box_lo[a] && v.origin[a] <= c->grid_box_hi[a];
    }
    v.on_grid = c->grid.enabled && v.starts_ok && inside;
    if (c->has_triangles && (!v.on_grid || !v.in_domain))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "triangle records are traced by the grid path only: this pose needs the literal loops (a direction of |d|^2 outside "
                    "(1e-30, 1e30)) or brute force (an origin that is not finite or lies outside the box the grid was built for)");
    return RT_OK;
}

int pose_commit(rt_context* c, const rt::PoseGrid& g, hipStream_t stream, const PoseVerdict& v) {
    RT_DEVICE(c);
    const bool trace = pose_trace();
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventPair { hipEvent_t* e; ~EventPair() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    if (trace) { RT_HIP(c, hipEventCreate(&ev[0])); RT_HIP(c, hipEventCreate(&ev[1])); }
    if (!c->d_rays) RT_HIP(c, hipMalloc((void**)&c->d_rays, sizeof(rt_ray) * (size_t)c->n_rays));
    if (trace) RT_HIP(c, hipEventRecord(ev[0], stream));
    const hipError_t e = rt::launch_pose_rays(g, c->d_rays, stream);
    if (e != hipSuccess) return fail_hip(c, e, "pose generation launch");
    if (trace) RT_HIP(c, hipEventRecord(ev[1], stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (trace) {
        float gen_ms = 0.f;
        RT_HIP(c, hipEventElapsedTime(&gen_ms, ev[0], ev[1]));
        std::fprintf(stderr, "[rt_set_pose] verdict %.4f ms generate %.4f ms rays %llu\n", (double)v.verdict_ms, (double)gen_ms, (unsigned long long)c->n_rays);
    }
    c->have_rays = true;
    c->pinhole = false;
    c->width = c->height = 0;
    c->z = 0.f;
    c->pose_w = g.width;
    c->pose_h = g.height;
    c->pose = g;
    c->dir_w_zero = true;
    c->primary_w_one = v.starts_ok;
    c->rays_out_of_domain = !v.in_domain;
    c->rays_off_grid = !v.on_grid;
    c->pose_outside = c->grid.enabled && v.starts_ok && !v.on_grid && !c->has_triangles;  // (its table decides: settle_outside_pose)
    c->primary_outside = false;
    for (int a = 0; a < 3; ++a) c->origin_lo[a] = c->origin_hi[a] = v.origin[a];
    apply_ray_domain(c);
    c->rects_dirty = true;
    c->tiles_dirty = true;
    return RT_OK;
}

int check_set_lights(rt_context* c, const void* lights, uint32_t n_lights) {
    if (n_lights && !lights) return fail(c, RT_ERR_INVALID_ARGUMENT, "lights is NULL with a non-zero count");
    if (n_lights >= (1u << 22)) return fail(c, RT_ERR_INVALID_ARGUMENT, "more than 4 194 303 lights");
    return RT_OK;
}

}  // namespace rt::host

using namespace rt::host;

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char* rt_last_error(const rt_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int rt_create(rt_context** out_ctx, const void* objs, uint32_t n_objs, const void* lights, uint32_t n_lights,
              const void* rays, uint64_t n_rays, uint32_t max_bounces, int kernel, int device, uint32_t flags) {
    g_create_error.clear();
    if (!out_ctx) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    *out_ctx = nullptr;
    if (kernel < 0 || kernel > 2) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "kernel must be 0, 1 or 2");
    if ((n_objs && !objs) || (n_lights && !lights))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "objs/lights is NULL with a non-zero count");
    if (flags & ~(RT_FLAG_UNFUSED | RT_FLAG_LITERAL | RT_FLAG_NO_RAYGEN | RT_FLAG_WAVEFRONT | RT_FLAG_MONOLITHIC | RT_FLAG_NO_GRID |
                  RT_FLAG_FAST_PHONG | RT_FLAG_DEVICE_OPENCL))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "unknown flag bits");
    if ((flags & RT_FLAG_DEVICE_OPENCL) && (flags & RT_FLAG_UNFUSED))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "RT_FLAG_DEVICE_OPENCL and RT_FLAG_UNFUSED are exclusive (the device build contracts)");
    if ((flags & RT_FLAG_DEVICE_OPENCL) && (flags & RT_FLAG_FAST_PHONG))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "RT_FLAG_DEVICE_OPENCL and RT_FLAG_FAST_PHONG are exclusive");
    if (flags & RT_FLAG_DEVICE_OPENCL)
        for (uint32_t i = 0; i < n_objs; ++i)
            if (static_cast<const rt_object_data*>(objs)[i].type == 2u)
                return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "RT_FLAG_DEVICE_OPENCL: triangles (type 2) have no reference arithmetic to match");
    if (n_lights >= (1u << 22))  // the large-scene path keeps a pixel's light index in 22 bits of its phase word
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "more than 4 194 303 lights");
    if ((flags & RT_FLAG_WAVEFRONT) && (flags & RT_FLAG_MONOLITHIC))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "RT_FLAG_WAVEFRONT and RT_FLAG_MONOLITHIC are exclusive");

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, "no HIP device available (this backend has no CPU fallback)");
    if (device < 0 || device >= n_dev) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "device ordinal out of range");

    rt_context* c = new (std::nothrow) rt_context();
    if (!c) return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->device = device;
    c->flags = flags;
    c->user_flags = flags;
    c->lights_capacity = n_lights;
    c->kernel = kernel;
    c->n_objs = n_objs;
    c->n_lights = n_lights;
    c->n_rays = n_rays;
    c->shard.n_local = n_rays;
    c->max_bounces = max_bounces;

    StopWatch sw_total, sw;
    int rc = RT_OK;
    auto bail = [&](int code) {
        g_create_error = c->error;
        rt_destroy(c);
        return code;
    };
#define RT_TRY(call)                                      \
    do {                                                  \
        hipError_t e2_ = (call);                          \
        if (e2_ != hipSuccess) { rc = fail_hip(c, e2_, #call); return bail(rc); } \
    } while (0)

    SetupTrace lap("rt_create");  // engineering aid: where rt_create's time goes
    DeviceGuard guard(device);  // restores the caller's current device on every return below
    if (!guard.ok) { rc = fail_hip(c, guard.err, "hipSetDevice"); return bail(rc); }
    RT_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    lap("device + stream");
    // (when rt_create is the process's first HIP call this is where the runtime starts up and the device context is made: ~140 ms
    //  on the test boxes, MEASURED - it stays in create_ms, which is what the caller waits for, but is no part of the upload)
    (void)sw.lap_ms();
    for (uint32_t i = 0; i < kTimingSlots; ++i) {
        RT_TRY(hipEventCreate(&c->ev_begin[i]));
        c->ev_begin_made = i + 1;
        RT_TRY(hipEventCreate(&c->ev_end[i]));
        c->ev_end_made = i + 1;
    }
    RT_TRY(hipMalloc((void**)&c->d_counters, sizeof(rt::Counters)));
    lap("events + counters");

    {
        std::vector<rt::HotPair> pairs;
        std::vector<rt::HotObject> hot;
        std::vector<rt::ColdObject> cold;
        repack_objects(static_cast<const rt_object_data*>(objs), n_objs, pairs, hot, cold);
        c->n_pairs = (uint32_t)pairs.size();
        lap("repack_objects");
        RT_TRY(hipMalloc((void**)&c->d_pairs, sizeof(rt::HotPair) * (pairs.size() + 1)));
        RT_TRY(hipMalloc((void**)&c->d_shadow_pairs, sizeof(rt::HotPair) * (pairs.size() + 1)));
        if (!pairs.empty()) {
            RT_TRY(hipMemcpy(c->d_pairs, pairs.data(), sizeof(rt::HotPair) * pairs.size(), hipMemcpyHostToDevice));
            // shadow stream: same records, objects ordered by decreasing size (stable), re-paired
            const rt_object_data* od = static_cast<const rt_object_data*>(objs);
            std::vector<uint32_t> order(n_objs);
            std::vector<double> size(n_objs);
            for (uint32_t i = 0; i < n_objs; ++i) { order[i] = i; size[i] = size_proxy(od[i]); }
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return size[a] > size[b]; });
            std::vector<rt::HotPair> spairs;
            pack_pairs(od, order.data(), n_objs, spairs);
            c->h_shadow_slot.resize(n_objs);  // (rt_set_transforms patches an object's half of its shadow pair where this order put it)
            for (uint32_t i = 0; i < n_objs; ++i) c->h_shadow_slot[order[i]] = i;
            RT_TRY(hipMemcpy(c->d_shadow_pairs, spairs.data(), sizeof(rt::HotPair) * spairs.size(), hipMemcpyHostToDevice));
        }
        lap("pair streams (sort, upload)");
        // one spare record keeps the arrays non-null for n_objs == 0; without triangles the compact records follow the HotObjects
        // (rt_device.h: compact_table), n_objs + 1 of them as well
        bool any_triangle = false;
        for (uint32_t i = 0; i < n_objs && !any_triangle; ++i) any_triangle = static_cast<const rt_object_data*>(objs)[i].type == 2u;
        static_assert(sizeof(rt::CompactObject) == sizeof(rt::HotObject), "one allocation, two tables of n_objs + 1 records");
        RT_TRY(hipMalloc((void**)&c->d_hot, sizeof(rt::HotObject) * (size_t)(n_objs + 1) * (any_triangle ? 1u : 2u)));
        RT_TRY(hipMalloc((void**)&c->d_cold, sizeof(rt::ColdObject) * (size_t)(n_objs + 1)));
        if (n_objs <= 64) {  // per-bundle culling is only used for scenes this small
            c->h_spheres.resize(4 * (size_t)n_objs);
            for (uint32_t i = 0; i < n_objs; ++i) {
                const Sphere sp = bounding_sphere(static_cast<const rt_object_data*>(objs)[i]);
                c->h_spheres[4 * i] = sp.x; c->h_spheres[4 * i + 1] = sp.y; c->h_spheres[4 * i + 2] = sp.z; c->h_spheres[4 * i + 3] = sp.r;
            }
        }
        RT_TRY(hipMalloc((void**)&c->d_bounds, sizeof(float4) * 65));
        {   // the spare HotObject behind the last one can never be hit (unknown type): records of the unified walk that hold
            // no candidate point at it (GridDesc::walk_none)
            rt::HotObject none{};
            none.type = 0xffffffffu;
            hot.push_back(none);
            RT_TRY(hipMemcpy(c->d_hot, hot.data(), sizeof(rt::HotObject) * (size_t)(n_objs + 1), hipMemcpyHostToDevice));
        }
        if (n_objs) RT_TRY(hipMemcpy(c->d_cold, cold.data(), sizeof(rt::ColdObject) * n_objs, hipMemcpyHostToDevice));
        {   // matrix rows of both directions + absorption side by side (ObjectRecord)
            std::vector<rt::ObjectRecord> rec((size_t)n_objs + 1);
            std::memset(rec.data(), 0, sizeof(rt::ObjectRecord) * rec.size());
            parallel_for(n_objs, 16384, [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; ++i) {
                    rec[i].inv_row[0] = hot[i].row0; rec[i].inv_row[1] = hot[i].row1; rec[i].inv_row[2] = hot[i].row2;
                    rec[i].type = hot[i].type;
                    rec[i].pad0 = hot[i].pad[0];
                    rec[i].absorption = cold[i].amb_absorb.w;
                    for (int r = 0; r < 3; ++r) rec[i].mv_row[r] = cold[i].mv_row[r];
                }
            });
            rec[n_objs].type = 0xffffffffu;
            RT_TRY(hipMalloc((void**)&c->d_objrec, sizeof(rt::ObjectRecord) * rec.size()));
            RT_TRY(hipMemcpy(c->d_objrec, rec.data(), sizeof(rt::ObjectRecord) * rec.size(), hipMemcpyHostToDevice));
        }
        if (!any_triangle) {   // the compact records, and which objects keep the scene from reading them (rt_compact.h)
            const rt_object_data* od = static_cast<const rt_object_data*>(objs);
            std::vector<rt::CompactObject> compact((size_t)n_objs + 1);
            c->h_not_diagonal.assign(n_objs, 0);
            std::atomic<uint32_t> not_diagonal{0};
            parallel_for(n_objs, 16384, [&](size_t i0, size_t i1) {
                uint32_t mine = 0;
                for (size_t i = i0; i < i1; ++i) {
                    compact[i] = pack_compact(od[i].mv, od[i].mvInverse, hot[i].type, cold[i].amb_absorb.w);
                    c->h_not_diagonal[i] = object_not_diagonal(od[i].type, od[i].mv, od[i].mvInverse) ? 1 : 0;
                    mine += c->h_not_diagonal[i];
                }
                not_diagonal.fetch_add(mine, std::memory_order_relaxed);
            });
            c->n_not_diagonal = not_diagonal.load();
            std::memset(&compact[n_objs], 0, sizeof(rt::CompactObject));
            compact[n_objs].type = 0xffffffffu;   // (as the spare HotObject: never hit)
            c->d_compact = reinterpret_cast<rt::CompactObject*>(c->d_hot + n_objs + 1);
            RT_TRY(hipMemcpy(c->d_compact, compact.data(), sizeof(rt::CompactObject) * compact.size(), hipMemcpyHostToDevice));
            const char* env = std::getenv("RT_COMPACT_RECORDS");   // "0": no frame reads them (tests, A/B runs)
            c->compact_allowed = !(env && env[0] == '0');
        }
    }
    lap("hot / cold / object records");
    RT_TRY(hipMalloc((void**)&c->d_lights, sizeof(rt::LightRec) * (size_t)(n_lights + 1)));
    if (n_lights) RT_TRY(hipMemcpy(c->d_lights, lights, sizeof(rt::LightRec) * n_lights, hipMemcpyHostToDevice));
    c->h_lights.resize(n_lights);
    if (n_lights) std::memcpy(static_cast<void*>(c->h_lights.data()), lights, sizeof(rt_light) * n_lights);

    for (uint32_t i = 0; i < n_objs; ++i)
        if (static_cast<const rt_object_data*>(objs)[i].type == 2u) { c->has_triangles = true; break; }
    for (uint32_t i = n_objs; i-- > 0;) {
        const uint32_t ty = static_cast<const rt_object_data*>(objs)[i].type;
        if (ty <= 1u) { c->nan_winner = (int)i; c->nan_winner_sphere = (ty == 0u); break; }
    }
    for (uint32_t i = 0; i < n_objs && c->affine_w; ++i) {
        const rt_object_data& o = static_cast<const rt_object_data*>(objs)[i];
        if (o.type >= 2u) continue;  // vertices, not matrices - or a type that is never hit (RT_TYPE_HIDDEN among them): no kernel reads its rows
        c->affine_w = bottom_rows_affine(o.mv, o.mvInverse);
    }
    {   // per object, for rt_set_transforms: the type and whether both bottom rows are (0,0,0,1) - affine_w is "none is not"
        c->h_kind.resize(n_objs);
        std::atomic<uint32_t> not_affine{0};
        parallel_for(n_objs, 16384, [&](size_t i0, size_t i1) {
            uint32_t mine = 0;
            for (size_t i = i0; i < i1; ++i) {
                const rt_object_data& o = static_cast<const rt_object_data*>(objs)[i];
                const bool affine = o.type >= 2u || bottom_rows_affine(o.mv, o.mvInverse);
                c->h_kind[i] = (uint8_t)(std::min(o.type, 3u) | (affine ? 0u : 0x80u));
                mine += affine ? 0u : 1u;
            }
            not_affine.fetch_add(mine, std::memory_order_relaxed);
        });
        c->n_not_affine = not_affine.load();
    }
    // An instance that can produce a NaN hit time for a FINITE ray (non-finite or singular rows x,y,z of mvInverse:
    // a scale of 0, garbage) makes the reference's result depend on the ORDER its loop meets the objects in - a NaN
    // time overwrites and is overwritten. The exact eliminations (any-hit shadow rays on a size-sorted stream, the
    // grid) assume finite times, so such scenes are rendered the literal way: every ray, every object, in order.
    if (!(c->flags & RT_FLAG_LITERAL)) {
        std::atomic<bool> degenerate{false};
        parallel_for(n_objs, 8192, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1 && !degenerate.load(std::memory_order_relaxed); ++i) {
                const rt_object_data& o = static_cast<const rt_object_data*>(objs)[i];
                if (o.type <= 1u && !std::isfinite(object_bound(o).r)) degenerate.store(true, std::memory_order_relaxed);
            }
        });
        if (degenerate.load()) { c->flags |= RT_FLAG_LITERAL; c->forced_literal = true; c->degenerate_literal = true; }
    }
    // RT_FLAG_DEVICE_OPENCL: the device normalize(0) is 0, so the shadow ray of a light AT the hit point (or of a directional
    // light of direction 0) has a finite start and direction 0. Every sphere of the reference's loop then accepts it with a NaN
    // time and every box that contains the start with MAX_FLOAT: the outcome depends on the order of the loop, which only the
    // literal loops follow. Such a ray needs a light on a surface, i.e. inside an object's bounding sphere.
    // A directional light's shadow rays have the light's own direction, unnormalised: one of |d|^2 outside the walks' window
    // (direction_in_domain; a denormal direction, say) gives an object-space direction that can round to 0 and the same NaN
    // times, so it goes literal too.
    // The predicate follows the lights (rt_set_lights evaluates it again), so what it needs of the objects is kept: lights_need_literal.
    if ((flags & RT_FLAG_DEVICE_OPENCL) && !(c->flags & RT_FLAG_LITERAL)) {
        c->h_obj_bounds.resize(4 * (size_t)n_objs);
        parallel_for(n_objs, 8192, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {
                const Bound b = object_bound(static_cast<const rt_object_data*>(objs)[i]);
                c->h_obj_bounds[4 * i] = b.x; c->h_obj_bounds[4 * i + 1] = b.y; c->h_obj_bounds[4 * i + 2] = b.z; c->h_obj_bounds[4 * i + 3] = b.r;
            }
        });
        if (lights_need_literal(c, static_cast<const rt_light*>(lights), n_lights)) {
            c->flags |= RT_FLAG_LITERAL;
            c->forced_literal = true;
            c->lights_literal = true;
        }
    }
    lap("instance checks");
    c->base_flags = c->flags;
    if (rays && n_rays) {
        const rt_ray* r = static_cast<const rt_ray*>(rays);
        uint32_t W = 0, H = 0;
        float z = 0.f;
        if (!(flags & RT_FLAG_NO_RAYGEN) && detect_pinhole(r, n_rays, W, H, z)) {
            c->pinhole = true;
            c->width = W;
            c->height = H;
            c->z = z;
            c->camera_out_of_domain = !camera_in_domain(W, H, z);
        } else {
            bool w0 = true;
            for (uint64_t i = 0; i < n_rays && w0; ++i) w0 = (r[i].direction[3] == 0.0f);
            c->dir_w_zero = w0;
            for (uint64_t i = 0; i < n_rays && !c->rays_out_of_domain; ++i)
                c->rays_out_of_domain = !direction_in_domain(r[i].direction[0], r[i].direction[1], r[i].direction[2]);
            for (uint64_t i = 0; i < n_rays; ++i) {  // where do primary rays start? (grid margins need it)
                if (r[i].start[3] != 1.0f || !std::isfinite(r[i].start[0] + r[i].start[1] + r[i].start[2])) { c->primary_w_one = false; break; }
                for (int a = 0; a < 3; ++a) {
                    c->origin_lo[a] = std::min(c->origin_lo[a], (double)r[i].start[a]);
                    c->origin_hi[a] = std::max(c->origin_hi[a], (double)r[i].start[a]);
                }
            }
            RT_TRY(hipMalloc((void**)&c->d_rays, sizeof(rt_ray) * (size_t)n_rays));
            RT_TRY(hipMemcpy(c->d_rays, rays, sizeof(rt_ray) * (size_t)n_rays, hipMemcpyHostToDevice));
            c->have_rays = true;
        }
    }
#undef RT_TRY
    apply_ray_domain(c);
    lap("ray scan + upload");
    (void)hipDeviceSynchronize();
    lap("device synchronise");
    c->setup.upload_ms = sw.lap_ms();
    if (n_objs >= kWavefrontGridMinObjects || (flags & RT_FLAG_WAVEFRONT) || c->has_triangles) {
        rc = build_grid(c, static_cast<const rt_object_data*>(objs), n_objs);
        if (rc != RT_OK) return bail(rc);
        c->setup.grid_ms = sw.lap_ms() - c->setup.blocks_ms;  // (build_grid ends with the block grid, which times itself)
        rc = build_light_tiles(c, static_cast<const rt_light*>(lights));
        if (rc != RT_OK) return bail(rc);
        c->setup.light_tiles_ms = sw.lap_ms();
        rc = upload_walk_records(c);
        if (rc != RT_OK) return bail(rc);
        c->setup.grid_ms += sw.lap_ms();
    }
    if (c->has_triangles && (!c->grid.enabled || (c->flags & (RT_FLAG_LITERAL | RT_FLAG_MONOLITHIC | RT_FLAG_NO_GRID)))) {
        fail(c, RT_ERR_INVALID_ARGUMENT,
             "triangle records (type 2, an extension of the reference's two primitives) are traced by the grid path only: "
             "it needs affine instances, ray w = 1, primary directions with 1e-30 < |d|^2 < 1e30, and none of RT_FLAG_LITERAL / "
             "RT_FLAG_MONOLITHIC / RT_FLAG_NO_GRID");
        return bail(RT_ERR_INVALID_ARGUMENT);
    }
    c->setup.create_ms = sw_total.lap_ms();
    *out_ctx = c;
    return RT_OK;
}

int rt_get_setup_times(rt_context* c, rt_setup_times_t* t) {
    if (!c || !t) return RT_ERR_INVALID_ARGUMENT;
    *t = c->setup;
    return RT_OK;
}

int rt_set_camera(rt_context* c, uint32_t width, uint32_t height, float z) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (width == 0 || height == 0 || (uint64_t)width * height != c->n_rays)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "width*height must equal n_rays");
    if (width > 0x1000000u || height > 0x1000000u) return fail(c, RT_ERR_INVALID_ARGUMENT, "grid too large");
    const bool out = !camera_in_domain(width, height, z);
    if (out && c->has_triangles)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "a camera with a direction of |d|^2 outside (1e-30, 1e30) needs the literal loops, which do not know triangle records");
    if (c->ss > 1) {
        const int rc = check_supersampling(c, c->ss, true, width, height, c->shard.tile_rays, c->shard.world);
        if (rc) return rc;
    }
    c->camera_out_of_domain = out;
    c->pinhole = true;
    c->pose_w = c->pose_h = 0;
    c->pose_outside = c->primary_outside = false;
    apply_ray_domain(c);
    c->width = width;
    c->height = height;
    c->z = z;
    c->rects_dirty = true;
    c->tiles_dirty = true;
    return RT_OK;
}

// ---- replaceable rays (hip_raytracer.h) ----
// Scan (rt_rays.hip) on the caller's stream, verdict on the host, then - only if the context can render these rays - the copy
// into the context's own buffer and the new state. Nothing of the context changes before the verdict is accepted.
static int check_set_rays(rt_context* c, const void* rays, uint64_t n_rays) {
    if (!rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "the ray array is NULL");
    if (n_rays != c->n_rays || n_rays == 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "n_rays must equal the context's ray count (the state buffers are sized by it)");
    if (c->ss > 1)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "a supersampling factor > 1 needs a pinhole camera: set the factor to 1 before replacing the rays");
    return RT_OK;
}

static int set_rays_from_device(rt_context* c, const void* d_src, uint64_t n_rays, hipStream_t stream) {
    const int refused = check_set_rays(c, d_src, n_rays);
    if (refused) return refused;
    if (reinterpret_cast<uintptr_t>(d_src) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the ray array must be 16-byte aligned");
    RT_DEVICE(c);
    if (!c->d_scan) RT_HIP(c, hipMalloc((void**)&c->d_scan, sizeof(rt::RayScan)));
    if (!c->h_scan) RT_HIP(c, hipHostMalloc((void**)&c->h_scan, sizeof(rt::RayScan), hipHostMallocDefault));
    // engineering aid (RT_RAYS_TRACE=1, tools/ab/set_rays_timing.py): device time of the scan and of the copy, on stderr
    const bool trace = std::getenv("RT_RAYS_TRACE") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventPair { hipEvent_t* e; ~EventPair() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    if (trace) { RT_HIP(c, hipEventCreate(&ev[0])); RT_HIP(c, hipEventCreate(&ev[1])); }
    if (trace) RT_HIP(c, hipEventRecord(ev[0], stream));
    const hipError_t e = rt::launch_ray_scan(static_cast<const float4*>(d_src), n_rays, c->d_scan, stream);
    if (e != hipSuccess) return fail_hip(c, e, "ray scan launch");
    if (trace) RT_HIP(c, hipEventRecord(ev[1], stream));
    RT_HIP(c, hipMemcpyAsync(c->h_scan, c->d_scan, sizeof(rt::RayScan), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    const rt::RayScan v = *c->h_scan;
    const bool dir_w_zero = !(v.flags & rt::kRayDirW), in_domain = !(v.flags & rt::kRayDomain), starts_ok = !(v.flags & rt::kRayStart);
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool inside = starts_ok;
    for (int a = 0; a < 3 && starts_ok; ++a) {
        const uint32_t lo_bits = rt::ray_unkey(~v.lo_inv[a]), hi_bits = rt::ray_unkey(v.hi[a]);
        float f_lo, f_hi;
        std::memcpy(&f_lo, &lo_bits, 4);
        std::memcpy(&f_hi, &hi_bits, 4);
        lo[a] = (double)f_lo;
        hi[a] = (double)f_hi;
        inside = inside && lo[a] >= c->grid_box_lo[a] && hi[a] <= c->grid_box_hi[a];
    }
    const bool on_grid = c->grid.enabled && dir_w_zero && starts_ok && inside;
    if (c->has_triangles && (!on_grid || !in_domain))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "triangle records are traced by the grid path only: these rays need the literal loops (a direction of |d|^2 outside "
                    "(1e-30, 1e30)) or brute force (direction.w != 0, start.w != 1 or not finite, or an origin outside the box the grid was built for)");
    float scan_ms = 0.f, copy_ms = 0.f;
    if (trace) RT_HIP(c, hipEventElapsedTime(&scan_ms, ev[0], ev[1]));
    if (!c->d_rays) RT_HIP(c, hipMalloc((void**)&c->d_rays, sizeof(rt_ray) * (size_t)n_rays));
    if (trace) RT_HIP(c, hipEventRecord(ev[0], stream));
    RT_HIP(c, hipMemcpyAsync(c->d_rays, d_src, sizeof(rt_ray) * (size_t)n_rays, hipMemcpyDeviceToDevice, stream));
    if (trace) RT_HIP(c, hipEventRecord(ev[1], stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (trace) {
        RT_HIP(c, hipEventElapsedTime(&copy_ms, ev[0], ev[1]));
        std::fprintf(stderr, "[rt_set_rays] scan %.4f ms copy %.4f ms rays %llu\n", (double)scan_ms, (double)copy_ms, (unsigned long long)n_rays);
    }
    c->have_rays = true;
    c->pinhole = false;
    c->width = c->height = 0;
    c->pose_w = c->pose_h = 0;
    c->z = 0.f;
    c->dir_w_zero = dir_w_zero;
    c->primary_w_one = starts_ok;
    c->rays_out_of_domain = !in_domain;
    c->rays_off_grid = !on_grid;
    c->pose_outside = c->primary_outside = false;  // (a buffer has no common origin and no table: outside the box it stays brute force)
    for (int a = 0; a < 3; ++a) { c->origin_lo[a] = lo[a]; c->origin_hi[a] = hi[a]; }
    apply_ray_domain(c);
    c->rects_dirty = true;
    c->tiles_dirty = true;
    return RT_OK;
}

int rt_set_rays_device(rt_context* c, const void* d_rays, uint64_t n_rays, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    return set_rays_from_device(c, d_rays, n_rays, static_cast<hipStream_t>(hip_stream));
}

int rt_set_rays(rt_context* c, const void* rays, uint64_t n_rays) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_rays(c, rays, n_rays);
    if (refused) return refused;
    RT_DEVICE(c);
    void* staged = nullptr;  // the context's own buffer keeps the rays in use until the scan has accepted the new ones
    RT_HIP(c, hipMalloc(&staged, sizeof(rt_ray) * (size_t)n_rays));
    hipError_t e = hipMemcpy(staged, rays, sizeof(rt_ray) * (size_t)n_rays, hipMemcpyHostToDevice);
    const int rc = e == hipSuccess ? set_rays_from_device(c, staged, n_rays, c->stream) : fail_hip(c, e, "upload of the rays");
    (void)hipFree(staged);
    return rc;
}

int rt_set_pose(rt_context* c, uint32_t width, uint32_t height, float z, const float* m, const float* origin, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    rt::PoseGrid g;
    int rc = pose_grid(c, width, height, z, m, origin, g);
    if (rc) return rc;
    PoseVerdict v;
    rc = pose_check(c, g, static_cast<hipStream_t>(hip_stream), v);
    if (rc) return rc;
    return pose_commit(c, g, static_cast<hipStream_t>(hip_stream), v);
}

int rt_generate_rays_device(rt_context* c, uint32_t width, uint32_t height, float z, const float* m, const float* origin, void* d_rays,
                            void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    rt::PoseGrid g;
    const int rc = pose_grid(c, width, height, z, m, origin, g);
    if (rc) return rc;
    if (width == 0 || height == 0) return RT_OK;
    if (!d_rays) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_generate_rays_device: NULL ray array");
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the ray array must be 16-byte aligned");
    RT_DEVICE(c);
    const hipError_t e = rt::launch_pose_rays(g, static_cast<float4*>(d_rays), static_cast<hipStream_t>(hip_stream));
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "pose generation launch");
}

int rt_get_rays_info(const rt_context* cc, rt_rays_info_t* info) {
    if (!cc || !info) return RT_ERR_INVALID_ARGUMENT;
    rt_context* c = const_cast<rt_context*>(cc);
    {   // (a pose outside the box: whether the grid serves the next frame is its table's verdict - built now, as rt_get_tiles_info does)
        const int rc = settle_outside_pose(c, c->stream);
        if (rc) return rc;
    }
    std::memset(info, 0, sizeof(*info));
    info->source = c->pinhole ? 1u : (c->have_rays ? (c->pose_w ? 3u : 2u) : 0u);
    const bool buffer = info->source >= 2u;
    info->dir_w_zero = (!buffer || c->dir_w_zero) ? 1u : 0u;
    info->directions_in_domain = (c->pinhole ? !c->camera_out_of_domain : !c->rays_out_of_domain) ? 1u : 0u;
    info->starts_ok = (!buffer || c->primary_w_one) ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        info->origin_lo[a] = (buffer && c->primary_w_one) ? (float)c->origin_lo[a] : 0.f;
        info->origin_hi[a] = (buffer && c->primary_w_one) ? (float)c->origin_hi[a] : 0.f;
        info->box_lo[a] = c->grid.enabled ? c->grid_box_lo[a] : 0.0;
        info->box_hi[a] = c->grid.enabled ? c->grid_box_hi[a] : 0.0;
    }
    info->grid_built = c->grid.enabled ? 1u : 0u;
    info->grid_in_use = (grid_in_use(c) && !(c->flags & RT_FLAG_LITERAL)) ? 1u : 0u;
    info->literal = (c->flags & RT_FLAG_LITERAL) ? 1u : 0u;
    info->primary_outside_box = (info->grid_in_use && !c->pinhole && c->rays_off_grid && c->primary_outside) ? 1u : 0u;
    return RT_OK;
}

// ---- screen tiles (hip_raytracer.h) ----
// the tile width (as a shift) do_launch would ask for: 8 x 8 when the work-items of a camera's frame walk 8 x 8 blocks, else 64 x 8
static uint32_t primary_col_shift(const rt_context* c) {
    if (!c->pinhole || !c->width) return 6u;
    const Shard& sh = c->shard;
    const bool row_tiles = sh.world <= 1 || (sh.tile_rays % c->width == 0 && (sh.tile_rays / c->width) % 8 == 0);
    if (!(row_tiles && sh.n_local % c->width == 0 && sh.n_local < 0x7fffffffull)) return 6u;
    return (c->width % 8u == 0 && (uint32_t)(sh.n_local / c->width) % 8u == 0) ? 3u : 6u;
}

// the table is a cache of the context's rays: building it on demand changes nothing a caller can observe but the answer
static int tiles_current(rt_context* c) {
    if (const int rc = settle_outside_pose(c, c->stream)) return rc;
    if (!use_wavefront(c) || (!c->pinhole && !c->have_rays)) {
        // (a pose outside the box whose table was refused, on a scene that takes the small-scene kernel without the grid: the reason stays)
        const uint32_t why = (!c->pinhole && c->have_rays && c->pose_w && c->pose_outside && !c->tiles_dirty) ? c->tiles_info.refused : 0u;
        c->tiles_info = rt_tiles_info_t{};
        c->tiles_info.refused = RT_TILES_REFUSED_NO_GRID | why;
        return RT_OK;
    }
    const uint32_t col_shift = primary_col_shift(c);
    if (!c->tiles_dirty && c->tiles_built_for == col_shift) return RT_OK;
    RT_DEVICE(c);
    StopWatch sw;
    const int rc = refresh_screen_tiles(c, c->stream, col_shift);
    if (rc == RT_OK) c->setup.screen_tiles_ms += sw.lap_ms();
    return rc;
}

int rt_get_tiles_info(const rt_context* cc, rt_tiles_info_t* info) {
    if (!cc || !info) return RT_ERR_INVALID_ARGUMENT;
    rt_context* c = const_cast<rt_context*>(cc);
    const int rc = tiles_current(c);
    if (rc) return rc;
    *info = c->tiles_info;
    if (!info->enabled || !(grid_in_use(c) && !(c->flags & RT_FLAG_LITERAL))) {  // (a camera's table of a frame the literal loops render)
        info->enabled = 0;
        info->source = 0;
        if (!info->refused) info->refused = RT_TILES_REFUSED_NO_GRID;
        return RT_OK;
    }
    if (info->source == 1u) {  // the host builder keeps no list lengths: read the offsets back
        const size_t n_tiles = (size_t)info->tiles_x * info->tiles_y;
        std::vector<uint32_t> start(n_tiles + 1);
        RT_DEVICE(c);
        RT_HIP(c, hipMemcpy(start.data(), c->tiles.tile_start, sizeof(uint32_t) * (n_tiles + 1), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < n_tiles; ++t) info->max_list = std::max(info->max_list, start[t + 1] - start[t]);
    }
    return RT_OK;
}

int rt_read_tiles(rt_context* c, uint32_t* tile_start, uint64_t n_start, uint32_t* entries, uint64_t n_entries) {
    if (!c || !tile_start || !entries) return RT_ERR_INVALID_ARGUMENT;
    rt_tiles_info_t info;
    const int rc = rt_get_tiles_info(c, &info);
    if (rc) return rc;
    if (!info.enabled) return fail(c, RT_ERR_STATE, "rt_read_tiles: the next frame uses no screen tiles (rt_get_tiles_info has the reason)");
    const uint64_t n_tiles = (uint64_t)info.tiles_x * info.tiles_y, total = info.n_entries + info.n_global;
    if (n_start < n_tiles + 1 || n_entries < total) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_read_tiles: an array is too small for the table");
    RT_DEVICE(c);
    RT_HIP(c, hipMemcpy(tile_start, c->tiles.tile_start, sizeof(uint32_t) * (size_t)(n_tiles + 1), hipMemcpyDeviceToHost));
    if (total) RT_HIP(c, hipMemcpy(entries, c->tiles.entries, sizeof(uint2) * (size_t)total, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_read_grid_spheres(const rt_context* c, double* spheres, uint64_t n) {
    if (!c || !spheres) return RT_ERR_INVALID_ARGUMENT;
    if (!c->grid.enabled || c->h_grid_spheres.size() != 4 * (size_t)c->n_objs)
        return fail(const_cast<rt_context*>(c), RT_ERR_STATE, "rt_read_grid_spheres: the context has no grid");
    if (n != c->n_objs) return fail(const_cast<rt_context*>(c), RT_ERR_INVALID_ARGUMENT, "rt_read_grid_spheres: n must be the object count");
    std::memcpy(spheres, c->h_grid_spheres.data(), sizeof(double) * 4 * (size_t)n);
    return RT_OK;
}

int rt_read_pose_spheres(rt_context* c, double* spheres, uint64_t n) {
    if (!c || !spheres) return RT_ERR_INVALID_ARGUMENT;
    rt_tiles_info_t info;
    const int rc = rt_get_tiles_info(c, &info);
    if (rc) return rc;
    if (!info.enabled || info.source != 3u || !c->d_outside_spheres)
        return fail(c, RT_ERR_STATE, "rt_read_pose_spheres: the current screen tiles were not built from per-pose spheres (rt_tiles_info_t::source != 3)");
    if (n != c->n_objs) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_read_pose_spheres: n must be the object count");
    RT_DEVICE(c);
    RT_HIP(c, hipMemcpy(spheres, c->d_outside_spheres, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_read_object_bounds(const rt_context* c, double* bounds, uint64_t n) {
    if (!c || !bounds) return RT_ERR_INVALID_ARGUMENT;
    if (!c->grid.enabled || c->h_obj_bound6.size() != rt::kBoundDoubles * (size_t)c->n_objs)
        return fail(const_cast<rt_context*>(c), RT_ERR_STATE, "rt_read_object_bounds: the context keeps no bounds (no grid, or a scene with triangles)");
    if (n != c->n_objs) return fail(const_cast<rt_context*>(c), RT_ERR_INVALID_ARGUMENT, "rt_read_object_bounds: n must be the object count");
    std::memcpy(bounds, c->h_obj_bound6.data(), sizeof(double) * rt::kBoundDoubles * (size_t)n);
    return RT_OK;
}

int rt_get_grid_constants(const rt_context* c, double constants[4]) {
    if (!c || !constants) return RT_ERR_INVALID_ARGUMENT;
    if (!c->grid.enabled) return fail(const_cast<rt_context*>(c), RT_ERR_STATE, "rt_get_grid_constants: the context has no grid");
    constants[0] = c->grid_cell;
    constants[1] = c->grid_diag;
    constants[2] = c->grid_s_max;
    constants[3] = c->grid_k2;
    return RT_OK;
}

// ---- replaceable lights (hip_raytracer.h) ----
int rt_set_lights(rt_context* c, const void* lights, uint32_t n_lights) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_set_lights(c, lights, n_lights);
    if (refused) return refused;
    RT_DEVICE(c);
    const rt_light* L = static_cast<const rt_light*>(lights);
    if (n_lights > c->lights_capacity) {  // a larger array first: a failed allocation leaves the context as it was
        rt::LightRec* d = nullptr;
        RT_HIP(c, hipMalloc((void**)&d, sizeof(rt::LightRec) * ((size_t)n_lights + 1)));
        if (c->d_lights) (void)hipFree(c->d_lights);
        c->d_lights = d;
        c->lights_capacity = n_lights;
    }
    if (n_lights) {
        RT_HIP(c, hipMemcpyAsync(c->d_lights, lights, sizeof(rt::LightRec) * n_lights, hipMemcpyHostToDevice, c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));  // `lights` may be pageable and is the caller's again on return
    }
    c->n_lights = n_lights;
    c->h_lights.assign(L, L + n_lights);  // (rt_set_transforms and rt_set_visibility evaluate the predicate below again, the former rebuilds the light tiles)
    refresh_lights_literal(c, L, n_lights);
    return build_light_tiles_device(c, L);
}

int rt_read_grid_pretest(const rt_context* c, float* pre, uint64_t n) {
    if (!c || !pre) return RT_ERR_INVALID_ARGUMENT;
    if (!c->grid.enabled || c->h_grid_pre.size() != c->n_objs)
        return fail(const_cast<rt_context*>(c), RT_ERR_STATE, "rt_read_grid_pretest: the context has no grid");
    if (n != c->n_objs) return fail(const_cast<rt_context*>(c), RT_ERR_INVALID_ARGUMENT, "rt_read_grid_pretest: n must be the object count");
    std::memcpy(pre, c->h_grid_pre.data(), sizeof(float) * (size_t)n);
    return RT_OK;
}

int rt_get_light_tiles_info(const rt_context* c, rt_light_tiles_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    *info = c->lt_info;
    return RT_OK;
}

int rt_read_light_tiles(rt_context* c, uint32_t* tile_start, uint64_t n_start, uint32_t* entries, uint64_t n_entries) {
    if (!c || !tile_start || !entries) return RT_ERR_INVALID_ARGUMENT;
    const rt_light_tiles_info_t& info = c->lt_info;
    const rt::LightTiles& lt = c->light_tiles;
    if (!info.enabled || !lt.blocks_enabled || !info.n_blocks)
        return fail(c, RT_ERR_STATE, "rt_read_light_tiles: no light tiles in block form are in use (rt_get_light_tiles_info has the reason)");
    const uint64_t n_tiles = (uint64_t)info.tiles_u * info.tiles_v;
    if (n_start < n_tiles + 1 || n_entries < info.n_entries) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_read_light_tiles: an array is too small for the table");
    RT_DEVICE(c);
    std::vector<uint32_t> blk(8 * (size_t)info.n_blocks), ids(4 * (size_t)info.n_blocks);
    RT_HIP(c, hipMemcpy(blk.data(), lt.blocks, sizeof(uint32_t) * blk.size(), hipMemcpyDeviceToHost));
    RT_HIP(c, hipMemcpy(ids.data(), lt.block_ids, sizeof(uint32_t) * ids.size(), hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (uint64_t t = 0; t < n_tiles; ++t) {  // the chains as the kernels walk them; an empty slot (k8 = 255, r8 = 0) ends a list
        tile_start[t] = (uint32_t)at;
        uint64_t steps = 0;
        for (uint32_t bl = (uint32_t)t;;) {
            bool ended = false;
            for (uint32_t e = 0; e < 3u; ++e) {
                const uint32_t lo = blk[8 * (size_t)bl + 2 + 2 * e], hi = blk[8 * (size_t)bl + 3 + 2 * e];
                if ((hi >> 16) == 0xff00u) { ended = true; break; }
                if (at >= info.n_entries) return fail(c, RT_ERR_STATE, "internal: the light tiles' chains hold more entries than the table");
                entries[3 * at] = ids[4 * (size_t)bl + e];
                entries[3 * at + 1] = lo;
                entries[3 * at + 2] = hi;
                ++at;
            }
            const uint32_t next = blk[8 * (size_t)bl];
            if (ended || next == 0u) break;
            if (next >= info.n_blocks || ++steps > info.n_blocks) return fail(c, RT_ERR_STATE, "internal: a light tile's chain leaves the table");
            bl = next;
        }
    }
    tile_start[n_tiles] = (uint32_t)at;
    if (at != info.n_entries) return fail(c, RT_ERR_STATE, "internal: the light tiles' chains do not hold the table's entries");
    return RT_OK;
}

int rt_set_shard(rt_context* c, uint64_t tile_rays, uint32_t rank, uint32_t world) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (world == 0 || rank >= world || (world > 1 && tile_rays == 0))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "need world >= 1, rank < world, tile_rays > 0");
    if (c->ss > 1) {
        const int rc = check_supersampling(c, c->ss, has_sample_grid(c), sample_width(c), sample_height(c), tile_rays, world);
        if (rc) return rc;
    }
    c->shard = Shard{tile_rays, rank, world, 1, local_count(c->n_rays, tile_rays, rank, world)};
    return RT_OK;
}

uint64_t rt_local_rays(const rt_context* c) { return c ? c->shard.n_local : 0; }

int rt_set_supersampling(rt_context* c, uint32_t s) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int rc = check_supersampling(c, s, has_sample_grid(c), sample_width(c), sample_height(c), c->shard.tile_rays, c->shard.world);
    if (rc) return rc;
    c->ss = s;
    return RT_OK;
}

uint32_t rt_supersampling(const rt_context* c) { return c ? c->ss : 0; }

uint64_t rt_local_pixels(const rt_context* c) { return c ? local_pixels(c) : 0; }

int rt_get_stats(rt_context* c, rt_stats_t* s) {
    if (!c || !s) return RT_ERR_INVALID_ARGUMENT;
    RT_DEVICE(c);
    if (c->ev_count) {
        const uint32_t slot = (c->ev_count - 1) % kTimingSlots;
        RT_HIP(c, hipEventSynchronize(c->ev_end[slot]));
        RT_HIP(c, hipEventElapsedTime(&c->last_ms, c->ev_begin[slot], c->ev_end[slot]));
    }
    s->rays_traced = c->counters.traced;
    s->rays_reference = c->counters.reference;
    s->hit_pixels = c->counters.hits;
    s->last_kernel_ms = c->last_ms;
    s->pinhole = c->pinhole ? 1u : 0u;
    s->width = c->pinhole ? c->width : 0;
    s->height = c->pinhole ? c->height : 0;
    s->local_rays = c->shard.n_local;
    s->wavefront = c->last_wavefront ? 1u : 0u;
    s->rounds = c->last_rounds;
    s->object_tests = c->counters.tests;
    return RT_OK;
}

int rt_timing_reset(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    c->ev_count = 0;
    return RT_OK;
}

int rt_timing_summary(rt_context* c, double* sum_ms, uint32_t* launches) {
    if (!c || !sum_ms || !launches) return RT_ERR_INVALID_ARGUMENT;
    RT_DEVICE(c);
    const uint32_t n = c->ev_count < kTimingSlots ? c->ev_count : kTimingSlots;
    double total = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        float ms = 0.f;
        RT_HIP(c, hipEventSynchronize(c->ev_end[i]));
        RT_HIP(c, hipEventElapsedTime(&ms, c->ev_begin[i], c->ev_end[i]));
        total += ms;
    }
    *sum_ms = total;
    *launches = n;
    return RT_OK;
}

void rt_destroy(rt_context* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_pairs) (void)hipFree(c->d_pairs);
    if (c->d_shadow_pairs) (void)hipFree(c->d_shadow_pairs);
    if (c->d_hot) (void)hipFree(c->d_hot);
    if (c->d_cold) (void)hipFree(c->d_cold);
    if (c->d_objrec) (void)hipFree(c->d_objrec);
    if (c->d_vis_types) (void)hipFree(c->d_vis_types);
    if (c->d_vis_slots) (void)hipFree(c->d_vis_slots);
    if (c->d_bounds) (void)hipFree(c->d_bounds);
    if (c->d_grid_cell_range) (void)hipFree(c->d_grid_cell_range);
    if (c->d_grid_cell_rec) (void)hipFree(c->d_grid_cell_rec);
    if (c->d_grid_entries) (void)hipFree(c->d_grid_entries);
    if (c->d_grid_always) (void)hipFree(c->d_grid_always);
    if (c->d_grid_entry_sphere) (void)hipFree(c->d_grid_entry_sphere);
    if (c->d_tile_start) (void)hipFree(c->d_tile_start);
    if (c->d_tile_entries) (void)hipFree(c->d_tile_entries);
    if (c->d_pose_spheres) (void)hipFree(c->d_pose_spheres);
    if (c->d_obj_bound6) (void)hipFree(c->d_obj_bound6);
    if (c->d_outside_spheres) (void)hipFree(c->d_outside_spheres);
    if (c->ptb.rect) (void)hipFree(c->ptb.rect);
    if (c->ptb.key) (void)hipFree(c->ptb.key);
    if (c->ptb.count) (void)hipFree(c->ptb.count);
    if (c->ptb.cursor) (void)hipFree(c->ptb.cursor);
    if (c->ptb.sums) (void)hipFree(c->ptb.sums);
    if (c->ptb.record) (void)hipFree(c->ptb.record);
    if (c->ptb.scratch) (void)hipFree(c->ptb.scratch);
    if (c->ptb.tile_start) (void)hipFree(c->ptb.tile_start);
    if (c->ptb.entries) (void)hipFree(c->ptb.entries);
    if (c->h_pose_record) (void)hipHostFree(c->h_pose_record);
    for (hipEvent_t ev : c->ev_tiles) if (ev) (void)hipEventDestroy(ev);
    if (c->d_lt_range) (void)hipFree(c->d_lt_range);
    if (c->d_lt_records) (void)hipFree(c->d_lt_records);
    if (c->d_lt_blocks) (void)hipFree(c->d_lt_blocks);
    if (c->d_lt_block_ids) (void)hipFree(c->d_lt_block_ids);
    if (c->d_walk_rec) (void)hipFree(c->d_walk_rec);
    if (c->d_walk_blocks) (void)hipFree(c->d_walk_blocks);
    if (c->d_walk_ids) (void)hipFree(c->d_walk_ids);
    if (c->d_lights) (void)hipFree(c->d_lights);
    {   // the light-tile builder's memory (rt_set_lights)
        rt::LightTileBuffers& b = c->ltb;
        void* arrays[] = {c->d_lt_pre, b.span, b.wq, b.packed, b.record, b.blocks, b.block_ids, b.lists.rect, b.lists.key, b.lists.sums,
                          b.lists.record, b.lists.count, b.lists.cursor, b.lists.tile_start, b.lists.scratch, b.lists.entries,
                          b.chains.sums, b.chains.record, b.chains.count, b.chains.cursor, b.chains.tile_start};
        for (void* p : arrays)
            if (p) (void)hipFree(p);
        if (c->h_lt_record) (void)hipHostFree(c->h_lt_record);
        if (c->h_lt_lists) (void)hipHostFree(c->h_lt_lists);
        for (hipEvent_t ev : c->ev_lt)
            if (ev) (void)hipEventDestroy(ev);
    }
    if (c->d_rays) (void)hipFree(c->d_rays);
    if (c->d_scan) (void)hipFree(c->d_scan);
    if (c->h_scan) (void)hipHostFree(c->h_scan);
    for (CountedSlot* s : {&c->query, &c->query_shade, &c->gb_records, &c->ao, &c->ao_filter}) {
        if (s->made) (void)hipEventSynchronize(s->ev[1]);  // (a device-form query or pass may still run on the caller's stream)
        if (s->d_counters) (void)hipFree(s->d_counters);
        for (hipEvent_t ev : s->ev) if (ev) (void)hipEventDestroy(ev);
    }
    for (hipEvent_t ev : c->ev_gb_trace) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->ev_ao_gbuffer) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->ev_ao_filter_frame) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->ev_xf) if (ev) (void)hipEventDestroy(ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t ev : c->ev_pass) if (ev) (void)hipEventDestroy(ev);
    if (c->d_counters) (void)hipFree(c->d_counters);
    free_wavefront(c);
    for (uint32_t i = 0; i < c->ev_begin_made; ++i) (void)hipEventDestroy(c->ev_begin[i]);
    for (uint32_t i = 0; i < c->ev_end_made; ++i) (void)hipEventDestroy(c->ev_end[i]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

}  // extern "C"
