// rt_api.cpp - the C ABI of include/hip_raytracer.h: context life cycle, scene re-pack + upload, render.
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

static size_t elem_bytes(const rt_context* c) { return c->kernel == RT_KERNEL_HITTEST ? sizeof(float) : 4 * sizeof(float); }

// tiles of the frame that ranks rank .. rank + span - 1 of `world` own (tile t belongs to rank t % world)
static uint64_t local_tiles(uint64_t tiles, uint32_t rank, uint32_t world, uint32_t span) {
    const uint64_t rest = tiles % world;
    return (tiles / world) * span + (rest > rank ? std::min<uint64_t>(rest - rank, span) : 0);
}

static uint64_t local_count(uint64_t n_rays, uint64_t tile_rays, uint32_t rank, uint32_t world, uint32_t span = 1) {
    if (world <= 1) return n_rays;
    const uint64_t tiles = (n_rays + tile_rays - 1) / tile_rays;
    return local_tiles(tiles, rank, world, span) * tile_rays;  // the last tile may be ragged: its padding work-items write background
}

static int ensure_out(rt_context* c) {
    const size_t need = (size_t)c->n_local * elem_bytes(c);
    return need > c->d_out_bytes ? grow_buffer(c, c->d_out, c->d_out_bytes, need, false) : RT_OK;
}

static int ensure_host_out(rt_context* c) {
    const size_t need = (size_t)c->n_local * elem_bytes(c);
    return need > c->h_out_bytes ? grow_buffer(c, c->h_out, c->h_out_bytes, need, true) : RT_OK;
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

// what the three packed render entry points refuse before they touch anything
static int check_packed(rt_context* c, int format) {
    if (!packed_bytes(format)) return fail(c, RT_ERR_INVALID_ARGUMENT, "unknown pixel format (RT_PIXEL_RGBA8 = 1, RT_PIXEL_RGB8 = 2)");
    if (c->kernel == RT_KERNEL_HITTEST)
        return fail(c, RT_ERR_STATE, "an RT_KERNEL_HITTEST context renders one float (the nearest t) per ray, not a colour: there is no 8-bit frame of it");
    return RT_OK;
}

static int pack_on(rt_context* c, const void* d_src, uint64_t n, int format, void* d_dst, hipStream_t stream) {
    const hipError_t e = rt::launch_pack(static_cast<const float4*>(d_src), n, format, d_dst, stream);
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "pack launch");
}

static uint32_t sample_height(const rt_context* c) { return c->pinhole ? c->height : c->pose_h; }
static bool has_sample_grid(const rt_context* c) { return c->pinhole || c->pose_w != 0; }

static uint64_t local_pixels(const rt_context* c) { return c->n_local / ((uint64_t)c->ss * c->ss); }

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

// s x s samples -> one pixel: `n_samples` consecutive samples of whole sample rows of the context's camera (a shard's tiles are that)
static int resolve_on(rt_context* c, const void* d_src, uint64_t n_samples, int format, void* d_dst, hipStream_t stream) {
    if (n_samples == 0) return RT_OK;
    const hipError_t e = rt::launch_resolve(static_cast<const float4*>(d_src), sample_width(c), (uint32_t)(n_samples / sample_width(c)), c->ss, format, d_dst, stream);
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "resolve launch");
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

static bool use_wavefront(const rt_context* c) {
    if (c->has_triangles) return true;
    if (c->flags & RT_FLAG_WAVEFRONT) return true;
    if (c->flags & RT_FLAG_MONOLITHIC) return false;
    if (c->n_objs >= kWavefrontMinObjects) return true;
    return c->n_objs >= kWavefrontGridMinObjects && grid_in_use(c) && !(c->flags & RT_FLAG_LITERAL);
}

static void free_wavefront(rt_context* c) {
    rt::WavefrontBuffers& b = c->wf;
    if (b.side_stream) (void)hipStreamDestroy(b.side_stream);
    if (b.ev_fork) (void)hipEventDestroy(b.ev_fork);
    if (b.ev_join) (void)hipEventDestroy(b.ev_join);
    b.side_stream = nullptr; b.ev_fork = b.ev_join = nullptr;
    if (b.state) (void)hipFree(b.state);
    for (int i = 0; i < 2; ++i) {
        if (b.q_closest[i]) (void)hipFree(b.q_closest[i]);
        if (b.q_any[i]) (void)hipFree(b.q_any[i]);
        if (b.q_slice[i]) (void)hipFree(b.q_slice[i]);
    }
    if (b.counts) (void)hipFree(b.counts);
    if (b.h_counts) (void)hipHostFree(b.h_counts);
    b = rt::WavefrontBuffers{};
}

static int ensure_wavefront(rt_context* c) {
    rt::WavefrontBuffers& b = c->wf;
    if (b.capacity >= c->n_local && b.state) return RT_OK;
    free_wavefront(c);
    const uint64_t n = c->n_local ? c->n_local : 1;
    RT_HIP(c, hipMalloc((void**)&b.state, rt::wavefront_state_bytes(n)));
    for (int i = 0; i < 2; ++i) {
        RT_HIP(c, hipMalloc((void**)&b.q_closest[i], rt::wavefront_queue_bytes(n)));
        RT_HIP(c, hipMalloc((void**)&b.q_any[i], rt::wavefront_queue_bytes(n)));
        RT_HIP(c, hipMalloc((void**)&b.q_slice[i], rt::wavefront_queue_bytes(n)));
    }
    RT_HIP(c, hipMalloc((void**)&b.counts, rt::wavefront_counter_bytes()));  // device-side round state + run-ticket counters
    RT_HIP(c, hipHostMalloc((void**)&b.h_counts, 16 * sizeof(uint32_t), hipHostMallocDefault));
    RT_HIP(c, hipStreamCreateWithFlags(&b.side_stream, hipStreamNonBlocking));
    RT_HIP(c, hipEventCreateWithFlags(&b.ev_fork, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&b.ev_join, hipEventDisableTiming));
    b.shadow_pairs = c->d_shadow_pairs;
    b.grid = c->grid;
    b.light_tiles = c->light_tiles;
    b.blocks = c->blocks;
    b.capacity = n;
    return RT_OK;
}

static int do_launch(rt_context* c, void* d_out, hipStream_t stream, bool count) {
    if (c->n_local == 0) {  // empty launch: nothing to render, nothing to time
        if (count) c->counters = rt::Counters{};
        c->aux_t = nullptr;
        c->aux_index = nullptr;
        return RT_OK;
    }
    if (!c->pinhole && !c->have_rays)
        return fail(c, RT_ERR_STATE, "no primary rays: rt_create got rays == NULL and rt_set_camera was not called");
    rt::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    p.scene.pairs = c->d_pairs;
    p.scene.n_pairs = c->n_pairs;
    p.scene.hot = c->d_hot;
    p.scene.bounds = c->d_bounds;
    p.scene.cold = c->d_cold;
    p.scene.objrec = c->d_objrec;
    p.scene.lights = c->d_lights;
    p.scene.n_objs = c->n_objs;
    p.scene.n_lights = c->n_lights;
    p.scene.literal = (c->flags & RT_FLAG_LITERAL) ? 1u : 0u;
    p.scene.fast_phong = (c->flags & RT_FLAG_FAST_PHONG) ? 1u : 0u;
    p.scene.affine = (c->affine_w && !c->has_triangles) ? 1u : 0u;
    p.scene.nan_winner = c->nan_winner;
    p.scene.nan_winner_sphere = c->nan_winner_sphere ? 1u : 0u;
    p.rays = c->pinhole ? nullptr : c->d_rays;
    p.n_rays = c->n_rays;
    p.n_local = c->n_local;
    p.tile_rays = c->tile_rays ? c->tile_rays : 1;
    p.run_rays = p.tile_rays * c->span;
    p.rank = c->rank;
    p.world = c->world;
    p.pinhole = c->pinhole ? 1u : 0u;
    p.width = c->width ? c->width : 1;
    p.half_w = (float)c->width / 2.0f;
    p.half_h = (float)c->height / 2.0f;
    p.height_f = (float)c->height;
    p.z = c->z;
    p.dir_w_zero = (c->pinhole || c->dir_w_zero) ? 1u : 0u;
    // 2-D pixel bundles need the grid shape (pinhole mode) and shard tiles made of whole 8-row bands
    const bool row_tiles = c->world <= 1 || (c->width && c->tile_rays % c->width == 0 && (c->tile_rays / c->width) % 8 == 0);
    if (c->pinhole && row_tiles && c->n_local % c->width == 0 && c->n_local < 0x7fffffffull) {
        p.tile2d = 1u;
        p.bundles_x = (c->width + 7u) / 8u;
        p.local_rows = (uint32_t)(c->n_local / c->width);
        p.tile_rows = c->world > 1 ? (uint32_t)(c->tile_rays / c->width) : p.local_rows;
        if (p.tile_rows == 0) p.tile_rows = 1;
        p.n_bundles = p.bundles_x * ((p.local_rows + 7u) / 8u);
        p.wf_tile_order = (c->width % 8u == 0 && p.local_rows % 8u == 0) ? 1u : 0u;
        p.tile_cull = (c->n_objs > 0 && c->n_objs <= 64 && c->z < 0.0f && !(c->flags & RT_FLAG_LITERAL)) ? 1u : 0u;
    } else {
        if (c->n_local > 0xffffffffull - 64) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many rays for one launch");
        p.n_bundles = (uint32_t)((c->n_local + 63u) / 64u);
    }
    p.max_bounces = c->max_bounces;
    p.out = d_out;
    p.aux_t = c->aux_t;
    p.aux_index = c->aux_index;
    p.counters = c->d_counters;

    RT_DEVICE(c);
    if (p.tile_cull && c->rects_dirty) {  // screen rectangles of the bounding spheres for this camera
        std::vector<float4> rects(c->n_objs);
        for (uint32_t i = 0; i < c->n_objs; ++i)
            rects[i] = screen_rect(Sphere{c->h_spheres[4 * i], c->h_spheres[4 * i + 1], c->h_spheres[4 * i + 2], c->h_spheres[4 * i + 3]},
                                   (double)c->z);
        RT_HIP(c, hipMemcpyAsync(c->d_bounds, rects.data(), sizeof(float4) * c->n_objs, hipMemcpyHostToDevice, stream));
        RT_HIP(c, hipStreamSynchronize(stream));  // `rects` is pageable host memory
        c->rects_dirty = false;
    }
    {   // a pose outside the grid's box: its table decides whether the grid serves the frame, so it is built before the path is chosen
        const int rc = settle_outside_pose(c, stream);
        if (rc) return rc;
    }
    c->last_wavefront = use_wavefront(c);
    c->last_rounds = 0;
    if (c->last_wavefront) {  // one-time host-side set-up (buffers, per-camera screen tiles) stays outside the timed region
        StopWatch sw;
        const bool had_buffers = c->wf.capacity >= c->n_local && c->wf.state;
        int rc = ensure_wavefront(c);
        if (rc) return rc;
        if (!had_buffers) c->setup.buffers_ms += sw.lap_ms();
        // a first-round wave is an 8 x 8 block of pixels (work-items in tile order) or 64 pixels of one row: the tile lists follow
        const uint32_t col_shift = p.wf_tile_order ? 3u : 6u;
        if (c->tiles_dirty || c->tiles_built_for != col_shift) {
            rc = refresh_screen_tiles(c, stream, col_shift);
            if (rc) return rc;
            c->setup.screen_tiles_ms += sw.lap_ms();  // (wall: a posed build's device passes - rt_tiles_info_t::build_device_ms - are inside it)
        }
        c->wf.tiles = c->tiles;
        {   // per frame: the grid's tables, or - for a ray buffer they were not built for - none, which is RT_FLAG_NO_GRID's frame
            const bool on = grid_in_use(c);
            c->wf.grid = on ? c->grid : rt::GridDesc{};
            c->wf.light_tiles = on ? c->light_tiles : rt::LightTiles{};
            c->wf.blocks = on ? c->blocks : rt::BlockGrid{};
            // from outside the box the primary rays must never enter the grid walk: their table is there, or the frame is not rendered
            c->wf.primary_outside = (on && !c->pinhole && c->rays_off_grid) ? 1u : 0u;
            if (c->wf.primary_outside && !(c->tiles.enabled && c->tiles.posed && c->tiles.width && c->tiles.outside))
                return fail(c, RT_ERR_STATE, "internal: a pose outside the grid's box without its screen tiles");
        }
    }
    if (count) RT_HIP(c, hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters), stream));
    const uint32_t slot = c->ev_count % kTimingSlots;
    RT_HIP(c, hipEventRecord(c->ev_begin[slot], stream));
    hipError_t e;
    const int arith = (c->flags & RT_FLAG_DEVICE_OPENCL) ? rt::kDeviceCL : ((c->flags & RT_FLAG_UNFUSED) ? rt::kUnfused : rt::kFused);
    if (c->last_wavefront) e = rt::launch_wavefront(p, c->kernel, arith, count, c->wf, stream, &c->last_rounds);
    else e = rt::launch_render(p, c->kernel, arith, count, stream);
    if (e != hipSuccess) return fail_hip(c, e, "kernel launch");
    RT_HIP(c, hipEventRecord(c->ev_end[slot], stream));
    c->ev_count += 1;
    // aux buffers apply to one render only
    c->aux_t = nullptr;
    c->aux_index = nullptr;
    return RT_OK;
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
        const int rc = check_supersampling(c, c->ss, true, g.width, g.height, c->tile_rays, c->world);
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
    c->n_local = n_rays;
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
        // one spare record keeps the arrays non-null for n_objs == 0
        RT_TRY(hipMalloc((void**)&c->d_hot, sizeof(rt::HotObject) * (size_t)(n_objs + 1)));
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
        c->affine_w = o.mv[3] == 0.f && o.mv[7] == 0.f && o.mv[11] == 0.f && o.mv[15] == 1.f && o.mvInverse[3] == 0.f &&
                      o.mvInverse[7] == 0.f && o.mvInverse[11] == 0.f && o.mvInverse[15] == 1.f;
    }
    {   // per object, for rt_set_transforms: the type and whether both bottom rows are (0,0,0,1) - affine_w is "none is not"
        c->h_kind.resize(n_objs);
        std::atomic<uint32_t> not_affine{0};
        parallel_for(n_objs, 16384, [&](size_t i0, size_t i1) {
            uint32_t mine = 0;
            for (size_t i = i0; i < i1; ++i) {
                const rt_object_data& o = static_cast<const rt_object_data*>(objs)[i];
                const bool affine = o.type >= 2u || (o.mv[3] == 0.f && o.mv[7] == 0.f && o.mv[11] == 0.f && o.mv[15] == 1.f && o.mvInverse[3] == 0.f &&
                                                     o.mvInverse[7] == 0.f && o.mvInverse[11] == 0.f && o.mvInverse[15] == 1.f);
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
        const int rc = check_supersampling(c, c->ss, true, width, height, c->tile_rays, c->world);
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
    const bool row_tiles = c->world <= 1 || (c->tile_rays % c->width == 0 && (c->tile_rays / c->width) % 8 == 0);
    if (!(row_tiles && c->n_local % c->width == 0 && c->n_local < 0x7fffffffull)) return 6u;
    return (c->width % 8u == 0 && (uint32_t)(c->n_local / c->width) % 8u == 0) ? 3u : 6u;
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
    c->tile_rays = tile_rays;
    c->rank = rank;
    c->world = world;
    c->n_local = local_count(c->n_rays, tile_rays, rank, world);
    return RT_OK;
}

uint64_t rt_local_rays(const rt_context* c) { return c ? c->n_local : 0; }

int rt_set_supersampling(rt_context* c, uint32_t s) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int rc = check_supersampling(c, s, has_sample_grid(c), sample_width(c), sample_height(c), c->tile_rays, c->world);
    if (rc) return rc;
    c->ss = s;
    return RT_OK;
}

uint32_t rt_supersampling(const rt_context* c) { return c ? c->ss : 0; }

uint64_t rt_local_pixels(const rt_context* c) { return c ? local_pixels(c) : 0; }

int rt_resolve_device(rt_context* c, const void* d_samples, uint32_t sample_width, uint32_t sample_rows, uint32_t s, int format,
                      void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (s < 1 || s > 4) return fail(c, RT_ERR_INVALID_ARGUMENT, "the supersampling factor is 1, 2, 3 or 4");
    if (format != 0 && !packed_bytes(format)) return fail(c, RT_ERR_INVALID_ARGUMENT, "unknown output (0 = float4, RT_PIXEL_RGBA8 = 1, RT_PIXEL_RGB8 = 2)");
    if (sample_width % s || sample_rows % s) return fail(c, RT_ERR_INVALID_ARGUMENT, "sample_width and sample_rows must be multiples of s");
    const uint64_t n_pixels = (uint64_t)(sample_width / s) * (sample_rows / s);
    if (n_pixels == 0) return RT_OK;
    if (!d_samples || !d_out) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_resolve_device: NULL frame");
    if (reinterpret_cast<uintptr_t>(d_samples) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the sample frame must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & (format ? 3u : 15u))
        return fail(c, RT_ERR_INVALID_ARGUMENT, format ? "d_out must be 4-byte aligned" : "a float4 d_out must be 16-byte aligned");
    RT_DEVICE(c);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (s == 1) {  // nothing to filter: the samples are the pixels
        if (format) return pack_on(c, d_samples, n_pixels, format, d_out, stream);
        RT_HIP(c, hipMemcpyAsync(d_out, d_samples, (size_t)n_pixels * 16, hipMemcpyDeviceToDevice, stream));
        return RT_OK;
    }
    int form = rt::kResolveAuto;  // the measured choice (rt_resolve.hip)
    if (const char* env = std::getenv("RT_RESOLVE_FORM"))  // measurement knob (tools/ab/supersample_timing.py): "pixel" / "sample"
        form = env[0] == 'p' ? rt::kResolveLanePerPixel : (env[0] == 's' ? rt::kResolveLanePerSample : rt::kResolveAuto);
    const hipError_t e = rt::launch_resolve(static_cast<const float4*>(d_samples), sample_width, sample_rows, s, format, d_out, stream, form);
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "resolve launch");
}

int rt_set_aux_device(rt_context* c, void* d_hit_t, void* d_hit_index) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->ss > 1 && (d_hit_t || d_hit_index))
        return fail(c, RT_ERR_STATE, "aux buffers are per work-item: not together with a supersampling factor > 1");
    c->aux_t = static_cast<float*>(d_hit_t);
    c->aux_index = static_cast<int32_t*>(d_hit_index);
    return RT_OK;
}

int rt_render_device(rt_context* c, void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!d_out && c->n_local) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out is NULL");
    // NULL is the legacy default stream - NOT the context's private stream: a caller that passes its framework's
    // "current stream" handle (0 for torch's default stream) gets a render that is ordered with its own work
    if (c->ss > 1) {  // samples into the context's sample frame, their pixels into d_out, on the caller's stream
        if (c->n_local == 0) return RT_OK;
        if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "a float4 d_out must be 16-byte aligned");
        RT_DEVICE(c);
        int rc = grow_buffer(c, c->d_samples, c->d_samples_bytes, (size_t)c->n_local * elem_bytes(c), false);
        if (rc == RT_OK) rc = do_launch(c, c->d_samples, static_cast<hipStream_t>(hip_stream), false);
        if (rc == RT_OK) rc = resolve_on(c, c->d_samples, c->n_local, 0, d_out, static_cast<hipStream_t>(hip_stream));
        return rc;
    }
    return do_launch(c, d_out, static_cast<hipStream_t>(hip_stream), false);
}

// The synchronous Render() of a LARGE frame, in passes: the frame is cut into interleaved 16-row tiles as for several GPUs
// (rt_set_shard's partition; a pass stands for consecutive ranks - RenderParams::run_rays), pass 0 renders three tiles of every
// four, pass 1 the fourth, and pass 0's tiles travel to the pinned host frame - one strided device-to-host copy on a stream of its
// own - WHILE pass 1 renders; only the last quarter's copy is left behind the kernels. The blocking read-back of 268 MB
// (OpenCLRaytracer.cpp:94) is 4.9 ms behind an 11.4 ms cfg4 render. Measured, cfg4 (tools/ab/render_split.py,
// profiles/r04_experiments/render_split*.txt): one pass 16.5 ms, "1,1" (round 4's first form) 14.8, "3,1" 13.55, "2,1" 13.9,
// "5,2,1" 13.8, "7,1" 15.1 - an unequal split wins because a small pass renders less efficiently than a large one (a quarter of the
// frame takes 3.5 ms, not 2.85) while the copy it hides is proportional to the pass before it: 3/4 of the copy (3.7 ms) fits behind
// the last quarter's render. Only for frames of the large-scene path with >= 4 M rays that the caller has not sharded himself;
// RT_RENDER_PASSES=1 switches it off, RT_RENDER_SPLIT="a,b,.." chooses another split. The pixels are the one-pass frame's, bit for
// bit (a shard is the same arithmetic on a subset of the rays).
// Float and 8-bit frames share it: `format` 0 is rt_render's float frame (elements of elem_bytes(c), straight from d_out to h_out);
// an rt_pixel_format adds the step after a pass's render - pack that pass's pixels into d_pack on the render stream - and
// what then travels is bytes, from d_pack to h_pack. The tile arithmetic is the same with another element size.
static int render_in_passes(rt_context* c, int format, const void** out) {
    // the split: spans of consecutive ranks of a world of their sum ("3,1": three tiles of every four, then the fourth). A byte
    // frame's copy is a quarter as long, so a smaller last pass pays: "7,1" (cfg4, RGBA8: 12.55 ms against 12.80 for "3,1", 13.22
    // for "1,1", 13.11 in one pass - profiles/packed_output_timing.json); a filtered float frame's copy is as short (wants_passes)
    uint32_t spans[kMaxPasses] = {(format || c->ss > 1) ? 7u : 3u, 1, 0, 0}, K = 2, world = 0;
    if (const char* env = std::getenv("RT_RENDER_SPLIT")) {
        K = 0;
        for (const char* q = env; *q && K < kMaxPasses;) {
            const long v = std::strtol(q, const_cast<char**>(&q), 10);
            if (v <= 0 || v > 64) { K = 0; break; }
            spans[K++] = (uint32_t)v;
            if (*q == ',') ++q;
        }
        if (K == 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "RT_RENDER_SPLIT: up to 4 comma-separated spans of 1..64 tiles");
    }
    for (uint32_t k = 0; k < K; ++k) world += spans[k];
    const uint64_t n_rays = c->n_rays;
    // supersampled frames: a tile holds whole pixel rows (16 sample rows for s = 2 and 4, lcm(16, 3) = 48 for s = 3), a pass filters
    // its samples (from d_samples) into its pixels, and everything behind the filter - pack, copy, host frame - counts in pixels
    const uint32_t ss = c->ss, ss2 = ss * ss;
    const uint64_t tile_rays = sample_width(c) ? (ss == 3 ? 48ull : 16ull) * sample_width(c) : 65536ull;
    const uint64_t tiles = (n_rays + tile_rays - 1) / tile_rays;
    const size_t render_elem = elem_bytes(c);                             // what a kernel writes per work-item
    const size_t elem = format ? packed_bytes(format) : render_elem;     // what travels to the host per pixel
    const size_t tile_bytes = (size_t)(tile_rays / ss2) * elem;
    const size_t frame_bytes = (size_t)tiles * tile_bytes;  // whole tiles: the ragged last one is padded behind the frame's end
    int rc = grow_buffer(c, format ? c->h_pack : c->h_out, format ? c->h_pack_bytes : c->h_out_bytes, frame_bytes, true);
    if (rc == RT_OK && ss > 1) rc = grow_buffer(c, c->d_samples, c->d_samples_bytes, (size_t)tiles * tile_rays * render_elem, false);
    if (rc == RT_OK && (ss == 1 || !format))
        rc = grow_buffer(c, c->d_out, c->d_out_bytes, (size_t)tiles * (tile_rays / ss2) * render_elem, false);  // the passes' outputs one behind the other
    if (rc == RT_OK && format) rc = grow_buffer(c, c->d_pack, c->d_pack_bytes, frame_bytes, false);
    if (rc != RT_OK) return rc;
    char* const d_frame = static_cast<char*>(format ? c->d_pack : c->d_out);  // what the copies read
    char* const h_frame = static_cast<char*>(format ? c->h_pack : c->h_out);
    if (!c->copy_stream) RT_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (uint32_t k = 0; k < K; ++k)
        if (!c->ev_pass[k]) RT_HIP(c, hipEventCreateWithFlags(&c->ev_pass[k], hipEventDisableTiming));
    uint64_t at = 0;      // this pass's first work-item within the device frame(s)
    uint32_t rank = 0;    // its first rank
    const uint64_t groups = tiles / world, rest = tiles % world;
    for (uint32_t k = 0; k < K && rc == RT_OK; rank += spans[k], ++k) {
        c->tile_rays = tile_rays;
        c->rank = rank;
        c->world = world;
        c->span = spans[k];
        c->n_local = local_count(n_rays, tile_rays, rank, world, spans[k]);
        char* const rendered = static_cast<char*>(ss > 1 ? c->d_samples : c->d_out) + (size_t)at * render_elem;
        char* buf = d_frame + (size_t)(at / ss2) * elem;
        const size_t run_bytes = (size_t)spans[k] * tile_bytes;
        at += c->n_local;
        if (c->n_local == 0) continue;
        rc = do_launch(c, rendered, c->stream, false);
        if (rc == RT_OK && ss > 1) rc = resolve_on(c, rendered, c->n_local, format, buf, c->stream);  // the byte forms fused
        else if (rc == RT_OK && format) rc = pack_on(c, rendered, c->n_local, format, buf, c->stream);
        if (rc != RT_OK) break;
        hipError_t e = hipEventRecord(c->ev_pass[k], c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_stream, c->ev_pass[k], 0);
        char* dst = h_frame + (size_t)rank * tile_bytes;
        if (e == hipSuccess && groups)  // run j of this pass is tiles j * world + rank ... of the frame
            e = hipMemcpy2DAsync(dst, (size_t)world * tile_bytes, buf, run_bytes, run_bytes, (size_t)groups, hipMemcpyDeviceToHost, c->copy_stream);
        if (e == hipSuccess && rest > rank)  // the short run of the frame's last, incomplete group of tiles
            e = hipMemcpyAsync(dst + (size_t)groups * world * tile_bytes, buf + (size_t)groups * run_bytes,
                               (size_t)std::min<uint64_t>(rest - rank, spans[k]) * tile_bytes, hipMemcpyDeviceToHost, c->copy_stream);
        if (e != hipSuccess) rc = fail_hip(c, e, "read-back of a pass");
    }
    c->tile_rays = 0;
    c->rank = 0;
    c->world = 1;
    c->span = 1;
    c->n_local = n_rays;
    hipError_t e = hipStreamSynchronize(c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->copy_stream);  // Render() is synchronous (OpenCLRaytracer.cpp:94)
    if (rc != RT_OK) return rc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail_hip(c, e, "hipStreamSynchronize");
    *out = h_frame;
    return RT_OK;
}

// the conditions that send a synchronous render through render_in_passes (float and 8-bit frames alike)
// A supersampled BYTE frame is small enough to go in one pass by default: its copy (a sixteenth of the sample frame's bytes for
// s = 2: 16.7 MB, 0.3 ms) hides less than a second pass's drains cost - cfg4, s = 2, RGBA8: 11.76 ms in one pass against 12.31 for
// "7,1", 12.42 "15,1", 12.44 "3,1", 12.53 "1,1" (profiles/supersample_timing.json). A supersampled FLOAT frame's copy is the byte
// frame's of an unfiltered one, and so is its best split: "7,1" (12.42 against 12.49 "15,1", 12.63 one pass, 12.69 "3,1", 13.04 "1,1").
static bool wants_passes(const rt_context* c, int format = 0) {
    const char* env = std::getenv("RT_RENDER_PASSES");  // "1": one pass whatever the frame; "2": two passes whatever its size (tests)
    const bool off = env && env[0] == '1', forced = env && env[0] == '2';
    const bool large = c->n_rays >= (1ull << 22) && !(c->ss > 1 && format);
    return !off && c->world <= 1 && (forced || large) && c->n_rays > 0 && c->n_local == c->n_rays && use_wavefront(c) &&
           (c->pinhole || c->have_rays) && !c->aux_t && !c->aux_index;  // (aux buffers are indexed by work-item of ONE whole-frame launch)
}

int rt_render(rt_context* c, const float** out) {
    if (!c || !out) return RT_ERR_INVALID_ARGUMENT;
    RT_DEVICE(c);
    if (wants_passes(c)) {
        const void* frame = nullptr;
        const int rc = render_in_passes(c, 0, &frame);
        if (rc == RT_OK) *out = static_cast<const float*>(frame);
        return rc;
    }
    int rc = ensure_out(c);
    if (rc) return rc;
    rc = ensure_host_out(c);
    if (rc) return rc;
    if (c->ss > 1) rc = grow_buffer(c, c->d_samples, c->d_samples_bytes, (size_t)c->n_local * elem_bytes(c), false);
    if (rc) return rc;
    rc = do_launch(c, c->ss > 1 ? c->d_samples : c->d_out, c->stream, false);
    if (rc) return rc;
    if (c->ss > 1) rc = resolve_on(c, c->d_samples, c->n_local, 0, c->d_out, c->stream);
    if (rc) return rc;
    const size_t bytes = (size_t)local_pixels(c) * elem_bytes(c);
    if (bytes) RT_HIP(c, hipMemcpyAsync(c->h_out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));  // Render() is synchronous (OpenCLRaytracer.cpp:94)
    *out = static_cast<const float*>(c->h_out);
    return RT_OK;
}

size_t rt_packed_pixel_bytes(int format) { return packed_bytes(format); }

int rt_pack_device(rt_context* c, const void* d_rgba_f32, uint64_t n_pixels, int format, void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!packed_bytes(format)) return fail(c, RT_ERR_INVALID_ARGUMENT, "unknown pixel format (RT_PIXEL_RGBA8 = 1, RT_PIXEL_RGB8 = 2)");
    if (n_pixels == 0) return RT_OK;
    if (!d_rgba_f32 || !d_out) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_pack_device: NULL frame");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_rgba_f32) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "the float4 frame must be 16-byte aligned");
    RT_DEVICE(c);
    int lane_pixels = 0;  // the measured choice (rt_pack.hip)
    if (const char* env = std::getenv("RT_PACK_LANE_PIXELS")) lane_pixels = env[0] == '1' ? 1 : (env[0] == '4' ? 4 : 0);  // measurement knob (tools/ab/packed_timing.py)
    const hipError_t e = rt::launch_pack(static_cast<const float4*>(d_rgba_f32), n_pixels, format, d_out, static_cast<hipStream_t>(hip_stream), lane_pixels);
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "pack launch");
}

int rt_render_device_packed(rt_context* c, int format, void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    int rc = check_packed(c, format);
    if (rc) return rc;
    if (c->n_local == 0) return RT_OK;
    if (!d_out) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out must be 4-byte aligned");
    RT_DEVICE(c);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);  // NULL: the legacy default stream, as for rt_render_device
    if (c->ss > 1) {  // filter and quantise in one pass over the sample frame
        rc = grow_buffer(c, c->d_samples, c->d_samples_bytes, (size_t)c->n_local * elem_bytes(c), false);
        if (rc == RT_OK) rc = do_launch(c, c->d_samples, stream, false);
        if (rc == RT_OK) rc = resolve_on(c, c->d_samples, c->n_local, format, d_out, stream);
        return rc;
    }
    rc = grow_buffer(c, c->d_scratch, c->d_scratch_bytes, (size_t)c->n_local * elem_bytes(c), false);
    if (rc) return rc;
    rc = do_launch(c, c->d_scratch, stream, false);
    if (rc) return rc;
    return pack_on(c, c->d_scratch, c->n_local, format, d_out, stream);
}

int rt_render_packed(rt_context* c, int format, const uint8_t** out) {
    if (!c || !out) return RT_ERR_INVALID_ARGUMENT;
    int rc = check_packed(c, format);
    if (rc) return rc;
    RT_DEVICE(c);
    if (wants_passes(c, format)) {
        const void* frame = nullptr;
        rc = render_in_passes(c, format, &frame);
        if (rc == RT_OK) *out = static_cast<const uint8_t*>(frame);
        return rc;
    }
    const size_t bytes = (size_t)local_pixels(c) * packed_bytes(format);
    if (c->ss > 1) rc = grow_buffer(c, c->d_samples, c->d_samples_bytes, (size_t)c->n_local * elem_bytes(c), false);
    else rc = ensure_out(c);  // the float frame: the context's own device framebuffer
    if (rc == RT_OK) rc = grow_buffer(c, c->d_pack, c->d_pack_bytes, bytes, false);
    if (rc == RT_OK) rc = grow_buffer(c, c->h_pack, c->h_pack_bytes, bytes, true);
    if (rc) return rc;
    rc = do_launch(c, c->ss > 1 ? c->d_samples : c->d_out, c->stream, false);
    if (rc) return rc;
    if (bytes) {
        if (c->ss > 1) rc = resolve_on(c, c->d_samples, c->n_local, format, c->d_pack, c->stream);  // filter + quantise, fused
        else rc = pack_on(c, c->d_out, c->n_local, format, c->d_pack, c->stream);
        if (rc) return rc;
        RT_HIP(c, hipMemcpyAsync(c->h_pack, c->d_pack, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    RT_HIP(c, hipStreamSynchronize(c->stream));  // synchronous, like rt_render
    *out = static_cast<const uint8_t*>(c->h_pack);
    return RT_OK;
}

int rt_render_aux(rt_context* c, float* hit_t, int32_t* hit_index) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->ss > 1) return fail(c, RT_ERR_STATE, "aux records are per work-item: not together with a supersampling factor > 1");
    int rc = ensure_out(c);
    if (rc) return rc;
    float* d_t = nullptr;
    int32_t* d_i = nullptr;
    const size_t n = (size_t)c->n_local;
    RT_DEVICE(c);
    if (hit_t) RT_HIP(c, hipMalloc((void**)&d_t, n ? n * 4 : 4));
    if (hit_index) {
        hipError_t e = hipMalloc((void**)&d_i, n ? n * 4 : 4);
        if (e != hipSuccess) { if (d_t) (void)hipFree(d_t); return fail_hip(c, e, "hipMalloc aux"); }
    }
    c->aux_t = d_t;
    c->aux_index = d_i;
    rc = do_launch(c, c->d_out, c->stream, false);
    hipError_t e = hipSuccess;
    if (rc == RT_OK) e = hipStreamSynchronize(c->stream);
    if (rc == RT_OK && e == hipSuccess && hit_t && n) e = hipMemcpy(hit_t, d_t, n * 4, hipMemcpyDeviceToHost);
    if (rc == RT_OK && e == hipSuccess && hit_index && n) e = hipMemcpy(hit_index, d_i, n * 4, hipMemcpyDeviceToHost);
    if (d_t) (void)hipFree(d_t);
    if (d_i) (void)hipFree(d_i);
    if (rc) return rc;
    if (e != hipSuccess) return fail_hip(c, e, "aux read-back");
    return RT_OK;
}

int rt_count_rays(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    RT_DEVICE(c);
    int rc = ensure_out(c);
    if (rc) return rc;
    rc = do_launch(c, c->d_out, c->stream, true);
    if (rc) return rc;
    if (c->n_local == 0) return RT_OK;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    RT_HIP(c, hipMemcpy(&c->counters, c->d_counters, sizeof(rt::Counters), hipMemcpyDeviceToHost));
    if (std::getenv("RT_WALK_STATS")) {  // engineering aid: what the grid walk did in the counted frame
        if (c->grid.enabled) std::fprintf(stderr, "[grid] %d x %d x %d cells, edge %g\n", c->grid.nx, c->grid.ny, c->grid.nz, (double)c->grid.cell);
        static const char* names[8] = {"rays", "wave trips", "live lane-trips", "cell fetches", "pre-tests", "exact tests", "exact rounds", "hand-out rounds"};
        for (int k = 0; k < 2; ++k) {
            const unsigned long long* v = c->counters.walk[k];
            if (!v[0]) continue;
            std::fprintf(stderr, "[walk %s]", k ? "any" : "closest");
            for (int j = 0; j < 8; ++j) std::fprintf(stderr, " %s %llu", names[j], v[j]);
            std::fprintf(stderr, " | per ray: fetches %.2f pre-tests %.2f exact %.2f lane-trips %.2f | live lanes/trip %.1f\n",
                         (double)v[3] / v[0], (double)v[4] / v[0], (double)v[5] / v[0], (double)v[2] / v[0], (double)v[2] / (v[1] ? v[1] : 1));
        }
    }
    return RT_OK;
}

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
    s->local_rays = c->n_local;
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
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->d_pack) (void)hipFree(c->d_pack);
    if (c->h_pack) (void)hipHostFree(c->h_pack);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->d_samples) (void)hipFree(c->d_samples);
    if (c->d_scan) (void)hipFree(c->d_scan);
    if (c->h_scan) (void)hipHostFree(c->h_scan);
    if (c->d_patch_stage) (void)hipFree(c->d_patch_stage);
    if (c->query_made) (void)hipEventSynchronize(c->ev_query[1]);  // (a device-form query may still run on the caller's stream)
    if (c->d_query_counters) (void)hipFree(c->d_query_counters);
    for (hipEvent_t ev : c->ev_query) if (ev) (void)hipEventDestroy(ev);
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
