// rt_render.cpp - the launch and everything that produces a frame: do_launch (one shard of the context's rays through the kernels),
// the pipeline behind every render entry point (render_pixels: trace, then at most one pass that filters or quantises),
// rt_render's large frames in passes, and the render / pack / resolve / aux / count entry points of include/hip_raytracer.h.
#include "rt_context.h"

namespace rt::host {

uint64_t local_count(uint64_t n_rays, uint64_t tile_rays, uint32_t rank, uint32_t world, uint32_t span) {
    if (world <= 1) return n_rays;
    const uint64_t tiles = (n_rays + tile_rays - 1) / tile_rays, rest = tiles % world;
    // tiles of the frame that ranks rank .. rank + span - 1 of `world` own (tile t belongs to rank t % world)
    const uint64_t mine = (tiles / world) * span + (rest > rank ? std::min<uint64_t>(rest - rank, span) : 0);
    return mine * tile_rays;  // the last tile may be ragged: its padding work-items write background
}

bool use_wavefront(const rt_context* c) {
    if (c->has_triangles) return true;
    if (c->flags & RT_FLAG_WAVEFRONT) return true;
    if (c->flags & RT_FLAG_MONOLITHIC) return false;
    if (c->n_objs >= kWavefrontMinObjects) return true;
    return c->n_objs >= kWavefrontGridMinObjects && grid_in_use(c) && !(c->flags & RT_FLAG_LITERAL);
}

void free_wavefront(rt_context* c) {
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

static int ensure_wavefront(rt_context* c, const Shard& sh) {
    rt::WavefrontBuffers& b = c->wf;
    if (b.capacity >= sh.n_local && b.state) return RT_OK;
    free_wavefront(c);
    const uint64_t n = sh.n_local ? sh.n_local : 1;
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

// One launch: the work-items of shard `sh` of the context's rays into d_out. The shard is an argument - the context's own
// (rt_set_shard) or one pass of render_in_passes - and nothing here, nor settle_outside_pose and refresh_screen_tiles below it,
// reads the context's. So are the kernel number, the aux pair and the event pair around the kernels: a frame passes the context's
// (launch_frame), the G-buffer pass RT_KERNEL_HITTEST with arrays and events of its own. sh.n_local > 0.
static int do_launch(rt_context* c, const Shard& sh, int kernel, void* d_out, float* aux_t, int32_t* aux_index, hipEvent_t ev_begin,
                     hipEvent_t ev_end, hipStream_t stream, bool count) {
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
    p.n_local = sh.n_local;
    p.tile_rays = sh.tile_rays ? sh.tile_rays : 1;
    p.run_rays = p.tile_rays * sh.span;
    p.rank = sh.rank;
    p.world = sh.world;
    p.pinhole = c->pinhole ? 1u : 0u;
    p.width = c->width ? c->width : 1;
    p.half_w = (float)c->width / 2.0f;
    p.half_h = (float)c->height / 2.0f;
    p.height_f = (float)c->height;
    p.z = c->z;
    p.dir_w_zero = (c->pinhole || c->dir_w_zero) ? 1u : 0u;
    // 2-D pixel bundles need the grid shape (pinhole mode) and shard tiles made of whole 8-row bands
    const bool row_tiles = sh.world <= 1 || (c->width && sh.tile_rays % c->width == 0 && (sh.tile_rays / c->width) % 8 == 0);
    if (c->pinhole && row_tiles && sh.n_local % c->width == 0 && sh.n_local < 0x7fffffffull) {
        p.tile2d = 1u;
        p.bundles_x = (c->width + 7u) / 8u;
        p.local_rows = (uint32_t)(sh.n_local / c->width);
        p.tile_rows = sh.world > 1 ? (uint32_t)(sh.tile_rays / c->width) : p.local_rows;
        if (p.tile_rows == 0) p.tile_rows = 1;
        p.n_bundles = p.bundles_x * ((p.local_rows + 7u) / 8u);
        p.wf_tile_order = (c->width % 8u == 0 && p.local_rows % 8u == 0) ? 1u : 0u;
        p.tile_cull = (c->n_objs > 0 && c->n_objs <= 64 && c->z < 0.0f && !(c->flags & RT_FLAG_LITERAL)) ? 1u : 0u;
    } else {
        if (sh.n_local > 0xffffffffull - 64) return fail(c, RT_ERR_INVALID_ARGUMENT, "too many rays for one launch");
        p.n_bundles = (uint32_t)((sh.n_local + 63u) / 64u);
    }
    p.max_bounces = c->max_bounces;
    p.out = d_out;
    p.aux_t = aux_t;
    p.aux_index = aux_index;
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
    p.scene.diagonal = c->last_wavefront ? compact_in_use(c) : 0u;  // (the round machine's kernels alone read the compact records)
    if (c->last_wavefront) {  // one-time host-side set-up (buffers, per-camera screen tiles) stays outside the timed region
        StopWatch sw;
        const bool had_buffers = c->wf.capacity >= sh.n_local && c->wf.state;
        int rc = ensure_wavefront(c, sh);
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
    RT_HIP(c, hipEventRecord(ev_begin, stream));
    hipError_t e;
    const int arith = (c->flags & RT_FLAG_DEVICE_OPENCL) ? rt::kDeviceCL : ((c->flags & RT_FLAG_UNFUSED) ? rt::kUnfused : rt::kFused);
    if (c->last_wavefront) e = rt::launch_wavefront(p, kernel, arith, count, c->wf, stream, &c->last_rounds);
    else e = rt::launch_render(p, kernel, arith, count, stream);
    if (e != hipSuccess) return fail_hip(c, e, "kernel launch");
    RT_HIP(c, hipEventRecord(ev_end, stream));
    return RT_OK;
}

// A frame's launch: the context's kernel, its pending aux pair and the next timing slot.
static int launch_frame(rt_context* c, const Shard& sh, void* d_out, hipStream_t stream, bool count) {
    if (sh.n_local == 0) {  // empty launch: nothing to render, nothing to time
        if (count) c->counters = rt::Counters{};
        c->aux_t = nullptr;
        c->aux_index = nullptr;
        return RT_OK;
    }
    const uint32_t slot = c->ev_count % kTimingSlots;
    const int rc = do_launch(c, sh, c->kernel, d_out, c->aux_t, c->aux_index, c->ev_begin[slot], c->ev_end[slot], stream, count);
    if (rc) return rc;
    c->ev_count += 1;
    // aux buffers apply to one render only
    c->aux_t = nullptr;
    c->aux_index = nullptr;
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

// s x s samples -> one pixel: `n_samples` consecutive samples of whole sample rows of the context's camera (a shard's tiles are that)
static int resolve_on(rt_context* c, const void* d_src, uint64_t n_samples, int format, void* d_dst, hipStream_t stream) {
    const hipError_t e = rt::launch_resolve(static_cast<const float4*>(d_src), sample_width(c), (uint32_t)(n_samples / sample_width(c)), c->ss, format, d_dst, stream);
    return e == hipSuccess ? RT_OK : fail_hip(c, e, "resolve launch");
}

// The pipeline behind every render entry point and every pass: shard `sh`'s pixels into d_dst, in `format` (0: the kernels' floats),
// on `stream`. The only place that chooses the route: with a supersampling factor the samples are traced into d_stage and one pass
// filters them - and quantises, for a byte format - into d_dst; without one a byte format is traced into d_stage and packed into
// d_dst, and floats are traced straight into d_dst (d_stage is not looked at).
static int render_pixels(rt_context* c, const Shard& sh, void* d_stage, int format, void* d_dst, hipStream_t stream) {
    const bool staged = c->ss > 1 || format;
    const int rc = launch_frame(c, sh, staged ? d_stage : d_dst, stream, false);
    if (rc || !staged || sh.n_local == 0) return rc;
    return c->ss > 1 ? resolve_on(c, d_stage, sh.n_local, format, d_dst, stream) : pack_on(c, d_stage, sh.n_local, format, d_dst, stream);
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
// Float and 8-bit frames share it: `format` 0 is rt_render's float frame (elements of elem_bytes(c), from d_out to h_out); an
// rt_pixel_format makes a pass's pixels bytes in d_pack, and what then travels is bytes, from d_pack to h_pack. The tile arithmetic
// is the same with another element size. Every pass is a Shard of its own: the context's is not touched.
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
    Buffer& d_pixels = format ? c->d_pack : c->d_out;  // what the copies read
    Buffer& h_pixels = format ? c->h_pack : c->h_out;
    Buffer& d_traced = ss > 1 ? c->d_samples : c->d_out;
    int rc = h_pixels.grow(c, frame_bytes);
    if (rc == RT_OK && ss > 1) rc = c->d_samples.grow(c, (size_t)tiles * tile_rays * render_elem);
    if (rc == RT_OK && (ss == 1 || !format))
        rc = c->d_out.grow(c, (size_t)tiles * (tile_rays / ss2) * render_elem);  // the passes' outputs one behind the other
    if (rc == RT_OK && format) rc = c->d_pack.grow(c, frame_bytes);
    if (rc != RT_OK) return rc;
    char* const d_frame = static_cast<char*>(d_pixels.p);
    char* const h_frame = static_cast<char*>(h_pixels.p);
    if (!c->copy_stream) RT_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (uint32_t k = 0; k < K; ++k)
        if (!c->ev_pass[k]) RT_HIP(c, hipEventCreateWithFlags(&c->ev_pass[k], hipEventDisableTiming));
    uint64_t at = 0;      // this pass's first work-item within the device frame(s)
    uint32_t rank = 0;    // its first rank
    const uint64_t groups = tiles / world, rest = tiles % world;
    for (uint32_t k = 0; k < K && rc == RT_OK; rank += spans[k], ++k) {
        const Shard pass{tile_rays, rank, world, spans[k], local_count(n_rays, tile_rays, rank, world, spans[k])};
        char* const traced = static_cast<char*>(d_traced.p) + (size_t)at * render_elem;
        char* buf = d_frame + (size_t)(at / ss2) * elem;
        const size_t run_bytes = (size_t)spans[k] * tile_bytes;
        at += pass.n_local;
        if (pass.n_local == 0) continue;
        rc = render_pixels(c, pass, traced, format, buf, c->stream);
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
static bool wants_passes(const rt_context* c, int format) {
    const char* env = std::getenv("RT_RENDER_PASSES");  // "1": one pass whatever the frame; "2": two passes whatever its size (tests)
    const bool off = env && env[0] == '1', forced = env && env[0] == '2';
    const bool large = c->n_rays >= (1ull << 22) && !(c->ss > 1 && format);
    return !off && c->shard.world <= 1 && (forced || large) && c->n_rays > 0 && c->shard.n_local == c->n_rays && use_wavefront(c) &&
           (c->pinhole || c->have_rays) && !c->aux_t && !c->aux_index;  // (aux buffers are indexed by work-item of ONE whole-frame launch)
}

// What rt_render (format 0: d_out -> h_out) and rt_render_packed (d_pack -> h_pack) do once their refusals are made: the frame of
// the context's shard in the pinned host buffer of the format, on the context's stream(s), drained. Floats without a factor are
// traced into d_out itself; everything else is staged - samples in d_samples, floats to quantise in d_out.
static int render_to_host(rt_context* c, int format, const void** out) {
    RT_DEVICE(c);
    if (wants_passes(c, format)) return render_in_passes(c, format, out);
    Buffer& d_pixels = format ? c->d_pack : c->d_out;
    Buffer& h_pixels = format ? c->h_pack : c->h_out;
    Buffer& d_stage = c->ss > 1 ? c->d_samples : c->d_out;
    const size_t traced = (size_t)c->shard.n_local * elem_bytes(c);
    const size_t bytes = (size_t)local_pixels(c) * (format ? packed_bytes(format) : elem_bytes(c));
    int rc = d_stage.grow(c, traced);
    if (rc == RT_OK) rc = d_pixels.grow(c, format ? bytes : traced);
    if (rc == RT_OK) rc = h_pixels.grow(c, format ? bytes : traced);
    if (rc == RT_OK) rc = render_pixels(c, c->shard, d_stage.p, format, d_pixels.p, c->stream);
    if (rc) return rc;
    if (bytes) RT_HIP(c, hipMemcpyAsync(h_pixels.p, d_pixels.p, bytes, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));  // Render() is synchronous (OpenCLRaytracer.cpp:94)
    *out = h_pixels.p;
    return RT_OK;
}

// ---- G-buffer frames (hip_raytracer.h) -----------------------------------------------------------------------------------------------
static int check_gbuffer(rt_context* c, const rt_gbuffer_t* o, bool device) {
    const rt_gbuffer_t m = o ? *o : rt_gbuffer_t{};
    return check_outputs(c, o, {{m.t, 4}, {m.index, 4}, {m.point, 16}, {m.normal, 16}, {m.albedo, 16}}, device,
                         "t and index must be 4-byte aligned", "point, normal and albedo must be 16-byte aligned");
}

// One pass over the context's shard on `stream`; the members of `o` are device pointers (each may be null). The primary round of the
// frame pipeline as a hittest frame - t is its aux_t (the loop's value, a NaN included), index its aux_index; the frame's own float
// goes to a buffer of the pass's own that nobody reads - then the record kernel behind it on the same stream. Nothing of the frame's state is left changed: the pending
// aux pair, the timing slots and the route rt_get_stats reports stay the renders'. c->shard.n_local > 0.
static int enqueue_gbuffer(rt_context* c, const rt_gbuffer_t& o, hipStream_t stream) {
    const Shard& sh = c->shard;
    const size_t n = (size_t)sh.n_local;
    if (const int rc = ensure_counted(c, c->gb_records)) return rc;
    for (hipEvent_t& e : c->ev_gb_trace)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    float* d_t = o.t;
    int32_t* d_index = o.index;
    c->gb_records.made = false;  // until this pass is enqueued whole: rt_get_gbuffer_info never pairs events of two passes
    int rc = c->d_gb_out.grow(c, n * sizeof(float));
    if (rc == RT_OK && !d_t) rc = c->d_gb_t.grow(c, n * sizeof(float));
    if (rc == RT_OK && !d_index) rc = c->d_gb_index.grow(c, n * sizeof(int32_t));
    if (rc) return rc;
    if (!d_t) d_t = static_cast<float*>(c->d_gb_t.p);
    if (!d_index) d_index = static_cast<int32_t*>(c->d_gb_index.p);
    const bool frame_wavefront = c->last_wavefront;
    const uint32_t frame_rounds = c->last_rounds;
    rc = do_launch(c, sh, RT_KERNEL_HITTEST, c->d_gb_out.p, d_t, d_index, c->ev_gb_trace[0], c->ev_gb_trace[1], stream, false);
    c->gb_wavefront = c->last_wavefront;
    c->last_wavefront = frame_wavefront;
    c->last_rounds = frame_rounds;
    if (rc) return rc;
    rc = enqueue_counted(c, c->gb_records, stream, "G-buffer record launch", [&] {
        const rt::GBufferShard shard{c->n_rays, sh.n_local, sh.tile_rays ? sh.tile_rays : 1, sh.rank, sh.world};
        const rt::GBufferRecords rec{d_t, d_index, reinterpret_cast<float4*>(o.point), reinterpret_cast<float4*>(o.normal),
                                     reinterpret_cast<float4*>(o.albedo)};
        return rt::launch_gbuffer_records(query_scene(c), query_camera(c), shard, query_arith(c), rec,
                                          static_cast<unsigned long long*>(c->gb_records.d_counters), stream);
    });
    if (rc) return rc;
    c->gb_items = sh.n_local;
    return RT_OK;
}

}  // namespace rt::host

using namespace rt::host;

extern "C" {

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

// NULL is the legacy default stream - NOT the context's private stream: a caller that passes its framework's
// "current stream" handle (0 for torch's default stream) gets a render that is ordered with its own work.
// With a factor: samples into the context's sample frame, their pixels into d_out, on the caller's stream.
int rt_render_device(rt_context* c, void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!d_out && c->shard.n_local) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (c->ss > 1) {
        if (c->shard.n_local == 0) return RT_OK;
        if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(c, RT_ERR_INVALID_ARGUMENT, "a float4 d_out must be 16-byte aligned");
    }
    RT_DEVICE(c);
    const int rc = c->ss > 1 ? c->d_samples.grow(c, (size_t)c->shard.n_local * elem_bytes(c)) : RT_OK;
    if (rc) return rc;
    return render_pixels(c, c->shard, c->d_samples.p, 0, d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_render(rt_context* c, const float** out) {
    if (!c || !out) return RT_ERR_INVALID_ARGUMENT;
    const void* frame = nullptr;
    const int rc = render_to_host(c, 0, &frame);
    if (rc == RT_OK) *out = static_cast<const float*>(frame);
    return rc;
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

// the float frame is staged in d_scratch (d_out stays rt_render's), the samples of a factor > 1 in d_samples
int rt_render_device_packed(rt_context* c, int format, void* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    int rc = check_packed(c, format);
    if (rc) return rc;
    if (c->shard.n_local == 0) return RT_OK;
    if (!d_out) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "d_out must be 4-byte aligned");
    RT_DEVICE(c);
    Buffer& d_stage = c->ss > 1 ? c->d_samples : c->d_scratch;
    rc = d_stage.grow(c, (size_t)c->shard.n_local * elem_bytes(c));
    if (rc) return rc;
    return render_pixels(c, c->shard, d_stage.p, format, d_out, static_cast<hipStream_t>(hip_stream));  // NULL: the legacy default stream, as for rt_render_device
}

int rt_render_packed(rt_context* c, int format, const uint8_t** out) {
    if (!c || !out) return RT_ERR_INVALID_ARGUMENT;
    const int refused = check_packed(c, format);
    if (refused) return refused;
    const void* frame = nullptr;
    const int rc = render_to_host(c, format, &frame);
    if (rc == RT_OK) *out = static_cast<const uint8_t*>(frame);
    return rc;
}

int rt_render_aux(rt_context* c, float* hit_t, int32_t* hit_index) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->ss > 1) return fail(c, RT_ERR_STATE, "aux records are per work-item: not together with a supersampling factor > 1");
    RT_DEVICE(c);
    int rc = c->d_out.grow(c, (size_t)c->shard.n_local * elem_bytes(c));
    if (rc) return rc;
    float* d_t = nullptr;
    int32_t* d_i = nullptr;
    const size_t n = (size_t)c->shard.n_local;
    if (hit_t) RT_HIP(c, hipMalloc((void**)&d_t, n ? n * 4 : 4));
    if (hit_index) {
        hipError_t e = hipMalloc((void**)&d_i, n ? n * 4 : 4);
        if (e != hipSuccess) { if (d_t) (void)hipFree(d_t); return fail_hip(c, e, "hipMalloc aux"); }
    }
    c->aux_t = d_t;
    c->aux_index = d_i;
    rc = launch_frame(c, c->shard, c->d_out.p, c->stream, false);
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
    int rc = c->d_out.grow(c, (size_t)c->shard.n_local * elem_bytes(c));
    if (rc) return rc;
    rc = launch_frame(c, c->shard, c->d_out.p, c->stream, true);
    if (rc) return rc;
    if (c->shard.n_local == 0) return RT_OK;
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

// NULL is the legacy default stream, as for rt_render_device
int rt_render_gbuffer_device(rt_context* c, const rt_gbuffer_t* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_gbuffer(c, d_out, true)) return rc;
    if (c->shard.n_local == 0) return RT_OK;
    if (const int rc = refuse_no_primary_rays(c)) return rc;
    RT_DEVICE(c);
    return enqueue_gbuffer(c, *d_out, static_cast<hipStream_t>(hip_stream));
}

// the host twin: every requested member staged in a context-owned buffer, on the context's stream; synchronous
int rt_render_gbuffer(rt_context* c, const rt_gbuffer_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = check_gbuffer(c, out, false)) return rc;
    if (c->shard.n_local == 0) return RT_OK;
    if (const int rc = refuse_no_primary_rays(c)) return rc;
    RT_DEVICE(c);
    const size_t n = (size_t)c->shard.n_local;
    const struct {
        void* host;
        Buffer& buffer;
        size_t bytes;
    } members[] = {{out->t, c->d_gb_t, n * sizeof(float)}, {out->index, c->d_gb_index, n * sizeof(int32_t)}, {out->point, c->d_gb_point, n * 16},
                   {out->normal, c->d_gb_normal, n * 16}, {out->albedo, c->d_gb_albedo, n * 16}};
    void* d[5] = {};
    CopyBack back;
    for (int k = 0; k < 5; ++k) {
        if (!members[k].host) continue;
        if (const int rc = members[k].buffer.grow(c, members[k].bytes)) return rc;
        d[k] = back.select<void>(members[k].host, members[k].buffer.p, members[k].bytes);
    }
    const rt_gbuffer_t device{static_cast<float*>(d[0]), static_cast<int32_t*>(d[1]), static_cast<float*>(d[2]), static_cast<float*>(d[3]),
                              static_cast<float*>(d[4])};
    if (const int rc = enqueue_gbuffer(c, device, c->stream)) return rc;
    return back.finish(c, c->stream);
}

int rt_get_gbuffer_info(rt_context* c, rt_gbuffer_info_t* info) {
    if (!c || !info) return RT_ERR_INVALID_ARGUMENT;
    if (!c->gb_records.made) return fail(c, RT_ERR_STATE, "rt_get_gbuffer_info: no G-buffer pass has been made on this context");
    RT_DEVICE(c);
    unsigned long long hits = 0;
    if (const int rc = read_counted(c, c->gb_records, &hits, &info->records_ms)) return rc;  // (waits for the record kernel)
    float trace = 0.f;
    RT_HIP(c, hipEventElapsedTime(&trace, c->ev_gb_trace[0], c->ev_gb_trace[1]));
    info->n_items = c->gb_items;
    info->hits = hits;
    info->trace_ms = (double)trace;
    info->wavefront = c->gb_wavefront ? 1u : 0u;
    info->reserved = 0;
    return RT_OK;
}

// ---- ambient-occlusion frames (hip_raytracer.h): the G-buffer pass into context-owned staging, then the AO kernel on the same stream ----
// Every pointer of d_params / d_out is device memory; the refusals are made. c->shard.n_local > 0. `between`: an event of the caller's
// recorded between the two passes (null: none).
static int enqueue_ao_frame(rt_context* c, const rt_ao_params_t& d_params, const rt_ao_t& d_out, hipStream_t stream, hipEvent_t between = nullptr) {
    const Shard& sh = c->shard;
    const size_t n = (size_t)sh.n_local;
    for (hipEvent_t& e : c->ev_ao_gbuffer)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    if (const int rc = ensure_counted(c, c->ao)) return rc;
    int rc = c->d_gb_index.grow(c, n * sizeof(int32_t));
    if (rc == RT_OK) rc = c->d_gb_point.grow(c, n * 16);
    if (rc == RT_OK) rc = c->d_gb_normal.grow(c, n * 16);
    if (rc) return rc;
    c->ao.made = false;  // until this pass is enqueued whole: rt_get_ao_info never pairs events of two passes
    c->ao_frame = true;
    const rt_gbuffer_t records{nullptr, static_cast<int32_t*>(c->d_gb_index.p), static_cast<float*>(c->d_gb_point.p),
                               static_cast<float*>(c->d_gb_normal.p), nullptr};
    RT_HIP(c, hipEventRecord(c->ev_ao_gbuffer[0], stream));
    if ((rc = enqueue_gbuffer(c, records, stream))) return rc;
    RT_HIP(c, hipEventRecord(c->ev_ao_gbuffer[1], stream));
    if (between) RT_HIP(c, hipEventRecord(between, stream));
    const rt::GBufferShard shard{c->n_rays, sh.n_local, sh.tile_rays ? sh.tile_rays : 1, sh.rank, sh.world};
    return enqueue_ao(c, shard, records.point, records.normal, records.index, d_params, d_out, stream);
}

// what both frame forms refuse, in this order; then an empty shard is RT_OK (`empty`) before the primary rays are asked for
static int check_ao_frame(rt_context* c, const rt_ao_params_t* params, const rt_ao_t* out, bool device, bool& empty) {
    if (const int rc = check_ao(c, params, out, device)) return rc;
    if (const int rc = refuse_ao_context(c)) return rc;
    empty = c->shard.n_local == 0;
    return empty ? RT_OK : refuse_no_primary_rays(c);
}

// NULL is the legacy default stream, as for rt_render_gbuffer_device
int rt_render_ao_device(rt_context* c, const rt_ao_params_t* params, const rt_ao_t* d_out, void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    bool empty = false;
    if (const int rc = check_ao_frame(c, params, d_out, true, empty)) return rc;
    if (empty) return RT_OK;
    RT_DEVICE(c);
    return enqueue_ao_frame(c, *params, *d_out, static_cast<hipStream_t>(hip_stream));
}

// the host twin: table and results staged in the patch buffer, on the context's stream; synchronous
int rt_render_ao(rt_context* c, const rt_ao_params_t* params, const rt_ao_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    bool empty = false;
    if (const int rc = check_ao_frame(c, params, out, false, empty)) return rc;
    if (empty) return RT_OK;
    RT_DEVICE(c);
    rt_ao_params_t d_params;
    rt_ao_t d_out;
    CopyBack back;
    char* unused = nullptr;
    if (const int rc = stage_ao_host(c, *params, *out, c->shard.n_local, 0, c->stream, d_params, d_out, back, unused)) return rc;
    if (const int rc = enqueue_ao_frame(c, d_params, d_out, c->stream)) return rc;
    return back.finish(c, c->stream);
}

// ---- filtered ambient occlusion (hip_raytracer.h): rt_render_ao_device's two passes with the counts in d_ao_counts, then the filter ------
// The staged index, point and normal, and the counts, are what the filter reads; width: the sample grid's. Refusals are made.
static int enqueue_ao_filtered_frame(rt_context* c, const rt_ao_params_t& d_params, const rt_ao_filter_params_t& filter,
                                     const rt_ao_filtered_t& d_out, hipStream_t stream) {
    const uint64_t n = c->shard.n_local, width = sample_width(c);
    if (const int rc = ensure_counted(c, c->ao_filter)) return rc;
    for (hipEvent_t& e : c->ev_ao_filter_frame)
        if (!e) RT_HIP(c, hipEventCreate(&e));
    if (const int rc = c->d_ao_counts.grow(c, (size_t)n)) return rc;
    c->ao_filter.made = false;  // until this pass is enqueued whole, as enqueue_ao_frame has it
    c->ao_filter_frame = true;
    uint8_t* const counts = static_cast<uint8_t*>(c->d_ao_counts.p);
    // marks of this form's own around its two internal passes: a later rt_render_ao* re-records the AO family's events, not these
    RT_HIP(c, hipEventRecord(c->ev_ao_filter_frame[0], stream));
    if (const int rc = enqueue_ao_frame(c, d_params, rt_ao_t{counts, nullptr}, stream, c->ev_ao_filter_frame[1])) return rc;
    RT_HIP(c, hipEventRecord(c->ev_ao_filter_frame[2], stream));
    return enqueue_ao_filter(c, counts, static_cast<const float*>(c->d_gb_point.p), static_cast<const float*>(c->d_gb_normal.p),
                             static_cast<const int32_t*>(c->d_gb_index.p), width, n / width, d_params.samples, filter, d_out, stream);
}

// what both frame forms refuse, in this order; then an empty frame is RT_OK (`empty`)
static int check_ao_filtered_frame(rt_context* c, const rt_ao_params_t* params, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out,
                                   bool device, bool& empty) {
    if (!params) return fail(c, RT_ERR_INVALID_ARGUMENT, "the parameter struct is NULL");
    if (const int rc = check_ao_filter(c, filter, out, params->samples, device)) return rc;
    uint8_t counts_stand_in = 0;  // the AO pass's output is the context's own count buffer
    const rt_ao_t counts{&counts_stand_in, nullptr};
    if (const int rc = check_ao(c, params, &counts, device)) return rc;
    if (const int rc = refuse_ao_context(c)) return rc;
    if (c->shard.world > 1)
        return fail(c, RT_ERR_STATE, "filtered ambient occlusion on a sharded context: a tile's neighbours live on other shards");
    empty = c->shard.n_local == 0;
    if (empty) return RT_OK;
    if (const int rc = refuse_no_primary_rays(c)) return rc;
    if (!has_sample_grid(c) || sample_width(c) == 0 || c->shard.n_local % sample_width(c))
        return fail(c, RT_ERR_STATE, "filtered ambient occlusion needs a sample grid: the primary rays come from a plain ray buffer, which has no width");
    return RT_OK;
}

int rt_render_ao_filtered_device(rt_context* c, const rt_ao_params_t* params, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* d_out,
                                 void* hip_stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    bool empty = false;
    if (const int rc = check_ao_filtered_frame(c, params, filter, d_out, true, empty)) return rc;
    if (empty) return RT_OK;
    RT_DEVICE(c);
    return enqueue_ao_filtered_frame(c, *params, *filter, *d_out, static_cast<hipStream_t>(hip_stream));
}

// the host twin: table and results staged in the patch buffer, on the context's stream; synchronous
int rt_render_ao_filtered(rt_context* c, const rt_ao_params_t* params, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    bool empty = false;
    if (const int rc = check_ao_filtered_frame(c, params, filter, out, false, empty)) return rc;
    if (empty) return RT_OK;
    RT_DEVICE(c);
    const uint64_t n = c->shard.n_local;
    const size_t dirs_bytes = (size_t)params->n_sets * params->samples * 16u;
    if (const int rc = ensure_patch_stage(c, dirs_bytes + ao_filter_output_bytes(n))) return rc;
    char* const base = static_cast<char*>(c->d_patch_stage.p);
    RT_HIP(c, hipMemcpyAsync(base, params->dirs, dirs_bytes, hipMemcpyHostToDevice, c->stream));
    rt_ao_params_t d_params = *params;
    d_params.dirs = base;
    rt_ao_filtered_t d_out;
    CopyBack back;
    stage_ao_filter_outputs(base, dirs_bytes, *out, n, d_out, back);
    if (const int rc = enqueue_ao_filtered_frame(c, d_params, *filter, d_out, c->stream)) return rc;
    return back.finish(c, c->stream);
}

}  // extern "C"
