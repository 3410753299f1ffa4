// rt_context.h - internal to the C-ABI layer (not installed): struct rt_context and what the host units share - rt_api.cpp (life
// cycle, rays / camera / pose, the setters and readers), rt_render.cpp (do_launch, the frame pipeline, the render entry points),
// rt_scene.cpp (re-pack, bounds, grid, walk blocks), rt_camera_tiles.cpp (screen tiles), rt_light_setup.cpp (light tiles),
// rt_object_patch.cpp (what the calls that patch a range of objects share; replaceable materials), rt_geometry.cpp (replaceable
// transforms), rt_visibility_host.cpp (replaceable visibility), rt_query_host.cpp (ray queries) and rt_multi.cpp (several GPUs). Everything with external linkage here
// lives in rt::host, apart from the launchers in rt::.
#pragma once
#include "hip_raytracer.h"
#include "rt_records.h"
#include "rt_kernels.h"
#include "rt_pack.h"
#include "rt_resolve.h"
#include "rt_rays.h"
#include "rt_raygen.h"
#include "rt_tiles.h"
#include "rt_grid_radii.h"
#include "rt_light_tiles.h"
#include "rt_materials.h"
#include "rt_transforms.h"
#include "rt_visibility.h"
#include "rt_query.h"
#include "rt_gbuffer.h"
#include "rt_ao.h"
#include "rt_ao_filter.h"
#include "rt_compact.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <new>
#include <string>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace rt::host {

struct StopWatch {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap_ms() {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

// engineering aid (RT_SETUP_TRACE=1): where the one-time host work goes, lap by lap, on stderr
struct SetupTrace {
    const char* who;
    bool on = std::getenv("RT_SETUP_TRACE") != nullptr;
    StopWatch sw;
    explicit SetupTrace(const char* w) : who(w) {}
    void operator()(const char* what) { if (on) std::fprintf(stderr, "[%s] %-28s %8.2f ms\n", who, what, sw.lap_ms()); }
};

// One-time host work over independent items (per-tile sorts, per-tile block chains, ...) on several threads: f(begin, end) over
// [0, n) in contiguous chunks, the calling thread taking the first one. RT_SETUP_THREADS=1 keeps it serial; the results do not
// depend on the number of threads (every item writes its own outputs).
template <class F>
void parallel_for(size_t n, size_t grain, F&& f) {
    size_t threads = std::thread::hardware_concurrency();
    if (threads == 0) threads = 1;
    threads = std::min<size_t>(threads, 16);
    if (const char* env = std::getenv("RT_SETUP_THREADS")) threads = (size_t)std::max(1, std::atoi(env));
    threads = std::min(threads, n / std::max<size_t>(grain, 1));
    if (threads <= 1) { if (n) f((size_t)0, n); return; }
    const size_t chunk = (n + threads - 1) / threads;
    std::vector<std::thread> pool;
    pool.reserve(threads - 1);
    for (size_t t = 1; t < threads; ++t) {
        const size_t lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
        if (lo == hi) continue;
        try { pool.emplace_back([&f, lo, hi] { f(lo, hi); }); }
        catch (...) { f(lo, hi); }  // (no thread to be had: this chunk on the calling thread)
    }
    f((size_t)0, std::min(n, chunk));
    for (std::thread& th : pool) th.join();
}

constexpr uint32_t kTimingSlots = 256;
constexpr uint32_t kMaxPasses = 4;  // of rt_render's frame (render_in_passes)

// Path choice unless a flag says otherwise. Measured at 2048^2 (scratch sweep, depth 3, 4 lights): the small-scene
// kernel wins up to 64 objects (per-bundle culling), the wavefront path with the grid from ~100 objects on
// (N=128: 1.4 vs 0.9 ms, N=512: 7.4 vs 1.3 ms). Without a usable grid the wavefront path only pays once the
// traversal loop dwarfs its per-round state traffic.
constexpr uint32_t kWavefrontMinObjects = 512;      // brute-force wavefront
constexpr uint32_t kWavefrontGridMinObjects = 96;   // wavefront when the conservative grid is available

// The work-items one launch renders: tiles of `tile_rays` rays dealt round-robin to `world` ranks, of which this launch stands for
// ranks rank .. rank + span - 1. The context's own is what rt_set_shard set (span 1); a pass of render_in_passes makes its own.
struct Shard {
    uint64_t tile_rays = 0;
    uint32_t rank = 0, world = 1, span = 1;
    uint64_t n_local = 0;
};

// a context-owned buffer that only ever grows: device memory, or pinned host memory (rt_api.cpp)
int grow_buffer(rt_context* c, void*& p, size_t& have, size_t need, bool pinned_host);
// One such buffer that knows its kind and frees itself with the context. A failed grow() leaves it empty.
struct Buffer {
    void* p = nullptr;
    size_t bytes = 0;
    const bool pinned_host;
    explicit Buffer(bool pinned = false) : pinned_host(pinned) {}
    ~Buffer() { if (p) (void)(pinned_host ? hipHostFree(p) : hipFree(p)); }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    int grow(rt_context* c, size_t need) { return grow_buffer(c, p, bytes, need, pinned_host); }
};

// What a query family keeps on its context (enqueue_counted and read_counted, below): the counter block its kernels add to,
// the event pair around the last kernel - both made by the family's first call - and whether there has been one.
struct CountedSlot {
    const size_t counter_bytes;
    void* d_counters = nullptr;
    hipEvent_t ev[2] = {};
    bool made = false;
    explicit CountedSlot(size_t bytes) : counter_bytes(bytes) {}
};

}  // namespace rt::host

struct rt_context {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t flags = 0;
    int kernel = 2;
    uint32_t n_objs = 0, n_lights = 0, max_bounces = 0;
    uint64_t n_rays = 0;

    rt::HotPair* d_pairs = nullptr;
    rt::HotPair* d_shadow_pairs = nullptr;  // the same objects sorted by decreasing size (shadow rays are order-free)
    uint32_t n_pairs = 0;
    rt::HotObject* d_hot = nullptr;
    rt::ColdObject* d_cold = nullptr;
    rt::ObjectRecord* d_objrec = nullptr;   // what materialise() reads of an object, in one 128-byte line
    float4* d_bounds = nullptr;            // screen rectangles for the current camera
    std::vector<double> h_spheres;         // per object: bounding sphere cx, cy, cz, R (R = +inf never cull, -inf never hit)
    bool rects_dirty = true;

    rt::LightRec* d_lights = nullptr;
    float4* d_rays = nullptr;
    bool have_rays = false;  // ray buffer uploaded
    bool dir_w_zero = true;

    bool pinhole = false;
    uint32_t width = 0, height = 0;
    float z = 0.f;

    rt::host::Shard shard;  // rt_set_shard's

    rt::host::Buffer d_out;        // context-owned device framebuffer
    rt::host::Buffer h_out{true};  // context-owned pinned host framebuffer (Render()'s return value)
    // 8-bit frames (rt_pack.hip): rt_render_packed's device and pinned byte frames, rt_render_device_packed's float scratch
    rt::host::Buffer d_pack, h_pack{true}, d_scratch;
    // supersampled frames (rt_resolve.hip): the factor, and the sample frame every render call with a factor > 1 filters from
    uint32_t ss = 1;
    rt::host::Buffer d_samples;
    // rt_render in passes (render_in_passes): the stream the read-backs run on, an event per pass
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_pass[rt::host::kMaxPasses] = {};

    float* aux_t = nullptr;  // caller-owned device buffers for the next render
    int32_t* aux_index = nullptr;

    rt::GridDesc grid = {};                 // device pointers owned by this context
    uint2* d_grid_cell_range = nullptr;
    float4* d_grid_cell_rec = nullptr;
    uint32_t* d_grid_entries = nullptr;
    uint32_t* d_grid_always = nullptr;
    float4* d_grid_entry_sphere = nullptr;
    std::vector<double> h_grid_spheres;     // per object: centre + grid radius (inf: always tested, < 0: never hit)
    std::vector<float> h_grid_pre;          // per object: pre-test radius as the grid's entry spheres carry it
    uint2* d_lt_range = nullptr;            // light tiles (rt_grid.h: LightTiles) for the last light's shadow rays
    float4* d_lt_records = nullptr;
    uint4* d_lt_blocks = nullptr;           // the light tiles' lists as blocks of three candidates (LightTiles::blocks)
    uint32_t* d_lt_block_ids = nullptr;
    rt::LightTiles light_tiles = {};
    // Replaceable lights (rt_set_lights): what rt_get_light_tiles_info reports of the table in use; the device builder's memory
    // (rt_light_tiles.hip; grow-only), its records' pinned mirrors and the events around its four stages; the flags rt_create was
    // given and the two reasons it may have added RT_FLAG_LITERAL for, kept apart because only one of them follows the lights;
    // and, under RT_FLAG_DEVICE_OPENCL, what object_bound gave per object (x, y, z, r) for the predicate on the new lights.
    rt_light_tiles_info_t lt_info = {};
    rt::LightTileBuffers ltb = {};
    float* d_lt_pre = nullptr;
    size_t ltb_tiles = 0, ltb_entries = 0, ltb_blocks = 0;
    rt::LightTileRecord* h_lt_record = nullptr;
    rt::PoseTileRecord* h_lt_lists = nullptr;   // [0] the lists', [1] the chains'
    hipEvent_t ev_lt[8] = {};
    uint32_t lights_capacity = 0;
    uint32_t user_flags = 0;
    bool degenerate_literal = false, lights_literal = false;
    std::vector<double> h_obj_bounds;
    rt::BlockGrid blocks = {};              // the closest-hit walk's coarse grid of 32-byte blocks (rt_grid.h: BlockGrid)
    int32_t block_occ[6] = {0, 0, 0, -1, -1, -1};  // its occupied range in cells of the grid proper: lowest x, y, z, highest x, y, z (rt_get_block_range)
    uint4* d_walk_blocks = nullptr;
    uint32_t* d_walk_ids = nullptr;
    std::vector<float4> h_walk;             // the unified walk's records while they are being put together (rt_grid.h: GridDesc::walk_rec)
    float4* d_walk_rec = nullptr;
    uint32_t* d_tile_start = nullptr;       // screen tiles (64 x 8 pixels) -> objects a pinhole primary ray can reach
    uint2* d_tile_entries = nullptr;
    rt::ScreenTiles tiles = {};
    bool tiles_dirty = true;
    uint32_t tiles_built_for = 0;           // the tile width (as a shift) the last build was asked for
    // A posed camera's table (rt_tiles.hip): the pose the ray buffer in use was generated from, the registration spheres on the
    // device (uploaded by the first posed build), the builder's device memory (grow-only), its record's pinned mirror, the
    // events around its passes, and what rt_get_tiles_info reports of the last build of either kind.
    rt::PoseGrid pose = {};
    double* d_pose_spheres = nullptr;
    rt::PoseTileBuffers ptb = {};
    size_t ptb_tiles = 0, ptb_entries = 0;
    rt::PoseTileRecord* h_pose_record = nullptr;
    hipEvent_t ev_tiles[4] = {};
    rt_tiles_info_t tiles_info = {};
    // A pose whose origin lies OUTSIDE the grid's box: `pose_outside` - the pose in use is such a one and the context
    // could serve it (a grid, a finite origin, no triangles); `primary_outside` - its table was built and accepted, so the frame keeps
    // the grid: tiles for the primary rays (registration spheres made for the pose's own origin, rt_tiles.hip: pose_spheres), the
    // grid for every later ray. The objects' bounds (kBoundDoubles per object; host copy from build_grid, device copy uploaded by the
    // first such pose, rt_set_transforms refreshes both) and the per-pose spheres on the device.
    bool pose_outside = false, primary_outside = false;
    std::vector<double> h_obj_bound6;
    double* d_obj_bound6 = nullptr;
    double* d_outside_spheres = nullptr;
    bool has_triangles = false;             // type-2 records (extension): only the grid path knows them
    int nan_winner = -1;                    // the last sphere / box of the scene decides what a NaN ray ends with (rt_device.h)
    bool nan_winner_sphere = false;
    bool forced_literal = false;            // a degenerate instance switched the context to RT_FLAG_LITERAL (rt_create)
    // Primary directions the exact eliminations are not made for - |d|^2 == 0, below 1e-30 or above 1e30 (or not finite): the
    // reference's tests then produce NaN times for every object (.cl:85-108), which only the literal loops reproduce. Such a
    // frame is rendered the literal way as a whole (apply_ray_domain): `flags` = base_flags | LITERAL while the rays in use
    // (the uploaded buffer, or the pinhole camera that replaced it) hold such a direction.
    uint32_t base_flags = 0;                // `flags` after rt_create's instance checks
    bool rays_out_of_domain = false, camera_out_of_domain = false;
    bool affine_w = true;                   // every mv / mvInverse has bottom row (0,0,0,1) exactly
    bool primary_w_one = true;              // every uploaded primary ray has start.w == 1
    double origin_lo[3] = {0, 0, 0}, origin_hi[3] = {0, 0, 0};  // box of the primary ray origins
    // Replaceable rays (rt_set_rays_device): the box build_grid's radii were derived for - the create-time origins united with the
    // padded object bounds, before the one-cell padding - and whether the ray buffer in use may be served by
    // the grid: direction.w = 0, start.w = 1, every origin inside that box. Off the grid a frame is rendered as RT_FLAG_NO_GRID
    // renders it (grid_in_use); a camera's rays start at the origin, which the box always holds.
    double grid_box_lo[3] = {0, 0, 0}, grid_box_hi[3] = {0, 0, 0};
    bool rays_off_grid = false;
    rt::RayScan* d_scan = nullptr;          // the ray scan's result (rt_rays.hip) and its pinned host mirror
    rt::RayScan* h_scan = nullptr;
    // The staging buffer of the calls that patch a range of objects from a host array (rt_set_materials, rt_set_transforms,
    // rt_set_visibility; rt_object_patch.cpp: ensure_patch_stage): one, grow-only, as large as the largest call so far needed.
    rt::host::Buffer d_patch_stage;
    // Replaceable transforms (rt_set_transforms, rt_geometry.cpp). Of the objects: type and "both bottom rows are (0,0,0,1)" per object
    // (bits 0-1 and bit 7), how many are not affine, and the position rt_create's size order gave each in the shadow stream. Of the
    // lights: a host copy (the light tiles are rebuilt, RT_FLAG_DEVICE_OPENCL's predicate is evaluated again). Of the grid: what
    // build_grid's radii were evaluated with (GridRadii, below), the create-time always-list and behind it the DYNAMIC objects - every
    // object an accepted call has named, tested by every ray from then on (the list the kernels read is d_grid_always, kMaxAlways
    // entries). A call stages its records in d_patch_stage and, behind them (at sizeof(rt_transform) * count of that call), their shadow slots.
    std::vector<uint8_t> h_kind;
    uint32_t n_not_affine = 0;
    // Compact records (rt_device.h: CompactObject; rt_compact.h). A context without triangles keeps one per object BEHIND its HotObjects,
    // in d_hot's allocation (d_compact = d_hot + n_objs + 1; null with triangles), and every patch pass keeps them true whatever
    // the predicate says, so that a scene may become diagonal by rt_set_transforms without a rebuild. Per object whether it is a sphere /
    // box that is not diagonal, how many are (maintained like n_not_affine), and whether RT_COMPACT_RECORDS allowed them at rt_create
    // ("0": no). compact_in_use() is the frame's switch, Scene::diagonal.
    rt::CompactObject* d_compact = nullptr;
    std::vector<uint8_t> h_not_diagonal;
    uint32_t n_not_diagonal = 0;
    bool compact_allowed = false;
    std::vector<uint32_t> h_shadow_slot;
    std::vector<rt_light> h_lights;
    double grid_cell = 0.0, grid_diag = 0.0, grid_s_max = 0.0, grid_k2 = 1.0;
    std::vector<uint32_t> h_always;
    uint32_t n_unbounded = 0;
    hipEvent_t ev_xf[2] = {};
    rt_geometry_info_t geo_info = {};
    // Replaceable visibility (rt_set_visibility, rt_visibility_host.cpp): the host mirror of the mask (1: hidden; empty until the first
    // call - nothing is hidden), what the patch pass reads of rt_create on the device - the type word each object was created with
    // (from h_kind; rt::kTypeKeep for a type other than 0, 1, 2) and its shadow slot, uploaded by the first call. A host mask is
    // staged in d_patch_stage.
    std::vector<uint8_t> h_hidden;
    uint32_t* d_vis_types = nullptr;
    uint32_t* d_vis_slots = nullptr;
    // Ray queries (rt_query_*, rt_query_host.cpp): the slot of the plain and hit-record queries (rt::QueryCounters). The host twins stage
    // rays and results in d_patch_stage.
    rt::host::CountedSlot query{sizeof(rt::QueryCounters)};
    // Shaded queries (rt_query_shade*): a slot of their own (rt::QueryShadeCounters), so that rt_get_query_info keeps reporting the last
    // plain or hit-record query.
    rt::host::CountedSlot query_shade{sizeof(rt::QueryShadeCounters)};
    // G-buffer frames (rt_render_gbuffer*, rt_render.cpp): the staging of (t, index) where the caller did not ask for them and of the
    // host twin's records (grow-only), the slot of the record kernel (its counter block is the hit count; `made` says a whole pass
    // has been enqueued), an event pair of its own around the primary round, and what rt_get_gbuffer_info reports of the last pass.
    // The hittest frame's `out` (MAX_FLOAT for a NaN time, where t keeps the NaN) goes to d_gb_out, which nothing reads.
    rt::host::Buffer d_gb_t, d_gb_index, d_gb_out, d_gb_point, d_gb_normal, d_gb_albedo;
    rt::host::CountedSlot gb_records{sizeof(unsigned long long)};
    hipEvent_t ev_gb_trace[2] = {};
    uint64_t gb_items = 0;
    bool gb_wavefront = false;
    // Ambient-occlusion frames (rt_ao*, rt_render_ao*; rt_query_host.cpp, rt_render.cpp): the slot of the pass (rt::AoCounters), the items
    // of the last one, whether it was a frame form and then the event pair around its internal G-buffer pass. The frame forms stage that
    // pass's index, point and normal in d_gb_index / d_gb_point / d_gb_normal (the G-buffer host twin's, which is synchronous); the host
    // twins stage the direction table and their results in d_patch_stage.
    rt::host::CountedSlot ao{sizeof(rt::AoCounters)};
    hipEvent_t ev_ao_gbuffer[2] = {};
    uint64_t ao_items = 0;
    bool ao_frame = false;
    // Filtered ambient occlusion (rt_ao_filter*, rt_render_ao_filtered*; rt_query_host.cpp, rt_render.cpp): the slot of the filter kernel
    // (rt::AoFilterCounters), the items of the last pass and whether it was a frame form - then gbuffer_ms and ao_ms lie between the three
    // events of ev_ao_filter_frame, this form's own: before the G-buffer pass, between it and the AO kernel, behind the AO kernel (the AO
    // family's events are re-recorded by a later rt_render_ao*). d_ao_counts: the frame forms' counts, grow-only.
    rt::host::CountedSlot ao_filter{sizeof(rt::AoFilterCounters) * rt::kAoFilterCounterSlots};
    rt::host::Buffer d_ao_counts;
    hipEvent_t ev_ao_filter_frame[3] = {};
    uint64_t ao_filter_items = 0;
    bool ao_filter_frame = false;
    // Posed cameras (rt_set_pose): the ray buffer in use was generated from a pose of this sample grid (0, 0: it was not). Nothing
    // but supersampling reads it - a posed frame renders as the buffer it is (pinhole stays false, width and height 0).
    uint32_t pose_w = 0, pose_h = 0;
    rt::WavefrontBuffers wf;
    bool last_wavefront = false;
    uint32_t last_rounds = 0;

    rt::Counters* d_counters = nullptr;
    rt::Counters counters = {};

    rt_setup_times_t setup = {};

    hipEvent_t ev_begin[rt::host::kTimingSlots];
    hipEvent_t ev_end[rt::host::kTimingSlots];
    uint32_t ev_count = 0;   // launches recorded since the last rt_timing_reset
    uint32_t ev_begin_made = 0, ev_end_made = 0;  // events created so far (rt_destroy frees a partial set too)
    float last_ms = 0.f;

    std::string error;
};

namespace rt::host {

int fail(rt_context* ctx, int code, const std::string& msg);
int fail_hip(rt_context* ctx, hipError_t e, const char* what);

// The C ABI must not change the calling thread's current HIP device (the caller is usually a host framework with
// its own idea of it): every entry point that needs the context's device switches to it through this guard, which
// restores the caller's device on every exit path.
struct DeviceGuard {
    int saved = -1;
    bool ok = true;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
        if (saved != device) {
            err = hipSetDevice(device);
            ok = (err == hipSuccess);
        }
    }
    ~DeviceGuard() {
        int now = -1;
        if (saved >= 0 && hipGetDevice(&now) == hipSuccess && now != saved) (void)hipSetDevice(saved);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define RT_DEVICE(ctx)                                                       \
    DeviceGuard device_guard_((ctx)->device);                                \
    if (!device_guard_.ok) return fail_hip((ctx), device_guard_.err, "hipSetDevice")

#define RT_HIP(ctx, call)                                           \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) return fail_hip((ctx), e_, #call);    \
    } while (0)

// one array of a group that grows together: the group's capacity `have` (in elements) is the caller's to set once all of them have grown
template <class T>
int grow_array(rt_context* c, T*& p, size_t have, size_t need) {
    void* q = p;
    size_t bytes = sizeof(T) * have;
    const int rc = grow_buffer(c, q, bytes, sizeof(T) * need, false);
    p = static_cast<T*>(q);
    return rc;
}

inline size_t packed_bytes(int format) { return format == RT_PIXEL_RGBA8 ? 4 : (format == RT_PIXEL_RGB8 ? 3 : 0); }

// the sample grid a factor > 1 filters over: the pinhole camera's, or the pose's the ray buffer was generated from (0: neither)
inline uint32_t sample_width(const rt_context* c) { return c->pinhole ? c->width : c->pose_w; }
inline uint32_t sample_height(const rt_context* c) { return c->pinhole ? c->height : c->pose_h; }
inline bool has_sample_grid(const rt_context* c) { return c->pinhole || c->pose_w != 0; }
inline size_t elem_bytes(const rt_context* c) { return c->kernel == RT_KERNEL_HITTEST ? sizeof(float) : 4 * sizeof(float); }
inline uint64_t local_pixels(const rt_context* c) { return c->shard.n_local / ((uint64_t)c->ss * c->ss); }  // what a render call delivers

// |d|^2 exactly as the walks compute it (fp32, unfused, left to right) against their `tame` window
inline bool direction_in_domain(float dx, float dy, float dz) {
    const volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const volatile float s1 = xx + yy;
    const float dd = s1 + zz;
    return dd > 1.0e-30f && dd < 1.0e30f;
}
// the grid (fine grid, block grid, light tiles) serves the rays in use: always a camera's, a ray buffer's unless a scan said no
// - or the rays are a pose's from outside the box whose screen tiles were accepted (primary_outside: tiles for them, the grid for the rest)
inline bool grid_in_use(const rt_context* c) { return c->grid.enabled && (c->pinhole || !c->rays_off_grid || c->primary_outside); }
// Scene::diagonal of the next wavefront frame (0: the full records). Every sphere / box is an affine scale-and-translate instance,
// there is no triangle, and the frame is not a literal one (those keep the full records).
inline uint32_t compact_in_use(const rt_context* c) {
    const bool diagonal = c->d_compact && scene_diagonal(c->has_triangles, c->affine_w, c->n_not_diagonal);
    return (diagonal && c->compact_allowed && !(c->flags & RT_FLAG_LITERAL)) ? 1u : 0u;
}

// View-space bounding sphere of what the traversal tests for object o: { x : |A x + b| <= r0 } with A, b the
// rows x,y,z of mvInverse (the kernels never consult mv for intersection) -> centre -A^-1 b, radius
// r0 * sigma_max(A^-1) <= r0 * |A^-1|_F. Computed in double, then inflated:
//   R_eff = R * (1 + 2^-9) + |c| * 2^-9
// which covers (a) the reference's own rounding: its discriminant accepts rays that pass a sphere at up to
// sqrt(1 + ~1e-6 (|c|/R)^2) radii, (b) the fp32 rounding of the bundle test. Anything doubtful (singular or
// non-finite matrices) gets +inf = never culled; unknown primitive types can never be hit = -inf.
struct Sphere { double x, y, z, r; };
// Bounding sphere of an instanced unit sphere / unit box in view space, in double precision and WITHOUT safety
// margins (callers add the ones their use needs): centre -A^-1 b, radius r0 * sigma_max(A^-1) (r0 = 1 or
// sqrt(0.75)), plus an upper bound of the squared condition number kappa^2 = (sigma_max / sigma_min)^2.
// r = +inf: no usable bound (test it for every ray); r = -inf: unknown type, can never be hit.
struct Bound { double x, y, z, r, kappa2; };

// The unified walk's record table (rt_grid.h: GridDesc::walk_rec), host side. build_grid puts down one head per cell of
// the grid padded by two empty cells on every side, then the 2nd, 3rd ... entries of every cell; build_light_tiles appends
// the light tiles' entries; upload_walk_records ships the table (or drops it when it would not fit 32-bit byte offsets).
constexpr uint32_t kWalkBorder = 2;
inline float4 walk_sphere(const float4& es) {
    const volatile float w = es.w;
    const volatile float w2 = w * w;  // the fp32 product the pre-test used to form per trip
    return make_float4(es.x, es.y, es.z, w2);
}
inline float4 walk_link(uint32_t object, uint32_t next, float key) {
    float4 r;
    std::memcpy(&r.x, &object, 4);
    std::memcpy(&r.y, &next, 4);
    r.z = key;
    r.w = 0.f;
    return r;
}

struct PoseVerdict {
    bool in_domain = false, starts_ok = false, on_grid = false;
    double origin[3] = {0, 0, 0};
    float verdict_ms = 0.f;
};

// The registration radius rg and the pre-test radius rpre of one object (rt_grid.h derives the bound; the comment is at the
// function): what build_grid evaluates per object, and rt_set_transforms for a moved one with what the grid was built for.
constexpr double kKappa2Tight = 4.0;
constexpr uint32_t kMaxAlways = 64;   // build_grid's limit for its always-list; create-time entries + dynamic objects share it
struct GridRadii {
    double lo[3], hi[3];   // the box of the ray origins and the padded bounds (rt_context::grid_box_lo / hi)
    double cell, diag;     // cell edge, the box's diagonal
    double S_max;          // the largest |origin| the box allows
};
// rg: -1 never hit, +inf always tested (`always`). rpre: the tight form (>= 0, `tight`) while kappa^2 <= kKappa2Tight and <= K2_limit -
// build_grid passes +inf and raises its K2 by the tight objects' kappa^2; a grid that is built already passes its K2 - else the full
// registration radius, negative.
struct ObjectRadii { double rg, rpre; bool tight, always; };
ObjectRadii grid_radii(const GridRadii& g, const Bound& b, uint32_t type, double K2_limit);
float pretest_as_stored(double rpre);  // rounded away from zero, as the grid's entry spheres carry it

// rt_scene.cpp
void pack_pairs(const rt_object_data* objs, const uint32_t* order, uint32_t n, std::vector<rt::HotPair>& pairs);
void repack_objects(const rt_object_data* objs, uint32_t n, std::vector<rt::HotPair>& pairs,
                    std::vector<rt::HotObject>& hot, std::vector<rt::ColdObject>& cold);
Bound object_bound(const rt_object_data& o);
Sphere bounding_sphere(const rt_object_data& o);
double size_proxy(const rt_object_data& o);
int build_grid(rt_context* c, const rt_object_data* objs, uint32_t n);
int upload_walk_records(rt_context* c);
// rt_camera_tiles.cpp
float4 screen_rect(const Sphere& s, double z);
bool detect_pinhole(const rt_ray* rays, uint64_t n, uint32_t& W, uint32_t& H, float& z);
int refresh_screen_tiles(rt_context* c, hipStream_t stream, uint32_t col_shift);
int settle_outside_pose(rt_context* c, hipStream_t stream);
bool pose_within_reach(const rt_context* c, const double origin[3]);
// rt_light_setup.cpp
bool lights_need_literal(const rt_context* c, const rt_light* L, uint32_t n_lights);
int build_light_tiles(rt_context* c, const rt_light* lights);
int build_light_tiles_device(rt_context* c, const rt_light* lights);
// rt_api.cpp: what the rt_*_multi entry points share with the single-context ones
int pose_grid(rt_context* c, uint32_t width, uint32_t height, float z, const float* m, const float* origin, rt::PoseGrid& g);
int pose_check(rt_context* c, const rt::PoseGrid& g, hipStream_t stream, PoseVerdict& v);
int pose_commit(rt_context* c, const rt::PoseGrid& g, hipStream_t stream, const PoseVerdict& v);
int check_set_lights(rt_context* c, const void* lights, uint32_t n_lights);
void apply_ray_domain(rt_context* c);
// rt_render.cpp: the work-items of ranks rank .. rank + span - 1 (whole tiles; 1 rank: everything); the path a frame takes; rt_destroy's part of it
uint64_t local_count(uint64_t n_rays, uint64_t tile_rays, uint32_t rank, uint32_t world, uint32_t span = 1);
bool use_wavefront(const rt_context* c);
void free_wavefront(rt_context* c);
// rt_object_patch.cpp: what the calls that patch a range [first, first + count) of a live context's objects share.
// The two refusals of a range and its array `p`, named `what` in the message; nothing is touched. Both at once: the range's, unless null_first.
int check_object_range(rt_context* c, const void* p, uint32_t first, uint32_t count, const char* what, bool null_first = false);
int check_set_materials(rt_context* c, const void* materials, uint32_t first, uint32_t count);
int ensure_patch_stage(rt_context* c, size_t bytes);  // c->d_patch_stage holds `bytes`; a failed call leaves the context as it was
void refresh_lights_literal(rt_context* c, const rt_light* L, uint32_t n_lights);
// Engineering aid: device time of a patch call's upload and of its pass, on stderr as "[label] copy .. ms patch .. ms unit count"
// (tools/ab/*_timing.py). Three events, created only when the variable `env` is set and destroyed on every exit path.
struct PatchTrace {
    rt_context* c;
    const char *env, *label, *unit;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on = false;
    PatchTrace(rt_context* ctx, const char* env_name, const char* bracket_label, const char* unit_word)
        : c(ctx), env(env_name), label(bracket_label), unit(unit_word) {}
    ~PatchTrace();
    PatchTrace(const PatchTrace&) = delete;
    PatchTrace& operator=(const PatchTrace&) = delete;
    int begin(hipStream_t stream);                               // before the upload, if any
    int uploaded(hipStream_t stream) { return mark(1, stream); }  // before the pass
    int patched(hipStream_t stream) { return mark(2, stream); }   // behind the pass
    int report(uint32_t count);                                  // once the stream is synchronised
private:
    int mark(int k, hipStream_t stream);
};
// rt_query_host.cpp: the records, the arithmetic mode and the primary rays as a query reads them; the G-buffer pass reads the same
rt::Scene query_scene(const rt_context* c);
int query_arith(const rt_context* c);
rt::QueryCamera query_camera(const rt_context* c);
// ... and the one path of the query families, the G-buffer pass among them:
// the slot's counter block and event pair exist (made by the first call)
int ensure_counted(rt_context* c, CountedSlot& s);
// One counted kernel on `stream`: the counters zeroed, event, launch() - a hipError_t; `what` names it in a failure -, event; then the
// slot is `made`. Asynchronous.
template <class Launch>
int enqueue_counted(rt_context* c, CountedSlot& s, hipStream_t stream, const char* what, Launch&& launch) {
    if (const int rc = ensure_counted(c, s)) return rc;
    RT_HIP(c, hipMemsetAsync(s.d_counters, 0, s.counter_bytes, stream));
    RT_HIP(c, hipEventRecord(s.ev[0], stream));
    const hipError_t e = launch();
    if (e != hipSuccess) return fail_hip(c, e, what);
    RT_HIP(c, hipEventRecord(s.ev[1], stream));
    s.made = true;
    return RT_OK;
}
// what the info readers share: waits for the slot's last kernel, reads its counter block into `counters` and takes the time between its events
int read_counted(rt_context* c, const CountedSlot& s, void* counters, double* ms);
// What every form refuses of an output struct `o` with the `members` (pointer, alignment: 4 the scalar arrays, 16 the vector arrays);
// `device`: they are device pointers, whose alignment the kernels' stores need. The two texts name the family's members.
struct OutputMember { const void* p; uintptr_t align; };
int check_outputs(rt_context* c, const void* o, std::initializer_list<OutputMember> members, bool device, const char* scalars_misaligned,
                  const char* vectors_misaligned);
int refuse_no_primary_rays(rt_context* c);
// Ambient occlusion (rt_query_host.cpp; the frame forms are rt_render.cpp's). check_ao: what every form refuses of its parameter and
// output structs (`device`: dirs and the outputs are device pointers, whose alignment the kernel needs); refuse_ao_context: a context with
// triangles. enqueue_ao: one pass over `shard.n_local` items on `stream`, every pointer device memory; asynchronous.
int check_ao(rt_context* c, const rt_ao_params_t* params, const rt_ao_t* out, bool device);
int refuse_ao_context(rt_context* c);
int enqueue_ao(rt_context* c, const rt::GBufferShard& shard, const float* d_point, const float* d_normal, const int32_t* d_index,
               const rt_ao_params_t& params, const rt_ao_t& d_out, hipStream_t stream);
// Filtered ambient occlusion (rt_query_host.cpp; the frame forms are rt_render.cpp's). check_ao_filter: what every form refuses of the
// filter's parameter and output structs and of K (`device`: the outputs are device pointers); enqueue_ao_filter: one pass over width x
// rows items on `stream`, every pointer device memory, asynchronous.
int check_ao_filter(rt_context* c, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out, uint32_t samples, bool device);
int enqueue_ao_filter(rt_context* c, const uint8_t* d_unoccluded, const float* d_point, const float* d_normal, const int32_t* d_index,
                      uint64_t width, uint64_t rows, uint32_t samples, const rt_ao_filter_params_t& filter, const rt_ao_filtered_t& d_out,
                      hipStream_t stream);
// The device copies of a host form's wanted outputs and their way back: select() hands out the device array of a wanted member (a
// null host pointer: not wanted, null), finish() copies every selected array to its host array on `stream` and waits for the stream.
struct CopyBack {
    struct Item { void* host; const void* dev; size_t bytes; } items[5];
    int count = 0;
    template <class T>
    T* select(void* host, void* dev, size_t bytes) {
        if (!host) return nullptr;
        items[count++] = Item{host, dev, bytes};
        return static_cast<T*>(dev);
    }
    int finish(rt_context* c, hipStream_t stream) const;
};
// A host form of the ambient-occlusion pass: its direction table (copied on `stream`), the wanted results (selected in `back`) and
// `extra` bytes of the caller's own (16-byte aligned, at d_extra) behind one another in the patch buffer; d_params / d_out are the device forms' arguments.
int stage_ao_host(rt_context* c, const rt_ao_params_t& params, const rt_ao_t& out, uint64_t n, size_t extra, hipStream_t stream,
                  rt_ao_params_t& d_params, rt_ao_t& d_out, CopyBack& back, char*& d_extra);
// The wanted results of a host form of the filter, n items, selected in `back` at base + offset .. (ao_filter_output_bytes(n) bytes of the
// patch buffer); returns the first byte behind them.
size_t stage_ao_filter_outputs(char* base, size_t offset, const rt_ao_filtered_t& out, uint64_t n, rt_ao_filtered_t& d_out, CopyBack& back);
size_t ao_filter_output_bytes(uint64_t n);
// rt_visibility_host.cpp: the two refusals of rt_set_visibility; nothing is touched
int check_set_visibility(rt_context* c, const void* visible, uint32_t first, uint32_t count);
// rt_geometry.cpp: every refusal of rt_set_transforms, decided on the host over the whole range; nothing is touched
int check_set_transforms(rt_context* c, const void* transforms, uint32_t first, uint32_t count);

}  // namespace rt::host
