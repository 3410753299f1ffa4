// rt_multi.cpp - several GPUs from one process (hip_raytracer.h: rt_create_multi ...): a context per device, a host thread per further shard.
#include "rt_context.h"

using namespace rt::host;

struct rt_multi {
    std::vector<rt_context*> ctx;
    std::vector<int> devices;
    std::vector<void*> d_local;      // per context: its packed tiles, on its own device
    std::vector<char> peer_ok;       // per context: devices[0] and its device can address each other's memory
    uint64_t n_rays = 0, tile_rays = 0, tiles = 0;
    uint32_t ss = 1;                 // supersampling factor of every context (rt_set_supersampling_multi)
    size_t elem = 16;
    void* h_frame = nullptr;         // rt_render_multi's frame: pinned, portable host memory (whole tiles) every device copies its tiles into
    std::vector<void*> d_bytes;      // per context: its tiles as bytes (rt_render_multi_packed; room for RGBA8), on its own device
    void* h_bytes = nullptr;         // rt_render_multi_packed's frame: pinned, portable, whole tiles of RGBA8 (RGB8 uses 3/4 of it)
    std::string error;
    // One host thread per further shard, alive from rt_create_multi to rt_destroy_multi (round 3 created and joined n - 1
    // threads per frame). A frame = one job: every worker renders its shard and puts its tiles in place, the calling thread
    // does shard 0 and waits for the others.
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t generation = 0;         // bumped per job
    uint32_t pending = 0;            // workers that have not finished the current job
    bool quit = false;
    void* job_target = nullptr;      // where the tiles go: a frame on devices[0], or the pinned host frame
    bool job_to_host = false;
    int job_format = 0;              // 0: float elements; an rt_pixel_format: every shard packs its tiles before they travel
    std::vector<int> rcs;
    std::vector<std::string> errs;
};

namespace {

thread_local std::string g_multi_error;

int multi_fail(rt_multi* m, int code, const std::string& msg) {
    if (m) m->error = msg;
    else g_multi_error = msg;
    return code;
}

// one shard: render on the context's own stream, then put its tiles where they belong - in the frame on devices[0]
// (rt_render_multi_device) or STRAIGHT in the pinned host frame (rt_render_multi: the reference's blocking read-back,
// OpenCLRaytracer.cpp:94, over every GPU's own PCIe link at once instead of a hop to devices[0] and one link for the lot)
int multi_render_shard(rt_multi* m, uint32_t r, void* frame, bool to_host, int format, std::string& err) {
    rt_context* c = m->ctx[r];
    DeviceGuard guard(c->device);
    if (!guard.ok) { err = std::string("hipSetDevice: ") + hipGetErrorString(guard.err); return RT_ERR_HIP; }
    const bool fused = format && m->ss > 1;  // a supersampled byte frame: filter + quantise in one pass, straight into the byte tiles
    int rc = fused ? RT_OK : rt_render_device(c, m->d_local[r], c->stream);  // (with a factor: this shard's PIXELS, tile_rays / s^2 per tile)
    if (rc != RT_OK) { err = c->error; return rc; }
    const uint32_t n = (uint32_t)m->ctx.size();
    const uint64_t mine = m->tiles / n + ((m->tiles % n) > r ? 1 : 0);
    const size_t tile_bytes = (size_t)(m->tile_rays / ((uint64_t)m->ss * m->ss)) * (format ? packed_bytes(format) : m->elem);
    hipError_t e = hipSuccess;
    void* local = m->d_local[r];  // what travels: the float tiles, or their bytes
    if (format) {
        if (!m->d_bytes[r]) {
            e = hipMalloc(&m->d_bytes[r], c->shard.n_local ? (size_t)c->shard.n_local * 4 : 16);
            if (e != hipSuccess) { err = std::string("byte tiles: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP; }
        }
        local = m->d_bytes[r];
        if (fused) rc = rt_render_device_packed(c, format, local, c->stream);
        else rc = rt_pack_device(c, m->d_local[r], c->shard.n_local, format, local, c->stream);
        if (rc != RT_OK) { err = c->error; return rc; }
    }
    if (mine) {
        // tile j of this shard is tile j * n + r of the frame: one strided copy
        char* dst = static_cast<char*>(frame) + (size_t)r * tile_bytes;
        if (to_host) {
            e = hipMemcpy2DAsync(dst, (size_t)n * tile_bytes, local, tile_bytes, tile_bytes, (size_t)mine, hipMemcpyDeviceToHost, c->stream);
        } else if (c->device == m->devices[0] || m->peer_ok[r]) {
            e = hipMemcpy2DAsync(dst, (size_t)n * tile_bytes, local, tile_bytes, tile_bytes, (size_t)mine, hipMemcpyDeviceToDevice, c->stream);
        } else {
            for (uint64_t j = 0; j < mine && e == hipSuccess; ++j)
                e = hipMemcpyPeerAsync(dst + (size_t)j * n * tile_bytes, m->devices[0], static_cast<char*>(local) + (size_t)j * tile_bytes,
                                       c->device, tile_bytes, c->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { err = std::string("tile placement: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    return RT_OK;
}

void multi_worker(rt_multi* m, uint32_t r) {
    uint64_t seen = 0;
    for (;;) {
        void* target;
        bool to_host;
        int format;
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv_go.wait(lk, [&] { return m->quit || m->generation != seen; });
            if (m->quit) return;
            seen = m->generation;
            target = m->job_target;
            to_host = m->job_to_host;
            format = m->job_format;
        }
        std::string err;
        const int rc = multi_render_shard(m, r, target, to_host, format, err);
        {
            std::lock_guard<std::mutex> lk(m->mu);
            m->rcs[r] = rc;
            m->errs[r] = err;
            if (--m->pending == 0) m->cv_done.notify_all();
        }
    }
}

// every shard renders and places its tiles; returns when the frame is complete
int multi_run_frame(rt_multi* m, void* target, bool to_host, int format = 0) {
    const uint32_t n = (uint32_t)m->ctx.size();
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->job_target = target;
        m->job_to_host = to_host;
        m->job_format = format;
        m->pending = (uint32_t)m->workers.size();
        m->generation += 1;
    }
    m->cv_go.notify_all();
    std::string err0;
    const int rc0 = multi_render_shard(m, 0, target, to_host, format, err0);
    {
        std::unique_lock<std::mutex> lk(m->mu);
        m->cv_done.wait(lk, [&] { return m->pending == 0; });
        m->rcs[0] = rc0;
        m->errs[0] = err0;
    }
    for (uint32_t r = 0; r < n; ++r)
        if (m->rcs[r] != RT_OK) return multi_fail(m, m->rcs[r], "shard " + std::to_string(r) + ": " + m->errs[r]);
    return RT_OK;
}

// A call every context takes, all or none: `check` (every refusal, nothing touched) on every context, then `apply` on every context.
template <class Check, class Apply>
int multi_all_or_none(rt_multi* m, Check check, Apply apply) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    for (rt_context* c : m->ctx) {
        const int rc = check(c);
        if (rc != RT_OK) return multi_fail(m, rc, c->error);
    }
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        const int rc = apply(m->ctx[r]);
        if (rc != RT_OK) return multi_fail(m, rc, "shard " + std::to_string(r) + ": " + m->ctx[r]->error);
    }
    return RT_OK;
}

}  // namespace

extern "C" {

const char* rt_multi_last_error(const rt_multi* m) { return m ? m->error.c_str() : g_multi_error.c_str(); }

void rt_destroy_multi(rt_multi* m) {
    if (!m) return;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->quit = true;
    }
    m->cv_go.notify_all();
    for (std::thread& t : m->workers) t.join();
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        if (m->ctx[r] && r < m->d_local.size() && m->d_local[r]) {
            DeviceGuard guard(m->ctx[r]->device);
            (void)hipFree(m->d_local[r]);
        }
        if (m->ctx[r] && r < m->d_bytes.size() && m->d_bytes[r]) {
            DeviceGuard guard(m->ctx[r]->device);
            (void)hipFree(m->d_bytes[r]);
        }
        rt_destroy(m->ctx[r]);
    }
    if (!m->devices.empty()) {
        DeviceGuard guard(m->devices[0]);
        if (m->h_frame) (void)hipHostFree(m->h_frame);
        if (m->h_bytes) (void)hipHostFree(m->h_bytes);
    }
    delete m;
}

int rt_create_multi(rt_multi** out, const void* objs, uint32_t n_objs, const void* lights, uint32_t n_lights, const void* rays,
                    uint64_t n_rays, uint32_t max_bounces, int kernel, const int* devices, uint32_t n_devices, uint64_t tile_rays,
                    uint32_t flags) {
    g_multi_error.clear();
    if (!out) return multi_fail(nullptr, RT_ERR_INVALID_ARGUMENT, "m is NULL");
    *out = nullptr;
    if (!devices || n_devices == 0 || n_devices > 64) return multi_fail(nullptr, RT_ERR_INVALID_ARGUMENT, "need 1..64 device ordinals");
    rt_multi* m = new (std::nothrow) rt_multi();
    if (!m) return multi_fail(nullptr, RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    m->devices.assign(devices, devices + n_devices);
    m->ctx.assign(n_devices, nullptr);
    m->d_local.assign(n_devices, nullptr);
    m->d_bytes.assign(n_devices, nullptr);
    m->peer_ok.assign(n_devices, 0);
    m->n_rays = n_rays;
    m->elem = kernel == RT_KERNEL_HITTEST ? sizeof(float) : 4 * sizeof(float);
    // the contexts are built side by side: each one's grid / tile builders run on a host thread of their own
    std::vector<int> rcs(n_devices, RT_OK);
    std::vector<std::string> errs(n_devices);
    {
        std::vector<std::thread> workers;
        for (uint32_t r = 0; r < n_devices; ++r)
            workers.emplace_back([&, r]() {
                rcs[r] = rt_create(&m->ctx[r], objs, n_objs, lights, n_lights, rays, n_rays, max_bounces, kernel, m->devices[r], flags);
                if (rcs[r] != RT_OK) errs[r] = rt_last_error(nullptr);
            });
        for (std::thread& t : workers) t.join();
    }
    for (uint32_t r = 0; r < n_devices; ++r)
        if (rcs[r] != RT_OK) {
            const int rc = multi_fail(nullptr, rcs[r], "context " + std::to_string(r) + " (device " + std::to_string(m->devices[r]) + "): " + errs[r]);
            rt_destroy_multi(m);
            return rc;
        }
    // tiles: the caller's, or row-tiles of 16 rows when the rays are the pinhole grid, else 65 536 rays
    if (tile_rays == 0) {
        const rt_context* c0 = m->ctx[0];
        tile_rays = c0->pinhole && c0->width ? 16ull * c0->width : 65536ull;
    }
    m->tile_rays = tile_rays;
    m->tiles = (n_rays + tile_rays - 1) / tile_rays;
    for (uint32_t r = 0; r < n_devices; ++r) {
        rt_context* c = m->ctx[r];
        int rc = rt_set_shard(c, tile_rays, r, n_devices);
        hipError_t e = hipSuccess;
        if (rc == RT_OK) {
            DeviceGuard guard(c->device);
            const size_t bytes = (size_t)c->shard.n_local * m->elem;
            e = hipMalloc(&m->d_local[r], bytes ? bytes : 16);
            if (e == hipSuccess && c->device != m->devices[0]) {  // both directions; "already enabled" is fine
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c->device, m->devices[0]) == hipSuccess && can) {
                    const hipError_t pe = hipDeviceEnablePeerAccess(m->devices[0], 0);
                    if (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) m->peer_ok[r] = 1;
                    (void)hipGetLastError();
                }
            }
        }
        if (rc != RT_OK || e != hipSuccess) {
            const int code = multi_fail(nullptr, rc != RT_OK ? rc : RT_ERR_HIP, rc != RT_OK ? c->error : std::string("hipMalloc: ") + hipGetErrorString(e));
            rt_destroy_multi(m);
            return code;
        }
    }
    m->rcs.assign(n_devices, RT_OK);
    m->errs.assign(n_devices, std::string());
    for (uint32_t r = 1; r < n_devices; ++r) m->workers.emplace_back(multi_worker, m, r);
    *out = m;
    return RT_OK;
}

int rt_set_camera_multi(rt_multi* m, uint32_t width, uint32_t height, float z) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    for (rt_context* c : m->ctx) {
        const int rc = rt_set_camera(c, width, height, z);
        if (rc != RT_OK) return multi_fail(m, rc, c->error);
    }
    return RT_OK;
}

// rt_set_pose on every context, all or none: every shard's verdict pass and refusals first, each on a host thread of its own and
// its context's device and stream; only when no shard refuses, every shard generates.
int rt_set_pose_multi(rt_multi* m, uint32_t width, uint32_t height, float z, const float* mat, const float* origin) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    const size_t n = m->ctx.size();
    rt::PoseGrid g;
    for (rt_context* c : m->ctx) {
        const int rc = pose_grid(c, width, height, z, mat, origin, g);
        if (rc != RT_OK) return multi_fail(m, rc, c->error);
    }
    std::vector<PoseVerdict> verdicts(n);
    std::vector<int> rcs(n, RT_OK);
    for (int phase = 0; phase < 2; ++phase) {
        auto shard = [&](size_t r) {
            rt_context* c = m->ctx[r];
            rcs[r] = phase == 0 ? pose_check(c, g, c->stream, verdicts[r]) : pose_commit(c, g, c->stream, verdicts[r]);
        };
        std::vector<std::thread> workers;
        for (size_t r = 1; r < n; ++r) workers.emplace_back(shard, r);
        if (n) shard(0);
        for (std::thread& t : workers) t.join();
        for (size_t r = 0; r < n; ++r)
            if (rcs[r] != RT_OK) return multi_fail(m, rcs[r], "shard " + std::to_string(r) + ": " + m->ctx[r]->error);
    }
    return RT_OK;
}

// All or none: what a shard can refuse of such a call it refuses on the host, before anything is touched (check_set_*).
int rt_set_lights_multi(rt_multi* m, const void* lights, uint32_t n_lights) {
    return multi_all_or_none(m, [&](rt_context* c) { return check_set_lights(c, lights, n_lights); },
                             [&](rt_context* c) { return rt_set_lights(c, lights, n_lights); });
}

int rt_set_materials_multi(rt_multi* m, const void* materials, uint32_t first, uint32_t count) {
    return multi_all_or_none(m, [&](rt_context* c) { return check_set_materials(c, materials, first, count); },
                             [&](rt_context* c) { return rt_set_materials(c, materials, first, count); });
}

// (every refusal is the host's: bounds, the grid box, the dynamic set's room, per shard)
int rt_set_transforms_multi(rt_multi* m, const void* transforms, uint32_t first, uint32_t count) {
    return multi_all_or_none(m, [&](rt_context* c) { return check_set_transforms(c, transforms, first, count); },
                             [&](rt_context* c) { return rt_set_transforms(c, transforms, first, count); });
}

int rt_set_visibility_multi(rt_multi* m, const uint8_t* visible, uint32_t first, uint32_t count) {
    return multi_all_or_none(m, [&](rt_context* c) { return check_set_visibility(c, visible, first, count); },
                             [&](rt_context* c) { return rt_set_visibility(c, visible, first, count); });
}

uint64_t rt_multi_frame_elems(const rt_multi* m) { return m ? m->tiles * m->tile_rays : 0; }

int rt_set_supersampling_multi(rt_multi* m, uint32_t s) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    if (s >= 2 && s <= 4 && !m->ctx.empty() && sample_width(m->ctx[0]) && m->tile_rays % ((uint64_t)s * sample_width(m->ctx[0])))
        return multi_fail(m, RT_ERR_INVALID_ARGUMENT, "with supersampling a tile must hold whole pixel rows: pass a tile_rays with tile_rays % (s * width) == 0 to rt_create_multi");
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        const int rc = rt_set_supersampling(m->ctx[r], s);
        if (rc != RT_OK) {  // all or none
            for (size_t q = 0; q < r; ++q) (void)rt_set_supersampling(m->ctx[q], m->ss);
            return multi_fail(m, rc, m->ctx[r]->error);
        }
    }
    m->ss = s;
    return RT_OK;
}

uint64_t rt_multi_frame_pixels(const rt_multi* m) { return m ? rt_multi_frame_elems(m) / ((uint64_t)m->ss * m->ss) : 0; }

rt_context* rt_multi_context(rt_multi* m, uint32_t r) { return (m && r < m->ctx.size()) ? m->ctx[r] : nullptr; }

int rt_render_multi_device(rt_multi* m, void* d_frame) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    if (!d_frame && m->n_rays) return multi_fail(m, RT_ERR_INVALID_ARGUMENT, "d_frame is NULL");
    return multi_run_frame(m, d_frame, false);
}

int rt_render_multi(rt_multi* m, const float** out) {
    if (!m || !out) return RT_ERR_INVALID_ARGUMENT;
    if (!m->h_frame) {
        // whole tiles (the last one may be ragged: its padding work-items are written like pixels), pinned and PORTABLE: every
        // device of the node copies into it
        DeviceGuard guard(m->devices[0]);
        if (!guard.ok) return multi_fail(m, RT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.err));
        const size_t frame_bytes = (size_t)rt_multi_frame_elems(m) * m->elem;
        const hipError_t e = hipHostMalloc(&m->h_frame, frame_bytes ? frame_bytes : 16, hipHostMallocPortable);
        if (e != hipSuccess) return multi_fail(m, e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP, std::string("host frame: ") + hipGetErrorString(e));
    }
    const int rc = multi_run_frame(m, m->h_frame, true);  // Render() is synchronous (OpenCLRaytracer.cpp:94): every shard has waited for its copy
    if (rc != RT_OK) return rc;
    *out = static_cast<const float*>(m->h_frame);
    return RT_OK;
}

int rt_render_multi_packed(rt_multi* m, int format, const uint8_t** out) {
    if (!m || !out) return RT_ERR_INVALID_ARGUMENT;
    if (!packed_bytes(format)) return multi_fail(m, RT_ERR_INVALID_ARGUMENT, "unknown pixel format (RT_PIXEL_RGBA8 = 1, RT_PIXEL_RGB8 = 2)");
    if (m->elem != 4 * sizeof(float))
        return multi_fail(m, RT_ERR_STATE, "RT_KERNEL_HITTEST contexts render one float (the nearest t) per ray, not a colour: there is no 8-bit frame of it");
    if (!m->h_bytes) {  // whole tiles, pinned and portable like rt_render_multi's float frame
        DeviceGuard guard(m->devices[0]);
        if (!guard.ok) return multi_fail(m, RT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.err));
        const size_t frame_bytes = (size_t)rt_multi_frame_elems(m) * 4;
        const hipError_t e = hipHostMalloc(&m->h_bytes, frame_bytes ? frame_bytes : 16, hipHostMallocPortable);
        if (e != hipSuccess) return multi_fail(m, e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP, std::string("host byte frame: ") + hipGetErrorString(e));
    }
    const int rc = multi_run_frame(m, m->h_bytes, true, format);
    if (rc != RT_OK) return rc;
    *out = static_cast<const uint8_t*>(m->h_bytes);
    return RT_OK;
}

/* the counters of the last counted render summed over the shards, the slowest shard's kernel time */
int rt_get_stats_multi(rt_multi* m, rt_stats_t* out) {
    if (!m || !out) return RT_ERR_INVALID_ARGUMENT;
    rt_stats_t sum;
    std::memset(&sum, 0, sizeof(sum));
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        rt_stats_t s;
        const int rc = rt_get_stats(m->ctx[r], &s);
        if (rc != RT_OK) return multi_fail(m, rc, m->ctx[r]->error);
        if (r == 0) sum = s;
        else {
            sum.rays_traced += s.rays_traced;
            sum.rays_reference += s.rays_reference;
            sum.hit_pixels += s.hit_pixels;
            sum.object_tests += s.object_tests;
            sum.local_rays += s.local_rays;
            sum.last_kernel_ms = std::max(sum.last_kernel_ms, s.last_kernel_ms);
            sum.rounds = std::max(sum.rounds, s.rounds);
            sum.wavefront = sum.wavefront | s.wavefront;
        }
    }
    *out = sum;
    return RT_OK;
}

int rt_count_rays_multi(rt_multi* m) {
    if (!m) return RT_ERR_INVALID_ARGUMENT;
    for (rt_context* c : m->ctx) {
        const int rc = rt_count_rays(c);
        if (rc != RT_OK) return multi_fail(m, rc, c->error);
    }
    return RT_OK;
}

}  // extern "C"
