// cpu_backend_c.cpp - C entry point over CPURaytracer, for callers that hold the scene as the reference's DEVICE-layout
// records (include/rt_records.h): the Python tests and bench.py's `cpu_baseline` leg (ctypes). It rebuilds the host
// records (the inverse of HIPRaytracer.cpp's converters), constructs the backend through the IRaytracer boundary and
// copies the frame out. No GPU, no libhip_raytracer.
#include <chrono>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "CPURaytracer.hpp"
#include "rt_records.h"

namespace {
thread_local const rt_ray* g_new_rays = nullptr;  // cpu_rt_render_set_rays: the rays SetRays gets before Render()
struct Pose { uint32_t width, height; float z; const float* m; const float* origin; };
thread_local const Pose* g_pose = nullptr;        // cpu_rt_render_set_pose: what SetPose gets before Render()
struct Materials { const rt_material* m; uint32_t first, count; };
thread_local const Materials* g_materials = nullptr;  // cpu_rt_render_set_materials: what SetMaterials gets before Render()
struct Transforms { const rt_transform* t; uint32_t first, count; };
thread_local const Transforms* g_transforms = nullptr;  // cpu_rt_render_set_transforms: what SetTransforms gets before Render()
struct Visibility { const uint8_t* v; uint32_t first, count; };
thread_local const Visibility* g_visibility = nullptr;  // cpu_rt_render_set_visibility: what SetVisibility gets before Render()

Material host_material(const rt_material& d) {
    Material m;
    m.ambient = rtm::vec3(d.ambient[0], d.ambient[1], d.ambient[2]);
    m.diffuse = rtm::vec3(d.diffuse[0], d.diffuse[1], d.diffuse[2]);
    m.specular = rtm::vec3(d.specular[0], d.specular[1], d.specular[2]);
    m.absorption = d.absorption; m.reflection = d.reflection; m.transparency = d.transparency; m.shininess = d.shininess;
    return m;
}

Ray3D host_ray(const rt_ray& r) {
    Ray3D h(rtm::vec3(0.f, 0.f, 0.f), rtm::vec3(0.f, 0.f, 0.f));
    h.start = rtm::vec4(r.start[0], r.start[1], r.start[2], r.start[3]);
    h.direction = rtm::vec4(r.direction[0], r.direction[1], r.direction[2], r.direction[3]);
    return h;
}

Light host_light(const rt_light& d) {
    LightProperties p;
    p.ambient = rtm::vec3(d.ambient[0], d.ambient[1], d.ambient[2]);
    p.diffuse = rtm::vec3(d.diffuse[0], d.diffuse[1], d.diffuse[2]);
    p.specular = rtm::vec3(d.specular[0], d.specular[1], d.specular[2]);
    Light l(p, rtm::mat4(1.f));
    l.lightPosition = rtm::vec4(d.position[0], d.position[1], d.position[2], d.position[3]);
    return l;
}

std::vector<Ray3D> host_rays(const rt_ray* rays, uint64_t n) {
    std::vector<Ray3D> q;
    q.reserve(n);
    for (uint64_t i = 0; i < n; ++i) q.push_back(host_ray(rays[i]));
    return q;
}

// The backend of the query entries: constructed with `objs_` (no lights, no frame rays), then SetTransforms(t_first,
// transforms_[0 .. t_count)) and SetVisibility(v_first, visible_[0 .. v_count)) (NULL with a count of 0: none). The vectors the
// backend refers to live here. make() is false for arguments it cannot serve (triangle records, a range beyond the objects, a NULL
// array with a count). The shaded query adds what a colour needs: lights, the kernel with its MAX_BOUNCES, and SetMaterials(m_first,
// materials_[0 .. m_count)).
struct QueryBackend {
    std::vector<ObjectData> objects;
    std::vector<Light> lights;
    std::vector<Ray3D> primary_rays;   // the backend's own rays: none for the queries, the frame's for cpu_rt_render_gbuffer (set before make())
    std::unique_ptr<CPURaytracer> backend;
    bool make(const void* objs_, uint32_t n_objs, unsigned int threads, const void* visible_, uint32_t v_first, uint32_t v_count,
              const void* transforms_, uint32_t t_first, uint32_t t_count, const void* lights_ = nullptr, uint32_t n_lights = 0,
              int kernel = 0, uint32_t max_bounces = 0, const void* materials_ = nullptr, uint32_t m_first = 0, uint32_t m_count = 0) {
        if ((!objs_ && n_objs) || (!visible_ && v_count) || (!transforms_ && t_count) || (!lights_ && n_lights) || (!materials_ && m_count) ||
            kernel < 0 || kernel > 2)
            return false;
        for (uint32_t i = 0; i < n_lights; ++i) lights.push_back(host_light(static_cast<const rt_light*>(lights_)[i]));
        const rt_object_data* objs = static_cast<const rt_object_data*>(objs_);
        objects.reserve(n_objs);
        for (uint32_t i = 0; i < n_objs; ++i) {
            const rt_object_data& d = objs[i];
            if (d.type == 2u) return false;
            ObjectData o(static_cast<ObjectData::PrimativeType>(d.type > 255u ? 255u : d.type), host_material(d.mat), rtm::mat4(1.f));
            std::memcpy(o.mv.data(), d.mv, sizeof(d.mv));
            std::memcpy(o.mvInverse.data(), d.mvInverse, sizeof(d.mvInverse));
            std::memcpy(o.mvInverseTranspose.data(), d.mvInverseTranspose, sizeof(d.mvInverseTranspose));
            objects.push_back(o);
        }
        backend.reset(new CPURaytracer(objects, lights, primary_rays, max_bounces, static_cast<CPURaytracer::Kernel>(kernel), threads));
        try {
            if (m_count) {
                std::vector<Material> ms;
                for (uint32_t i = 0; i < m_count; ++i) ms.push_back(host_material(static_cast<const rt_material*>(materials_)[i]));
                backend->SetMaterials(m_first, ms);
            }
            if (t_count) {
                const rt_transform* src = static_cast<const rt_transform*>(transforms_);
                std::vector<Transform> ts(t_count);
                for (uint32_t i = 0; i < t_count; ++i) {
                    std::memcpy(ts[i].mv.data(), src[i].mv, sizeof(src[i].mv));
                    std::memcpy(ts[i].mvInverse.data(), src[i].mvInverse, sizeof(src[i].mvInverse));
                }
                backend->SetTransforms(t_first, ts);
            }
            if (v_count) {
                const uint8_t* v = static_cast<const uint8_t*>(visible_);
                backend->SetVisibility(v_first, std::vector<uint8_t>(v, v + v_count));
            }
        } catch (const std::exception&) { return false; }
        return true;
    }
};
}  // namespace

extern "C" {

int cpu_rt_render_supersampled(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                               const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                               uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, uint32_t supersample, uint64_t sample_width);

// out: n_rays x 4 floats (kernels 1, 2) or n_rays floats (kernel 0). Returns 0, or -1 for arguments it cannot serve
// (unknown kernel; type-2 triangle records, which are the HIP backend's own extension).
int cpu_rt_render(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                  const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced, uint64_t* hit_pixels,
                  double* seconds, unsigned int* threads_used) {
    return cpu_rt_render_supersampled(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced, hit_pixels,
                                      seconds, threads_used, 1, 0);
}

// The same with CPURaytracer::SetSupersampling(supersample, sample_width): out holds n_rays / supersample^2 pixels. -1 also for a
// factor / width the backend refuses.
int cpu_rt_render_supersampled(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                               const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                               uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, uint32_t supersample, uint64_t sample_width) {
    if (kernel < 0 || kernel > 2 || (!out && n_rays)) return -1;
    const rt_object_data* objs = static_cast<const rt_object_data*>(objs_);
    const rt_light* lights = static_cast<const rt_light*>(lights_);
    const rt_ray* rays = static_cast<const rt_ray*>(rays_);
    std::vector<ObjectData> objects;
    objects.reserve(n_objs);
    for (uint32_t i = 0; i < n_objs; ++i) {
        const rt_object_data& d = objs[i];
        if (d.type == 2u) return -1;
        const Material m = host_material(d.mat);
        rtm::mat4 mv(1.f);
        std::memcpy(mv.data(), d.mv, sizeof(d.mv));
        ObjectData o(static_cast<ObjectData::PrimativeType>(d.type > 255u ? 255u : d.type), m, rtm::mat4(1.f));
        o.mv = mv;  // the uploaded matrices, byte for byte (the ctor's own inverse is not what the caller uploaded)
        std::memcpy(o.mvInverse.data(), d.mvInverse, sizeof(d.mvInverse));
        std::memcpy(o.mvInverseTranspose.data(), d.mvInverseTranspose, sizeof(d.mvInverseTranspose));
        objects.push_back(o);
    }
    std::vector<Light> ls;
    ls.reserve(n_lights);
    for (uint32_t i = 0; i < n_lights; ++i) ls.push_back(host_light(lights[i]));
    std::vector<Ray3D> rs;
    rs.reserve(n_rays);
    for (uint64_t i = 0; i < n_rays; ++i) rs.push_back(host_ray(rays[i]));
    std::unique_ptr<CPURaytracer> backend(new CPURaytracer(objects, ls, rs, max_bounces, static_cast<CPURaytracer::Kernel>(kernel), threads));
    if (supersample != 1) {
        try { backend->SetSupersampling(supersample, (size_t)sample_width); } catch (const std::exception&) { return -1; }
    }
    if (g_new_rays) {
        std::vector<Ray3D> replaced;
        replaced.reserve(n_rays);
        for (uint64_t i = 0; i < n_rays; ++i) replaced.push_back(host_ray(g_new_rays[i]));
        try { backend->SetRays(replaced); } catch (const std::exception&) { return -1; }
    }
    if (g_pose) {
        try { backend->SetPose(g_pose->width, g_pose->height, g_pose->z, g_pose->m, g_pose->origin); } catch (const std::exception&) { return -1; }
    }
    if (g_materials) {
        std::vector<Material> ms;
        ms.reserve(g_materials->count);
        for (uint32_t i = 0; i < g_materials->count; ++i) ms.push_back(host_material(g_materials->m[i]));
        try { backend->SetMaterials(g_materials->first, ms); } catch (const std::exception&) { return -1; }
    }
    if (g_transforms) {
        std::vector<Transform> ts(g_transforms->count);
        for (uint32_t i = 0; i < g_transforms->count; ++i) {
            std::memcpy(ts[i].mv.data(), g_transforms->t[i].mv, sizeof(g_transforms->t[i].mv));
            std::memcpy(ts[i].mvInverse.data(), g_transforms->t[i].mvInverse, sizeof(g_transforms->t[i].mvInverse));
        }
        try { backend->SetTransforms(g_transforms->first, ts); } catch (const std::exception&) { return -1; }
    }
    if (g_visibility) {
        const std::vector<uint8_t> mask(g_visibility->v, g_visibility->v + g_visibility->count);
        try { backend->SetVisibility(g_visibility->first, mask); } catch (const std::exception&) { return -1; }
    }
    const uint64_t n_out = backend->Pixels();
    IRaytracer* raytracer = backend.get();  // everything below goes through the reference's interface
    const auto t0 = std::chrono::steady_clock::now();
    const cl_float4* px = raytracer->Render();
    const auto t1 = std::chrono::steady_clock::now();
    for (uint64_t i = 0; i < n_out; ++i) {
        if (kernel == 0) out[i] = px[i].s[0];
        else std::memcpy(out + 4 * i, px[i].s, 16);
    }
    if (rays_traced) *rays_traced = backend->RaysTraced();
    if (hit_pixels) *hit_pixels = backend->HitPixels();
    if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
    if (threads_used) *threads_used = backend->Threads();
    return 0;
}

// CPURaytracer::SetRays through the C entry: the backend is constructed with `rays_` and renders `new_rays_` (as many) after
// SetRays - the frame must not depend on the constructor's rays. Same outputs and return value as cpu_rt_render.
int cpu_rt_render_set_rays(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                           const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                           uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, const void* new_rays_) {
    g_new_rays = static_cast<const rt_ray*>(new_rays_);
    const int rc = new_rays_ ? cpu_rt_render_supersampled(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced,
                                                          hit_pixels, seconds, threads_used, 1, 0)
                             : -1;
    g_new_rays = nullptr;
    return rc;
}

// CPURaytracer::SetPose through the C entry: the backend is constructed with `rays_` and renders the posed grid (width, height, z,
// m[9] row-major, origin[3]; width * height == n_rays) after SetPose. Same outputs and return value as cpu_rt_render.
int cpu_rt_render_set_pose(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                           const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                           uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, uint32_t width, uint32_t height, float z,
                           const float* m, const float* origin) {
    if (!m || !origin) return -1;
    const Pose pose{width, height, z, m, origin};
    g_pose = &pose;
    const int rc = cpu_rt_render_supersampled(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced,
                                              hit_pixels, seconds, threads_used, 1, 0);
    g_pose = nullptr;
    return rc;
}

// CPURaytracer::SetMaterials through the C entry: the backend is constructed with `objs_` and renders after
// SetMaterials(first, materials_[0 .. count)) - rt_material records. new_rays_ (or NULL) and m / origin (or NULL: no pose) are
// cpu_rt_render_set_rays' and cpu_rt_render_set_pose's arguments, so that the options combine. Same outputs and return value as
// cpu_rt_render; -1 also for a range beyond the objects.
int cpu_rt_render_set_materials(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                                const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                                uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, const void* materials_, uint32_t first,
                                uint32_t count, const void* new_rays_, uint32_t width, uint32_t height, float z, const float* m,
                                const float* origin) {
    if (!materials_ && count) return -1;
    const Materials mats{static_cast<const rt_material*>(materials_), first, count};
    const Pose pose{width, height, z, m, origin};
    g_materials = &mats;
    g_new_rays = static_cast<const rt_ray*>(new_rays_);
    g_pose = (m && origin) ? &pose : nullptr;
    const int rc = cpu_rt_render_supersampled(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced,
                                              hit_pixels, seconds, threads_used, 1, 0);
    g_materials = nullptr;
    g_new_rays = nullptr;
    g_pose = nullptr;
    return rc;
}

// CPURaytracer::SetTransforms through the C entry: the backend is constructed with `objs_` and renders after
// SetTransforms(t_first, transforms_[0 .. t_count)) - rt_transform records. The arguments behind them are
// cpu_rt_render_set_materials' (materials_ NULL with count 0: none), so that the options combine. Same outputs and return value
// as cpu_rt_render; -1 also for a range beyond the objects.
int cpu_rt_render_set_transforms(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                                 const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                                 uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, const void* transforms_, uint32_t t_first,
                                 uint32_t t_count, const void* materials_, uint32_t first, uint32_t count, const void* new_rays_, uint32_t width,
                                 uint32_t height, float z, const float* m, const float* origin) {
    if (!transforms_ && t_count) return -1;
    const Transforms ts{static_cast<const rt_transform*>(transforms_), t_first, t_count};
    g_transforms = &ts;
    const int rc = cpu_rt_render_set_materials(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced, hit_pixels,
                                               seconds, threads_used, materials_, first, count, new_rays_, width, height, z, m, origin);
    g_transforms = nullptr;
    return rc;
}

// CPURaytracer::SetVisibility through the C entry: the backend is constructed with `objs_` and renders after
// SetVisibility(v_first, visible_[0 .. v_count)) - one byte per object, 0 hidden. The arguments behind them are
// cpu_rt_render_set_transforms' (transforms_ NULL with t_count 0: none), so that the options combine. Same outputs and return value
// as cpu_rt_render; -1 also for a range beyond the objects.
int cpu_rt_render_set_visibility(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                                 const void* rays_, uint64_t n_rays, float* out, unsigned int threads, uint64_t* rays_traced,
                                 uint64_t* hit_pixels, double* seconds, unsigned int* threads_used, const void* visible_, uint32_t v_first,
                                 uint32_t v_count, const void* transforms_, uint32_t t_first, uint32_t t_count, const void* materials_,
                                 uint32_t first, uint32_t count, const void* new_rays_, uint32_t width, uint32_t height, float z, const float* m,
                                 const float* origin) {
    if (!visible_ && v_count) return -1;
    const Visibility vis{static_cast<const uint8_t*>(visible_), v_first, v_count};
    g_visibility = &vis;
    const int rc = cpu_rt_render_set_transforms(kernel, max_bounces, objs_, n_objs, lights_, n_lights, rays_, n_rays, out, threads, rays_traced, hit_pixels,
                                                seconds, threads_used, transforms_, t_first, t_count, materials_, first, count, new_rays_, width, height,
                                                z, m, origin);
    g_visibility = nullptr;
    return rc;
}

// CPURaytracer::QueryClosest / QueryOccluded through the C entry: on a QueryBackend of these objects, transforms and visibility the
// `n_rays` rt_ray records of `rays_` are queried. t, index (n_rays each) and occluded (n_rays bytes) may each be
// NULL. Returns 0, or -1 for arguments it cannot serve (triangle records, a range beyond the objects, a NULL array with a count).
int cpu_rt_query(const void* objs_, uint32_t n_objs, const void* rays_, uint64_t n_rays, float* t, int32_t* index, uint8_t* occluded,
                 unsigned int threads, const void* visible_, uint32_t v_first, uint32_t v_count, const void* transforms_, uint32_t t_first,
                 uint32_t t_count) {
    if (!rays_ && n_rays) return -1;
    QueryBackend q;
    if (!q.make(objs_, n_objs, threads, visible_, v_first, v_count, transforms_, t_first, t_count)) return -1;
    const std::vector<Ray3D> rays = host_rays(static_cast<const rt_ray*>(rays_), n_rays);
    if (t || index) {
        std::vector<float> qt;
        std::vector<int32_t> qi;
        q.backend->QueryClosest(rays, qt, qi);
        if (t && n_rays) std::memcpy(t, qt.data(), sizeof(float) * n_rays);
        if (index && n_rays) std::memcpy(index, qi.data(), sizeof(int32_t) * n_rays);
    }
    if (occluded) {
        std::vector<uint8_t> occ;
        q.backend->QueryOccluded(rays, occ);
        if (n_rays) std::memcpy(occluded, occ.data(), n_rays);
    }
    return 0;
}

// CPURaytracer::QueryHits / HitRecords through the C entry, on a backend made as cpu_rt_query's. records_only == 0: QueryHits with
// `mask` (NULL or n_rays int32); t and index are OUTPUTS. records_only != 0: HitRecords; t and index are INPUTS. point, normal
// (n_rays x 4 floats) and reflected (n_rays rt_ray records) may each be NULL; t and index may be NULL only as outputs. Returns 0 or -1.
int cpu_rt_query_hits(const void* objs_, uint32_t n_objs, const void* rays_, uint64_t n_rays, const int32_t* mask, float* t, int32_t* index,
                      float* point, float* normal, void* reflected, int records_only, unsigned int threads, const void* visible_,
                      uint32_t v_first, uint32_t v_count, const void* transforms_, uint32_t t_first, uint32_t t_count) {
    if ((!rays_ && n_rays) || (records_only && n_rays && (!t || !index))) return -1;
    QueryBackend q;
    if (!q.make(objs_, n_objs, threads, visible_, v_first, v_count, transforms_, t_first, t_count)) return -1;
    const std::vector<Ray3D> rays = host_rays(static_cast<const rt_ray*>(rays_), n_rays);
    CPURaytracer::Hits hits;
    try {
        if (records_only) {
            hits.t.assign(t, t + n_rays);
            hits.index.assign(index, index + n_rays);
            q.backend->HitRecords(rays, hits);
        } else {
            q.backend->QueryHits(rays, mask ? std::vector<int32_t>(mask, mask + n_rays) : std::vector<int32_t>(), hits);
        }
    } catch (const std::exception&) { return -1; }
    rt_ray* refl = static_cast<rt_ray*>(reflected);
    for (uint64_t i = 0; i < n_rays; ++i) {
        if (!records_only && t) t[i] = hits.t[i];
        if (!records_only && index) index[i] = hits.index[i];
        if (point) std::memcpy(point + 4 * i, &hits.point[i], 16);
        if (normal) std::memcpy(normal + 4 * i, &hits.normal[i], 16);
        if (refl) {
            std::memcpy(refl[i].start, &hits.reflected[i].start, 16);
            std::memcpy(refl[i].direction, &hits.reflected[i].direction, 16);
        }
    }
    return 0;
}

// CPURaytracer::RenderGBuffer through the C entry, on a backend made as cpu_rt_query's with `rays_` as its primary rays and
// SetMaterials(m_first, materials_[0 .. m_count)). t, index (n_rays each), point, normal and albedo (n_rays x 4 floats) may each be
// NULL. Returns 0 or -1.
int cpu_rt_render_gbuffer(const void* objs_, uint32_t n_objs, const void* rays_, uint64_t n_rays, float* t, int32_t* index, float* point,
                          float* normal, float* albedo, unsigned int threads, const void* visible_, uint32_t v_first, uint32_t v_count,
                          const void* transforms_, uint32_t t_first, uint32_t t_count, const void* materials_, uint32_t m_first,
                          uint32_t m_count) {
    if (!rays_ && n_rays) return -1;
    QueryBackend q;
    q.primary_rays = host_rays(static_cast<const rt_ray*>(rays_), n_rays);
    if (!q.make(objs_, n_objs, threads, visible_, v_first, v_count, transforms_, t_first, t_count, nullptr, 0, 0, 0, materials_, m_first, m_count))
        return -1;
    CPURaytracer::GBuffer g;
    try {
        q.backend->RenderGBuffer(g);
    } catch (const std::exception&) { return -1; }
    for (uint64_t i = 0; i < n_rays; ++i) {
        if (t) t[i] = g.t[i];
        if (index) index[i] = g.index[i];
        if (point) std::memcpy(point + 4 * i, &g.point[i], 16);
        if (normal) std::memcpy(normal + 4 * i, &g.normal[i], 16);
        if (albedo) std::memcpy(albedo + 4 * i, &g.albedo[i], 16);
    }
    return 0;
}

// CPURaytracer::FilterAO through the C entry: n = width * rows items; index may be NULL; ao, grey and taps may each be NULL. Needs no
// scene. Returns 0, or -1 for what FilterAO throws on.
int cpu_rt_ao_filter(const uint8_t* unoccluded, const float* point, const float* normal, const int32_t* index, uint64_t width, uint64_t rows,
                     uint32_t samples, uint32_t radius, float normal_min, float plane_max, float* ao, uint8_t* grey, uint8_t* taps) {
    const uint64_t n = width * rows;
    if (n && (!unoccluded || !point || !normal)) return -1;
    std::vector<rtm::vec4> p(n), nr(n);
    for (uint64_t i = 0; i < n; ++i) {
        p[i] = rtm::vec4(point[4 * i], point[4 * i + 1], point[4 * i + 2], point[4 * i + 3]);
        nr[i] = rtm::vec4(normal[4 * i], normal[4 * i + 1], normal[4 * i + 2], normal[4 * i + 3]);
    }
    CPURaytracer::FilteredAO f;
    try {
        CPURaytracer::FilterAO(std::vector<uint8_t>(unoccluded, unoccluded + n), p, nr, index ? std::vector<int32_t>(index, index + n) : std::vector<int32_t>(),
                               (size_t)width, samples, radius, normal_min, plane_max, f);
    } catch (const std::exception&) { return -1; }
    if (n) {
        if (ao) std::memcpy(ao, f.ao.data(), n * sizeof(float));
        if (grey) std::memcpy(grey, f.grey.data(), n);
        if (taps) std::memcpy(taps, f.taps.data(), n);
    }
    return 0;
}

// CPURaytracer::QueryShade through the C entry, on a backend made as cpu_rt_query's plus `lights_`, the colour `kernel` (1, 2) with
// `max_bounces`, and SetMaterials(m_first, materials_[0 .. m_count)). `mask`: NULL or n_rays int32. rgba (n_rays x 4 floats), t and
// index (n_rays each) may each be NULL; counts (or NULL) receives n_rays traced, rays_reference, hit_rays. Returns 0 or -1.
int cpu_rt_query_shade(int kernel, uint32_t max_bounces, const void* objs_, uint32_t n_objs, const void* lights_, uint32_t n_lights,
                       const void* rays_, uint64_t n_rays, const int32_t* mask, float* rgba, float* t, int32_t* index, uint64_t* counts,
                       unsigned int threads, const void* visible_, uint32_t v_first, uint32_t v_count, const void* transforms_, uint32_t t_first,
                       uint32_t t_count, const void* materials_, uint32_t m_first, uint32_t m_count) {
    if ((!rays_ && n_rays) || kernel < 1 || kernel > 2) return -1;
    QueryBackend q;
    if (!q.make(objs_, n_objs, threads, visible_, v_first, v_count, transforms_, t_first, t_count, lights_, n_lights, kernel, max_bounces,
                materials_, m_first, m_count))
        return -1;
    const std::vector<Ray3D> rays = host_rays(static_cast<const rt_ray*>(rays_), n_rays);
    CPURaytracer::Shade out;
    try {
        q.backend->QueryShade(rays, mask ? std::vector<int32_t>(mask, mask + n_rays) : std::vector<int32_t>(), out);
    } catch (const std::exception&) { return -1; }
    for (uint64_t i = 0; i < n_rays; ++i) {
        if (rgba) std::memcpy(rgba + 4 * i, &out.rgba[i], 16);
        if (t) t[i] = out.t[i];
        if (index) index[i] = out.index[i];
    }
    if (counts) { counts[0] = out.n_rays; counts[1] = out.rays_reference; counts[2] = out.hit_rays; }
    return 0;
}

}  // extern "C"
