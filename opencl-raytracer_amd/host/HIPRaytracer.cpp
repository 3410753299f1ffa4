#include "HIPRaytracer.hpp"

#include <cstring>

#include "rt_records.h"

namespace {

// host records -> the device layouts of rt_records.h (what the reference's cl_* converters do,
// OpenCLRaytracer.cpp:108-146)
void put3(float* dst, const rtm::vec3& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = 0.f; }
void put4(float* dst, const rtm::vec4& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }

rt_material to_device(const Material& m) {
    rt_material d;
    std::memset(&d, 0, sizeof(d));
    put3(d.ambient, m.ambient);
    put3(d.diffuse, m.diffuse);
    put3(d.specular, m.specular);
    d.absorption = m.absorption;
    d.reflection = m.reflection;
    d.transparency = m.transparency;
    d.shininess = m.shininess;
    return d;
}

rt_object_data to_device(const ObjectData& o) {
    rt_object_data d;
    std::memset(&d, 0, sizeof(d));
    d.mat = to_device(o.mat);
    std::memcpy(d.mv, o.mv.data(), sizeof(d.mv));
    std::memcpy(d.mvInverse, o.mvInverse.data(), sizeof(d.mvInverse));
    std::memcpy(d.mvInverseTranspose, o.mvInverseTranspose.data(), sizeof(d.mvInverseTranspose));
    d.type = static_cast<uint32_t>(o.type);
    return d;
}

rt_light to_device(const Light& l) {
    rt_light d;
    put3(d.ambient, l.ambient);
    put3(d.diffuse, l.diffuse);
    put3(d.specular, l.specular);
    put4(d.position, l.lightPosition);
    return d;
}

}  // namespace

HIPRaytracer::HIPRaytracer(const std::vector<ObjectData>& objects_, const std::vector<Light>& lights_,
                           const std::vector<Ray3D>& rays_, unsigned int MAX_BOUNCES, int device, unsigned int flags,
                           int kernel)
    : IRaytracer(objects_, lights_, rays_) {
    std::vector<rt_object_data> objs;
    objs.reserve(objects.size());
    for (const ObjectData& o : objects) objs.push_back(to_device(o));
    std::vector<rt_light> ls;
    ls.reserve(lights.size());
    for (const Light& l : lights) ls.push_back(to_device(l));
    static_assert(sizeof(Ray3D) == sizeof(rt_ray), "Ray3D is already in device layout");
    const int rc = rt_create(&ctx, objs.data(), static_cast<uint32_t>(objs.size()), ls.data(),
                             static_cast<uint32_t>(ls.size()), rays.data(), rays.size(), MAX_BOUNCES, kernel, device, flags);
    if (rc != RT_OK) throw std::runtime_error(std::string("HIPRaytracer: ") + rt_last_error(nullptr));
}

HIPRaytracer::HIPRaytracer(const std::vector<ObjectData>& objects_, const std::vector<Light>& lights_,
                           const std::vector<Ray3D>& rays_, unsigned int MAX_BOUNCES, const std::vector<int>& devices,
                           unsigned int flags, int kernel)
    : IRaytracer(objects_, lights_, rays_) {
    std::vector<rt_object_data> objs;
    objs.reserve(objects.size());
    for (const ObjectData& o : objects) objs.push_back(to_device(o));
    std::vector<rt_light> ls;
    ls.reserve(lights.size());
    for (const Light& l : lights) ls.push_back(to_device(l));
    // tile_rays = 0: row-tiles of 16 rows when the rays are the pinhole grid, else 65 536 rays
    const int rc = rt_create_multi(&multi, objs.data(), static_cast<uint32_t>(objs.size()), ls.data(), static_cast<uint32_t>(ls.size()),
                                   rays.data(), rays.size(), MAX_BOUNCES, kernel, devices.data(), static_cast<uint32_t>(devices.size()), 0, flags);
    if (rc != RT_OK) throw std::runtime_error(std::string("HIPRaytracer: ") + rt_multi_last_error(nullptr));
}

HIPRaytracer::~HIPRaytracer() {
    rt_destroy(ctx);
    rt_destroy_multi(multi);
}

// what a call of the one-GPU or of the several-GPU object returned: anything but RT_OK throws the library's message for that object
void HIPRaytracer::Check(int rc, const char* method) const {
    if (rc != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::") + method + ": " + (multi ? rt_multi_last_error(multi) : rt_last_error(ctx)));
}

cl_float4* HIPRaytracer::Render() {
    const float* out = nullptr;
    Check(multi ? rt_render_multi(multi, &out) : rt_render(ctx, &out), "Render");
    return reinterpret_cast<cl_float4*>(const_cast<float*>(out));
}

const uint8_t* HIPRaytracer::RenderPacked(rt_pixel_format format) {
    const uint8_t* out = nullptr;
    Check(multi ? rt_render_multi_packed(multi, format, &out) : rt_render_packed(ctx, format, &out), "RenderPacked");
    return out;
}

void HIPRaytracer::SetSupersampling(unsigned int s) {
    Check(multi ? rt_set_supersampling_multi(multi, s) : rt_set_supersampling(ctx, s), "SetSupersampling");
}

void HIPRaytracer::SetRays(const std::vector<Ray3D>& rays_) {
    if (multi) throw std::runtime_error("HIPRaytracer::SetRays: not available on the several-GPU object");
    if (rt_set_rays(ctx, rays_.data(), rays_.size()) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::SetRays: ") + rt_last_error(ctx));
    pose_width = 0;
}

void HIPRaytracer::SetPose(unsigned int width, unsigned int height, float z, const float m[9], const float origin[3], void* stream) {
    Check(multi ? rt_set_pose_multi(multi, width, height, z, m, origin) : rt_set_pose(ctx, width, height, z, m, origin, stream), "SetPose");
    pose_width = width;
}

void HIPRaytracer::SetLights(const std::vector<Light>& lights_) {
    std::vector<rt_light> ls;
    ls.reserve(lights_.size());
    for (const Light& l : lights_) ls.push_back(to_device(l));
    Check(multi ? rt_set_lights_multi(multi, ls.data(), (uint32_t)ls.size()) : rt_set_lights(ctx, ls.data(), (uint32_t)ls.size()), "SetLights");
}

void HIPRaytracer::SetMaterials(uint32_t first, const std::vector<Material>& materials) {
    std::vector<rt_material> ms;
    ms.reserve(materials.size());
    for (const Material& m : materials) ms.push_back(to_device(m));
    const uint32_t n = (uint32_t)ms.size();
    Check(multi ? rt_set_materials_multi(multi, ms.data(), first, n) : rt_set_materials(ctx, ms.data(), first, n), "SetMaterials");
}

void HIPRaytracer::SetTransforms(uint32_t first, const std::vector<Transform>& transforms) {
    std::vector<rt_transform> ts(transforms.size());
    for (size_t i = 0; i < transforms.size(); ++i) {
        std::memcpy(ts[i].mv, transforms[i].mv.data(), sizeof(ts[i].mv));
        std::memcpy(ts[i].mvInverse, transforms[i].mvInverse.data(), sizeof(ts[i].mvInverse));
    }
    const uint32_t n = (uint32_t)ts.size();
    Check(multi ? rt_set_transforms_multi(multi, ts.data(), first, n) : rt_set_transforms(ctx, ts.data(), first, n), "SetTransforms");
}

void HIPRaytracer::SetVisibility(uint32_t first, const std::vector<uint8_t>& visible) {
    const uint32_t n = (uint32_t)visible.size();
    Check(multi ? rt_set_visibility_multi(multi, visible.data(), first, n) : rt_set_visibility(ctx, visible.data(), first, n), "SetVisibility");
}

std::vector<uint8_t> HIPRaytracer::ReadVisibility(uint32_t first, uint32_t count) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    std::vector<uint8_t> out(count);
    if (rt_read_visibility(c, out.data(), first, count) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::ReadVisibility: ") + rt_last_error(c));
    return out;
}

void HIPRaytracer::QueryClosest(const std::vector<Ray3D>& q, std::vector<float>& t, std::vector<int32_t>& index) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    t.assign(q.size(), 0.f);
    index.assign(q.size(), -1);
    if (!c || rt_query_closest(c, q.data(), q.size(), t.data(), index.data()) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::QueryClosest: ") + (c ? rt_last_error(c) : "no context"));
}

void HIPRaytracer::QueryOccluded(const std::vector<Ray3D>& q, std::vector<uint8_t>& occluded) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    occluded.assign(q.size(), 0);
    if (!c || rt_query_occluded(c, q.data(), q.size(), occluded.data()) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::QueryOccluded: ") + (c ? rt_last_error(c) : "no context"));
}

void HIPRaytracer::Pick(const std::vector<uint64_t>& work_items, std::vector<float>& t, std::vector<int32_t>& index) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    t.assign(work_items.size(), 0.f);
    index.assign(work_items.size(), -1);
    if (!c || rt_query_primary(c, work_items.data(), work_items.size(), t.data(), index.data()) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::Pick: ") + (c ? rt_last_error(c) : "no context"));
}

rt_query_info_t HIPRaytracer::QueryInfo() {
    rt_query_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_query_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::QueryInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

namespace {
// n zero records and the rt_hits_t that points at them (Ray3D and rtm::vec4 are the ABI's 32- and 16-byte records)
rt_hits_t sized(HIPRaytracer::Hits& h, size_t n) {
    h.t.assign(n, 0.f);
    h.index.assign(n, -1);
    h.point.assign(n, rtm::vec4());
    h.normal.assign(n, rtm::vec4());
    Ray3D zero(rtm::vec3(0.f, 0.f, 0.f), rtm::vec3(0.f, 0.f, 0.f));
    zero.start = rtm::vec4();
    h.reflected.assign(n, zero);
    rt_hits_t out;
    out.t = h.t.data();
    out.index = h.index.data();
    out.point = reinterpret_cast<float*>(h.point.data());
    out.normal = reinterpret_cast<float*>(h.normal.data());
    out.reflected = h.reflected.data();
    return out;
}
}  // namespace

HIPRaytracer::Hits HIPRaytracer::QueryHits(const std::vector<Ray3D>& q, const std::vector<int32_t>& mask) {
    static_assert(sizeof(Ray3D) == 32 && sizeof(rtm::vec4) == 16, "the ABI's records");
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!mask.empty() && mask.size() != q.size()) throw std::runtime_error("HIPRaytracer::QueryHits: the mask must be empty or have one entry per ray");
    Hits h;
    const rt_hits_t out = sized(h, q.size());
    if (!c || rt_query_hits(c, q.data(), q.size(), mask.empty() ? nullptr : mask.data(), &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::QueryHits: ") + (c ? rt_last_error(c) : "no context"));
    return h;
}

HIPRaytracer::Hits HIPRaytracer::PickHits(const std::vector<uint64_t>& work_items) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    Hits h;
    const rt_hits_t out = sized(h, work_items.size());
    if (!c || rt_query_primary_hits(c, work_items.data(), work_items.size(), &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::PickHits: ") + (c ? rt_last_error(c) : "no context"));
    return h;
}

HIPRaytracer::Hits HIPRaytracer::PickHit(unsigned int i, unsigned int j) {
    const rt_stats_t st = Stats();
    const unsigned int width = st.pinhole ? st.width : pose_width;
    if (!width) throw std::runtime_error("HIPRaytracer::PickHit: needs a camera or a pose; with a plain ray buffer use PickHits");
    return PickHits(std::vector<uint64_t>(1, (uint64_t)j * width + i));
}

namespace {
rt_shade_t sized(HIPRaytracer::Shade& s, size_t n) {
    s.rgba.assign(n, rtm::vec4());
    s.t.assign(n, 0.f);
    s.index.assign(n, -1);
    rt_shade_t out;
    out.rgba = reinterpret_cast<float*>(s.rgba.data());
    out.t = s.t.data();
    out.index = s.index.data();
    return out;
}
}  // namespace

HIPRaytracer::Shade HIPRaytracer::QueryShade(const std::vector<Ray3D>& q, const std::vector<int32_t>& mask) {
    static_assert(sizeof(Ray3D) == 32 && sizeof(rtm::vec4) == 16, "the ABI's records");
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!mask.empty() && mask.size() != q.size()) throw std::runtime_error("HIPRaytracer::QueryShade: the mask must be empty or have one entry per ray");
    Shade s;
    const rt_shade_t out = sized(s, q.size());
    if (!c || rt_query_shade(c, q.data(), q.size(), mask.empty() ? nullptr : mask.data(), &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::QueryShade: ") + (c ? rt_last_error(c) : "no context"));
    return s;
}

HIPRaytracer::Shade HIPRaytracer::PickColours(const std::vector<uint64_t>& work_items) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    Shade s;
    const rt_shade_t out = sized(s, work_items.size());
    if (!c || rt_query_primary_shade(c, work_items.data(), work_items.size(), &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::PickColours: ") + (c ? rt_last_error(c) : "no context"));
    return s;
}

rtm::vec4 HIPRaytracer::PickColour(unsigned int i, unsigned int j) {
    const rt_stats_t st = Stats();
    const unsigned int width = st.pinhole ? st.width : pose_width;
    if (!width) throw std::runtime_error("HIPRaytracer::PickColour: needs a camera or a pose; with a plain ray buffer use PickColours");
    return PickColours(std::vector<uint64_t>(1, (uint64_t)j * width + i)).rgba[0];
}

rt_query_shade_info_t HIPRaytracer::QueryShadeInfo() {
    rt_query_shade_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_query_shade_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::QueryShadeInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

HIPRaytracer::GBuffer HIPRaytracer::RenderGBuffer(unsigned int shard) {
    static_assert(sizeof(rtm::vec4) == 16, "the ABI's records");
    rt_context* c = multi ? rt_multi_context(multi, shard) : ctx;
    if (!c) throw std::runtime_error("HIPRaytracer::RenderGBuffer: no context");
    const size_t n = (size_t)rt_local_rays(c);
    GBuffer g;
    g.t.assign(n, 0.f);
    g.index.assign(n, -1);
    g.point.assign(n, rtm::vec4());
    g.normal.assign(n, rtm::vec4());
    g.albedo.assign(n, rtm::vec4());
    rt_gbuffer_t out;
    out.t = g.t.data();
    out.index = g.index.data();
    out.point = reinterpret_cast<float*>(g.point.data());
    out.normal = reinterpret_cast<float*>(g.normal.data());
    out.albedo = reinterpret_cast<float*>(g.albedo.data());
    if (n && rt_render_gbuffer(c, &out) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::RenderGBuffer: ") + rt_last_error(c));
    return g;
}

rt_gbuffer_info_t HIPRaytracer::GBufferInfo(unsigned int shard) {
    rt_gbuffer_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, shard) : ctx;
    if (!c || rt_get_gbuffer_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::GBufferInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

HIPRaytracer::AO HIPRaytracer::RenderAO(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, unsigned int shard) {
    static_assert(sizeof(rtm::vec4) == 16, "the ABI's records");
    rt_context* c = multi ? rt_multi_context(multi, shard) : ctx;
    if (!c) throw std::runtime_error("HIPRaytracer::RenderAO: no context");
    if (samples == 0 || dirs.empty() || dirs.size() % samples) throw std::runtime_error("HIPRaytracer::RenderAO: dirs holds a whole number of sets of `samples` directions");
    const size_t n = (size_t)rt_local_rays(c);
    AO a;
    a.unoccluded.assign(n, (uint8_t)samples);
    a.ao.assign(n, 1.f);
    rt_ao_params_t params;
    params.samples = samples;
    params.n_sets = (uint32_t)(dirs.size() / samples);
    params.bias = bias;
    params.reserved = 0;
    params.dirs = dirs.data();
    if (n == 0) return a;
    rt_ao_t out;
    out.unoccluded = a.unoccluded.data();
    out.ao = a.ao.data();
    if (rt_render_ao(c, &params, &out) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::RenderAO: ") + rt_last_error(c));
    return a;
}

rt_ao_info_t HIPRaytracer::AOInfo(unsigned int shard) {
    rt_ao_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, shard) : ctx;
    if (!c || rt_get_ao_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::AOInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

HIPRaytracer::FilteredAO HIPRaytracer::FilterAO(const std::vector<uint8_t>& unoccluded, const std::vector<rtm::vec4>& point,
                                                const std::vector<rtm::vec4>& normal, const std::vector<int32_t>& index, size_t width,
                                                unsigned int samples, unsigned int radius, float normal_min, float plane_max) {
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c) throw std::runtime_error("HIPRaytracer::FilterAO: no context");
    const size_t n = unoccluded.size();
    if (point.size() != n || normal.size() != n || (!index.empty() && index.size() != n) || (n && (width == 0 || n % width)))
        throw std::runtime_error("HIPRaytracer::FilterAO: one entry per item, whole rows of `width`");
    FilteredAO f;
    f.ao.assign(n, 1.f);
    f.grey.assign(n, 255);
    f.taps.assign(n, 0);
    if (n == 0) return f;
    const rt_ao_filter_params_t filter{radius, normal_min, plane_max, 0};
    const rt_ao_filtered_t out{f.ao.data(), f.grey.data(), f.taps.data()};
    if (rt_ao_filter(c, unoccluded.data(), &point[0].x, &normal[0].x, index.empty() ? nullptr : index.data(), width, n / width, samples, &filter,
                     &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::FilterAO: ") + rt_last_error(c));
    return f;
}

HIPRaytracer::FilteredAO HIPRaytracer::RenderAOFiltered(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, unsigned int radius,
                                                        float normal_min, float plane_max) {
    if (multi) throw std::runtime_error("HIPRaytracer::RenderAOFiltered: not on the several-GPU object (a tile's neighbours live on other shards)");
    if (!ctx) throw std::runtime_error("HIPRaytracer::RenderAOFiltered: no context");
    if (samples == 0 || dirs.empty() || dirs.size() % samples)
        throw std::runtime_error("HIPRaytracer::RenderAOFiltered: dirs holds a whole number of sets of `samples` directions");
    const size_t n = (size_t)rt_local_rays(ctx);
    FilteredAO f;
    f.ao.assign(n, 1.f);
    f.grey.assign(n, 255);
    f.taps.assign(n, 0);
    rt_ao_params_t params;
    params.samples = samples;
    params.n_sets = (uint32_t)(dirs.size() / samples);
    params.bias = bias;
    params.reserved = 0;
    params.dirs = dirs.data();
    if (n == 0) return f;
    const rt_ao_filter_params_t filter{radius, normal_min, plane_max, 0};
    const rt_ao_filtered_t out{f.ao.data(), f.grey.data(), f.taps.data()};
    if (rt_render_ao_filtered(ctx, &params, &filter, &out) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::RenderAOFiltered: ") + rt_last_error(ctx));
    return f;
}

rt_ao_filter_info_t HIPRaytracer::AOFilterInfo() {
    rt_ao_filter_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_ao_filter_info(c, &info) != RT_OK)
        throw std::runtime_error(std::string("HIPRaytracer::AOFilterInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

rt_geometry_info_t HIPRaytracer::GeometryInfo() {
    rt_geometry_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_geometry_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::GeometryInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

rt_light_tiles_info_t HIPRaytracer::LightTilesInfo() {
    rt_light_tiles_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_light_tiles_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::LightTilesInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

void HIPRaytracer::SetRaysDevice(const void* d_rays, size_t n, void* stream) {
    if (multi) throw std::runtime_error("HIPRaytracer::SetRaysDevice: not available on the several-GPU object");
    if (rt_set_rays_device(ctx, d_rays, n, stream) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::SetRaysDevice: ") + rt_last_error(ctx));
    pose_width = 0;
}

size_t HIPRaytracer::Pixels() const {
    if (multi) {
        const size_t s = rt_supersampling(rt_multi_context(multi, 0));
        return s ? rays.size() / (s * s) : rays.size();
    }
    return (size_t)rt_local_pixels(ctx);
}

rt_tiles_info_t HIPRaytracer::TilesInfo() {
    rt_tiles_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_tiles_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::TilesInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

rt_rays_info_t HIPRaytracer::RaysInfo() {
    rt_rays_info_t info;
    rt_context* c = multi ? rt_multi_context(multi, 0) : ctx;
    if (!c || rt_get_rays_info(c, &info) != RT_OK) throw std::runtime_error(std::string("HIPRaytracer::RaysInfo: ") + (c ? rt_last_error(c) : "no context"));
    return info;
}

rt_stats_t HIPRaytracer::Stats() {
    rt_stats_t s;
    // (several GPUs: the counters summed over the shards, the slowest shard's kernel time - the whole frame's figures)
    Check(multi ? rt_get_stats_multi(multi, &s) : rt_get_stats(ctx, &s), "Stats");
    return s;
}
