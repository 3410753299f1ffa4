// HIPRaytracer.hpp - drop-in replacement for the reference's OpenCLRaytracer (OpenCLRaytracer.hpp:24-85):
//     IRaytracer* raytracer = new HIPRaytracer(objects, lights, rays, MAX_BOUNCES);
//     cl_float4* pixels = raytracer->Render();
// The host side sees only the C ABI (include/hip_raytracer.h); kernels live in libhip_raytracer.so.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "IRaytracer.hpp"
#include "hip_raytracer.h"

class HIPRaytracer : public IRaytracer {
public:
    // Same argument meaning as OpenCLRaytracer's ctor (OpenCLRaytracer.hpp:61). Errors throw std::runtime_error
    // (the reference lets Boost.Compute exceptions escape). `kernel` selects hittest / shade / shade_and_reflect;
    // the reference host only ever loads shade_and_reflect (OpenCLRaytracer.cpp:53-59).
    HIPRaytracer(const std::vector<ObjectData>& objects, const std::vector<Light>& lights, const std::vector<Ray3D>& rays,
                 unsigned int MAX_BOUNCES, int device = 0, unsigned int flags = 0,
                 int kernel = RT_KERNEL_SHADE_AND_REFLECT);
    // The same raytracer over several GPUs of one node (north_star: row-tiles across the GPUs, gathered on the first):
    // one entry of `devices` per shard (an ordinal may repeat: a rehearsal on fewer GPUs), interleaved row-tiles,
    // Render() returns the whole frame as before. rt_create_multi / rt_render_multi of the C ABI.
    HIPRaytracer(const std::vector<ObjectData>& objects, const std::vector<Light>& lights, const std::vector<Ray3D>& rays,
                 unsigned int MAX_BOUNCES, const std::vector<int>& devices, unsigned int flags = 0,
                 int kernel = RT_KERNEL_SHADE_AND_REFLECT);
    ~HIPRaytracer() override;
    HIPRaytracer(const HIPRaytracer&) = delete;
    HIPRaytracer& operator=(const HIPRaytracer&) = delete;

    // Inherited via IRaytracer: synchronous; the returned buffer is owned by this object and overwritten by
    // the next call (OpenCLRaytracer.cpp:94,104).
    cl_float4* Render() override;

    // The frame as 8-bit pixels (hip_raytracer.h, "8-bit frames"): quantised on the GPU(s), a quarter (RGBA8) or 3/16 (RGB8) of
    // Render()'s bytes cross the bus. Synchronous; width * height pixels of 4 or 3 bytes in work-item order, in a buffer owned
    // by the library and overwritten by the next RenderPacked(). Works for the one-GPU and the several-GPU object.
    const uint8_t* RenderPacked(rt_pixel_format format = RT_PIXEL_RGBA8);

    // Supersampled frames (hip_raytracer.h, "supersampled frames"): the rays are the SAMPLE grid (s W x s H at s z, accepted as a
    // pinhole grid by rt_create); after SetSupersampling(s) Render() / RenderPacked() return Pixels() = rays / s^2 pixels, box-filtered
    // on the GPU(s). s = 1 is off. Throws std::runtime_error with the library's message for what it refuses.
    void SetSupersampling(unsigned int s);
    size_t Pixels() const;

    // Replaceable rays (hip_raytracer.h, "replaceable rays"): the next Render() uses these primary rays - as many as the object was
    // constructed with - instead of the constructor's (which are not touched: the reference's interface holds them by const
    // reference). SetRays takes host rays, SetRaysDevice n records of 32 bytes in DEVICE memory, scanned and copied on the GPU
    // behind the work already on `stream` (a hipStream_t; nullptr = the legacy default stream). Both are synchronous. One-GPU
    // objects only; throws std::runtime_error with the library's message for what it refuses.
    void SetRays(const std::vector<Ray3D>& rays);
    void SetRaysDevice(const void* d_rays, size_t n, void* stream = nullptr);

    // Posed cameras (hip_raytracer.h, "posed cameras"): the next Render() sees the pinhole grid (width, height, z) through the fp32
    // matrix m (row-major) from `origin`; the rays are generated on the GPU(s) into the library's own buffer. width * height is the
    // number of rays the object was constructed with; with SetSupersampling(s > 1) it is the sample grid. Synchronous; `stream` (a
    // hipStream_t; nullptr = the legacy default stream) counts for the one-GPU object, the several-GPU object uses every shard's own.
    // Throws std::runtime_error with the library's message for what it refuses.
    void SetPose(unsigned int width, unsigned int height, float z, const float m[9], const float origin[3], void* stream = nullptr);

    // Replaceable lights (hip_raytracer.h, "replaceable lights"): the next Render() lights the scene with these lights - any count,
    // none included - instead of the constructor's (which are not touched). The last light's tiles are rebuilt on the GPU(s).
    // Synchronous; the several-GPU object replaces them on every shard, all or none. Throws std::runtime_error with the library's
    // message for what it refuses.
    void SetLights(const std::vector<Light>& lights);
    // rt_get_light_tiles_info: the light tiles the next frame's shadow rays to the last light use - rt_create's (host-built) or,
    // after SetLights, the ones built on the GPU. The several-GPU object reports its first shard's.
    rt_light_tiles_info_t LightTilesInfo();

    // Replaceable materials (hip_raytracer.h, "replaceable materials"): the next Render() shades objects first .. first + n - 1
    // with these materials instead of the constructor's (which are not touched); geometry stays. The object records are patched
    // on the GPU(s), nothing is rebuilt. Synchronous; the several-GPU object patches every shard, all or none. Throws
    // std::runtime_error with the library's message for what it refuses (a range beyond the objects).
    void SetMaterials(uint32_t first, const std::vector<Material>& materials);

    // Replaceable transforms (hip_raytracer.h, "replaceable transforms"): the next Render() has objects first .. first + n - 1
    // where these mv / mvInverse put them; materials and type stay. The records are patched on the GPU(s); on a scene large
    // enough for the grid the objects become dynamic (at most 64 of them, GeometryInfo()). Synchronous; the several-GPU object
    // moves them on every shard, all or none. Throws std::runtime_error with the library's message for what it refuses.
    void SetTransforms(uint32_t first, const std::vector<Transform>& transforms);
    // rt_get_geometry_info: the dynamic set and what the last SetTransforms did. The several-GPU object reports its first shard's.
    rt_geometry_info_t GeometryInfo();

    // Replaceable visibility (hip_raytracer.h, "replaceable visibility"): the next Render() does not hit objects first .. first + n - 1
    // whose entry of `visible` is 0, and hits the others as the constructor's type says; indices, materials and matrices stay. Every
    // copy of the type word is patched on the GPU(s), no table is rebuilt. Synchronous; the several-GPU object patches every shard,
    // all or none. Throws std::runtime_error with the library's message for what it refuses (a range beyond the objects).
    void SetVisibility(uint32_t first, const std::vector<uint8_t>& visible);
    // rt_read_visibility: 1 / 0 per object first .. first + count - 1, read from every device copy of the type word. The several-GPU
    // object reads its first shard's.
    std::vector<uint8_t> ReadVisibility(uint32_t first, uint32_t count);

    // Ray queries (hip_raytracer.h, "ray queries"): closest hit and occlusion for rays of the caller's own - any number, whatever the
    // frame's - on the objects as SetTransforms / SetVisibility have left them; the frame is untouched. t[i]: the nearest time
    // (MAX_FLOAT on a miss), index[i]: the object or -1; occluded[i]: something lies on start .. start + direction. Pick: the same for
    // the frame's OWN primary rays of the work-items j * width + i - the object under the mouse. Synchronous (rt_query_closest,
    // rt_query_occluded, rt_query_primary); the several-GPU object asks its first shard, which holds the whole scene. Throws
    // std::runtime_error with the library's message for what it refuses.
    void QueryClosest(const std::vector<Ray3D>& rays, std::vector<float>& t, std::vector<int32_t>& index);
    void QueryOccluded(const std::vector<Ray3D>& rays, std::vector<uint8_t>& occluded);
    void Pick(const std::vector<uint64_t>& work_items, std::vector<float>& t, std::vector<int32_t>& index);
    rt_query_info_t QueryInfo();

    // Hit-record queries (hip_raytracer.h, "hit-record queries"): QueryClosest's (t, index) with WHERE the ray meets the winner and how
    // the surface faces there - point: the view-space intersection; normal: the unit normal in xyz, w = 0; reflected: the next ray of
    // the reflection chain - in the context's arithmetic mode, one entry per ray; zero records where index is -1. `mask`: empty, or
    // one entry per ray - a negative entry is not traced and reads as a miss (pass the previous bounce's index along a chain).
    // PickHit(i, j): the record under column i, row j of the camera's or the last SetPose's grid (std::runtime_error with a plain
    // ray buffer: use PickHits); PickHits: of the frame's own primary rays of the work-items. Synchronous (rt_query_hits,
    // rt_query_primary_hits); the several-GPU object asks its first shard.
    struct Hits {
        std::vector<float> t;
        std::vector<int32_t> index;
        std::vector<rtm::vec4> point, normal;
        std::vector<Ray3D> reflected;
    };
    Hits QueryHits(const std::vector<Ray3D>& rays, const std::vector<int32_t>& mask = std::vector<int32_t>());
    Hits PickHits(const std::vector<uint64_t>& work_items);
    Hits PickHit(unsigned int i, unsigned int j);

    // Shaded queries (hip_raytracer.h, "shaded queries"): the COLOUR along rays of the caller's own - any number - on the objects,
    // materials and lights as the setters have left them, with this object's kernel, MAX_BOUNCES and arithmetic; the frame is
    // untouched. rgba[i]: the pixel a fresh object constructed with these rays renders, bit for bit ((0,0,0,1) on a miss); t[i],
    // index[i]: its primary hit as the kernel takes it. `mask`: empty, or one entry per ray - a negative entry is not traced and reads
    // as a miss. PickColour(i, j): the pixel under column i, row j of the camera's or the last SetPose's grid as an unsharded,
    // unfiltered frame holds it (std::runtime_error with a plain ray buffer: use PickColours); PickColours: of the frame's own primary
    // rays of the work-items. Synchronous (rt_query_shade, rt_query_primary_shade); the several-GPU object asks its first shard.
    // Throws std::runtime_error with the library's message for what it refuses (a hittest object, a scene with triangles).
    struct Shade {
        std::vector<rtm::vec4> rgba;
        std::vector<float> t;
        std::vector<int32_t> index;
    };
    Shade QueryShade(const std::vector<Ray3D>& rays, const std::vector<int32_t>& mask = std::vector<int32_t>());
    Shade PickColours(const std::vector<uint64_t>& work_items);
    rtm::vec4 PickColour(unsigned int i, unsigned int j);
    rt_query_shade_info_t QueryShadeInfo();

    // G-buffer frames (hip_raytracer.h, "G-buffer frames"): the primary hit of every local work-item of the frame - t, index, the
    // view-space point, the unit normal (w = 0) and the winner's diffuse colour (w = 1) - one entry per work-item (per sample under
    // supersampling) in the order Render() writes pixels; zero records where index is -1. The pass is the frame's own primary round
    // plus one streaming kernel, follows every setter and leaves the frame alone; it works with every kernel and on scenes with
    // triangles. Synchronous (rt_render_gbuffer). The several-GPU object has no gathered form: `shard` names the device whose own
    // tiles are delivered. GBufferInfo(): rt_get_gbuffer_info of that shard's last pass.
    struct GBuffer {
        std::vector<float> t;
        std::vector<int32_t> index;
        std::vector<rtm::vec4> point, normal, albedo;
    };
    GBuffer RenderGBuffer(unsigned int shard = 0);
    rt_gbuffer_info_t GBufferInfo(unsigned int shard = 0);

    // Ambient-occlusion frames (hip_raytracer.h, "ambient-occlusion frames"): `samples` (1, 2, 4 ... 64) occlusion rays per local
    // work-item from its primary hit, along the directions of its set of `dirs` (n_sets * samples entries, w ignored; a direction's
    // length is the occlusion radius) mirrored to the normal's side, started `bias` along the normal - the G-buffer pass and one
    // kernel. unoccluded: the rays that reached their end; ao = unoccluded / samples; a miss reads samples and 1. One entry per
    // work-item in the order Render() writes pixels; the frame is left alone. Synchronous (rt_render_ao); `shard` as RenderGBuffer's.
    // Throws on a scene with triangles. AOInfo(): rt_get_ao_info of that shard's last pass.
    struct AO {
        std::vector<uint8_t> unoccluded;
        std::vector<float> ao;
    };
    AO RenderAO(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias = 1e-3f, unsigned int shard = 0);
    rt_ao_info_t AOInfo(unsigned int shard = 0);

    // Filtered ambient occlusion (hip_raytracer.h, "filtered ambient occlusion"): an edge-aware box blur of the AO counts over a
    // (2 radius + 1)^2 window - a live item averages the live items of its window whose normal has a cosine >= normal_min with its own
    // and that lie within plane_max of its tangent plane. ao = sum / (taps * samples), grey the byte of "8-bit frames", taps the
    // accepted items; a dead item reads 1, 255 and 0. FilterAO: the pass alone on the caller's row-major array of `width` columns
    // (rt_ao_filter; index may be empty; the several-GPU object runs it on its first shard). RenderAOFiltered: RenderAO's passes and the
    // filter over the frame's sample grid with nothing copied back in between (rt_render_ao_filtered); it throws on the several-GPU
    // object, on rays from a plain buffer (no width) and on a scene with triangles. AOFilterInfo(): rt_get_ao_filter_info.
    struct FilteredAO {
        std::vector<float> ao;
        std::vector<uint8_t> grey, taps;
    };
    FilteredAO FilterAO(const std::vector<uint8_t>& unoccluded, const std::vector<rtm::vec4>& point, const std::vector<rtm::vec4>& normal,
                        const std::vector<int32_t>& index, size_t width, unsigned int samples, unsigned int radius, float normal_min,
                        float plane_max);
    FilteredAO RenderAOFiltered(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, unsigned int radius, float normal_min,
                                float plane_max);
    rt_ao_filter_info_t AOFilterInfo();

    rt_stats_t Stats();
    // rt_get_tiles_info: the screen tiles the next large-scene frame's primary round would use - the camera's (host-built) or, after
    // SetPose, the pose's (built on the GPU) - built now if the rays changed. The several-GPU object reports its first shard's.
    // (source 3: the table of a pose outside the grid's box, from spheres made for its origin - hip_raytracer.h, "outside the box")
    rt_tiles_info_t TilesInfo();
    // rt_get_rays_info: where the next frame's primary rays come from and whether the grid serves them - grid_in_use, and
    // primary_outside_box for a pose outside the grid's box whose tiles were accepted. The several-GPU object reports its first shard's.
    rt_rays_info_t RaysInfo();
    rt_context* Context() { return ctx; }

private:
    void Check(int rc, const char* method) const;  // throws "HIPRaytracer::<method>: " + the last error of ctx or of multi
    rt_context* ctx = nullptr;
    rt_multi* multi = nullptr;   // set instead of ctx by the several-GPU constructor
    unsigned int pose_width = 0; // the last SetPose's grid width (0: the rays in use are the camera's or a plain buffer)
};
