// CPURaytracer.hpp - a host-CPU backend behind the same IRaytracer boundary.
//
// The reference once had one: `new CPURaytracer(...)` survives as a comment next to the OpenCL backend's construction
// (OpenCL-Raytracer.cpp:74), and ObjectData::Raycast (ObjectData.cpp:12-133) is what is left of its ray tests. This
// class resurrects it as an in-repo baseline: plain C++ on std::thread, no GPU, no dependency on libhip_raytracer.
//
// Semantics are those of the KERNELS (shade_and_reflect_kernel.cl / shade_kernel.cl / hittest_kernel.cl), not of the
// ObjectData.cpp remnant, which disagrees with them: normals go through `mv` (Q2), equal hit times go to
// the later sphere / the earlier box (Q3), the box slab for a zero direction uses copysign (Q5), shade_and_reflect keeps
// the last light's colour with a possibly stale specular (Q1/Q1b), the bounce loop post-decrements an unsigned (Q8).
// Arithmetic: fp32, multiply-adds contracted exactly where the OpenCL front-end marks them (fmaf), IEEE sqrt / divide -
// the same contract as the HIP backend's default flavour, so the two backends can be compared pixel for pixel.
#pragma once

#include <cstdint>
#include <vector>

#include "IRaytracer.hpp"

class CPURaytracer : public IRaytracer {
public:
    enum Kernel { kHittest = 0, kShade = 1, kShadeAndReflect = 2 };

    // Same argument meaning as OpenCLRaytracer's ctor (OpenCLRaytracer.hpp:61); `threads` = 0 uses every hardware thread.
    CPURaytracer(const std::vector<ObjectData>& objects, const std::vector<Light>& lights, const std::vector<Ray3D>& rays,
                 unsigned int MAX_BOUNCES, Kernel kernel = kShadeAndReflect, unsigned int threads = 0);

    // Inherited via IRaytracer. Synchronous; one float4 per ray, owned by this object, overwritten by the next call.
    // shade / shade_and_reflect: RGB in s[0..2]; pixels whose primary ray misses keep the reference's upload-time
    // value {0,0,0,1} (OpenCLRaytracer.cpp:32). hittest: nearest t in s[0] (MAX_FLOAT on a miss).
    cl_float4* Render() override;

    // Supersampled frames (hip_raytracer.h, "supersampled frames"), the same option as HIPRaytracer's so that the two backends
    // stay interchangeable: the rays are the SAMPLE grid, rows of `sample_width`; Render() then returns Pixels() = rays / s^2
    // pixels, the s x s samples of each added in fp32 in (b, a) order and multiplied once by fl(1 / s^2) - the same loop on the
    // host. s = 1 (the default) is off. Throws std::invalid_argument for what rt_set_supersampling refuses.
    void SetSupersampling(unsigned int s, size_t sample_width);
    size_t Pixels() const { return Rays().size() / ((size_t)ss * ss); }

    // Replaceable rays, the same option as HIPRaytracer's: the next Render() traces a copy of `rays` - as many as the object was
    // constructed with, std::invalid_argument otherwise - instead of the constructor's.
    void SetRays(const std::vector<Ray3D>& rays);

    // Posed cameras, the same option as HIPRaytracer's: the pinhole grid (width, height, z) seen through the fp32 matrix m
    // (row-major) from `origin`, built here in the float order hip_raytracer.h states ("posed cameras": every product and sum
    // rounded, nothing fused - this library is built with -ffp-contract=off) and handed to SetRays. width * height must be the
    // number of rays the object was constructed with; std::invalid_argument otherwise.
    void SetPose(size_t width, size_t height, float z, const float m[9], const float origin[3]);

    // Replaceable lights, the same option as HIPRaytracer's: the next Render() lights the scene with a copy of `lights` - any count -
    // instead of the constructor's. Only the array is replaced.
    void SetLights(const std::vector<Light>& lights);

    // Replaceable materials, the same option as HIPRaytracer's: the next Render() shades objects first .. first + n - 1 with
    // `materials` instead of the constructor's; geometry stays. std::invalid_argument for a range beyond the objects.
    void SetMaterials(uint32_t first, const std::vector<Material>& materials);

    // Replaceable transforms, the same option as HIPRaytracer's: the next Render() has objects first .. first + n - 1 where these
    // mv / mvInverse put them; materials and type stay. std::invalid_argument for a range beyond the objects.
    void SetTransforms(uint32_t first, const std::vector<Transform>& transforms);

    // Replaceable visibility, the same option as HIPRaytracer's: the next Render() does not hit objects first .. first + n - 1 whose
    // entry of `visible` is 0 (their type becomes kTypeHidden), and hits the others as the constructor's type says.
    // std::invalid_argument for a range beyond the objects.
    void SetVisibility(uint32_t first, const std::vector<uint8_t>& visible);

    // Ray queries, the same option as HIPRaytracer's (hip_raytracer.h, "ray queries"), and its executable definition without a GPU:
    // the reference's object loop over the CURRENT objects (SetTransforms and SetVisibility as set so far) for rays of the caller's
    // own, any number of them. t[i] is the loop's time - MAX_FLOAT on a miss, NaN where the loop ends with NaN - and index[i] the
    // winner where t[i] < MAX_FLOAT, else -1; occluded[i] = !(t >= 1 || t < 0), the kernels' shadow predicate (.cl:229). Lights,
    // materials, MAX_BOUNCES and the frame's rays do not enter; Render() is not disturbed.
    void QueryClosest(const std::vector<Ray3D>& rays, std::vector<float>& t, std::vector<int32_t>& index) const;
    void QueryOccluded(const std::vector<Ray3D>& rays, std::vector<uint8_t>& occluded) const;

    // Hit-record queries, the same option as HIPRaytracer's (hip_raytracer.h, "hit-record queries"), and its executable definition
    // in the default arithmetic: QueryClosest's (t, index) and, where index >= 0, what raycast() leaves in the HitRecord of that
    // winner at that time - finish_hit() and reflection_ray(), the functions Render() uses - one entry per ray. point:
    // HitRecord.intersection; normal: HitRecord.normal in xyz, w = 0; reflected: the next ray of the reflection chain. Where
    // index == -1 (a miss, a NaN time, a ray whose `mask` entry is negative: not traced, t = MAX_FLOAT) the records are zero.
    // `mask` is empty or one entry per ray (std::invalid_argument otherwise).
    struct Hits {
        std::vector<float> t;
        std::vector<int32_t> index;
        std::vector<rtm::vec4> point, normal;
        std::vector<Ray3D> reflected;
    };
    void QueryHits(const std::vector<Ray3D>& rays, const std::vector<int32_t>& mask, Hits& hits) const;
    // The record stage alone, for a winner and a time of the caller's: point / normal / reflected of `hits` from its t and index
    // (sized as `rays`; an index that is negative or beyond the objects gives zero records).
    void HitRecords(const std::vector<Ray3D>& rays, Hits& hits) const;

    // Shaded queries, the same option as HIPRaytracer's (hip_raytracer.h, "shaded queries"), and the definition that runs without a
    // GPU: per ray of the caller's own - any number - the pixel Render() would hold for it (rgba; a miss is {0,0,0,1}) and the
    // primary (t, index) as this object's kernel takes them (a NaN time is a hit for shade_and_reflect, a miss for shade), over the
    // CURRENT objects, materials and lights (the setters as called so far). A ray whose `mask` entry is negative reads as a miss
    // (t = MAX_FLOAT, index -1) and is not counted. `mask` is empty or one entry per ray; std::invalid_argument otherwise and for a
    // hittest object. Render() is not disturbed. n_rays: traced primary rays; rays_reference: every ray of their paths, as
    // RaysTraced() counts a frame; hit_rays as HitPixels().
    struct Shade {
        std::vector<rtm::vec4> rgba;
        std::vector<float> t;
        std::vector<int32_t> index;
        uint64_t n_rays = 0, rays_reference = 0, hit_rays = 0;
    };
    void QueryShade(const std::vector<Ray3D>& rays, const std::vector<int32_t>& mask, Shade& out) const;

    // G-buffer frames, the same option as HIPRaytracer's (hip_raytracer.h, "G-buffer frames"), and the definition that runs without a
    // GPU: QueryHits over this object's own primary rays (SetRays / SetPose as set so far), one entry per ray in ray order, and the
    // winner's diffuse colour with w = 1 as `albedo` (SetMaterials as set so far); zero records where index == -1. No triangles
    // here, as everywhere in this backend. Render() is not disturbed.
    struct GBuffer {
        std::vector<float> t;
        std::vector<int32_t> index;
        std::vector<rtm::vec4> point, normal, albedo;
    };
    void RenderGBuffer(GBuffer& out) const;

    // Ambient-occlusion frames, the same option as HIPRaytracer's (hip_raytracer.h, "ambient-occlusion frames"), as the composition it
    // is defined as: RenderGBuffer, then per live item (index >= 0, finite point and normal) `samples` rays - set (h >> 16) % n_sets
    // with h = (uint32)i * 0x9E3779B1; d = dirs[set * samples + k], negated where (d.x n.x + d.y n.y) + d.z n.z < 0; start = p +
    // (bias * n), float, product then sum - through QueryOccluded; unoccluded = samples - the occluded ones, ao = unoccluded *
    // (1.0f / samples); a dead item reads samples and 1. std::invalid_argument for another `samples` than 1, 2, 4 ... 64, a table
    // that is no 1 .. 4096 whole sets, a bias that is negative or not finite.
    struct AO {
        std::vector<uint8_t> unoccluded;
        std::vector<float> ao;
    };
    void RenderAO(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, AO& out) const;

    // Filtered ambient occlusion (hip_raytracer.h, "filtered ambient occlusion"), a second statement of ao.py's filter() in plain loops:
    // a row-major array of `width` columns (n = unoccluded.size() a multiple of it); index may be empty (every item may be live). A live
    // item p (index >= 0, finite point and normal) accepts itself and every live q != p of its (2 radius + 1)^2 window inside the array
    // with (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_min and |(n_p.x d.x + n_p.y d.y) + n_p.z d.z| <= plane_max, d = P_q - P_p,
    // float, product then sum; taps = the accepted items, ao = (float)sum of their counts / (float)(taps * samples), grey the byte of
    // "8-bit frames"; a dead item reads 0, 1 and 255. std::invalid_argument for another `samples` than 1, 2, 4 ... 64, a radius outside
    // 1 .. 4, a plane_max that is negative or not finite, arrays of different lengths or a width that does not divide them.
    struct FilteredAO {
        std::vector<float> ao;
        std::vector<uint8_t> grey, taps;
    };
    static void FilterAO(const std::vector<uint8_t>& unoccluded, const std::vector<rtm::vec4>& point, const std::vector<rtm::vec4>& normal,
                         const std::vector<int32_t>& index, size_t width, unsigned int samples, unsigned int radius, float normal_min,
                         float plane_max, FilteredAO& out);
    // RenderGBuffer and RenderAO, then FilterAO over rows of `width` work-items: what HIPRaytracer::RenderAOFiltered is defined as.
    void RenderAOFiltered(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, size_t width, unsigned int radius,
                          float normal_min, float plane_max, FilteredAO& out) const;

    uint64_t RaysTraced() const { return rays_traced; }   // primary + shadow + reflection rays of the last Render()
    uint64_t HitPixels() const { return hit_pixels; }
    unsigned int Threads() const { return n_threads; }

    struct Instance;  // per object: what the object loop streams for every ray (built once by the ctor)
    struct Surface;   // per object: what a finished ray needs (matrices, material)

private:
    unsigned int max_bounces;
    Kernel kernel;
    unsigned int n_threads;
    std::vector<Instance> instances;
    std::vector<Surface> surfaces;
    std::vector<cl_float4> pixels;
    unsigned int ss = 1;                // supersampling factor; > 1: Render() returns `filtered`
    size_t ss_width = 0;
    std::vector<cl_float4> filtered;
    uint64_t rays_traced = 0, hit_pixels = 0;
    std::vector<Ray3D> own_rays;        // SetRays' copy; empty: the constructor's rays (IRaytracer holds them by reference)
    bool replaced = false;
    const std::vector<Ray3D>& Rays() const { return replaced ? own_rays : rays; }
    std::vector<Light> own_lights;      // SetLights' copy (IRaytracer holds the constructor's by reference)
    bool lights_replaced = false;
    const std::vector<Light>& Lights() const { return lights_replaced ? own_lights : lights; }

public:
    ~CPURaytracer() override;
};
