// CPURaytracer.cpp - see CPURaytracer.hpp. Own code: it shares nothing with oracle/ (the test-side checker) or with the
// HIP kernels; what it shares with both is the specification, i.e. the reference kernels' statements, cited inline as
// `.cl:<line>` = shade_and_reflect_kernel.cl (shade_kernel.cl / hittest_kernel.cl where they differ).
//
// Built with -ffp-contract=off: a multiply-add is fused exactly where fmuladd() is written (the sites the OpenCL
// front-end contracts, re-derived from the kernels' LLVM IR: in a*x + b*y + c*z + d*w the first product is fused onto
// the second), everything else rounds after every operation. dot() and normalize() are the plain left-to-right forms.
#include "CPURaytracer.hpp"

#include <stdexcept>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#define RT_INLINE inline __attribute__((always_inline))

// Per object, split by who reads it: the object loop streams `rows` + `type` for EVERY ray (52 of the record's 248 bytes -
// with 100 000 objects the loop is bound by how fast the cores can stream this array), everything else is touched once
// per finished ray.
struct CPURaytracer::Instance {
    float rows[3][4];  // rows x, y, z of mvInverse: rows[r] = (s_r, s_{4+r}, s_{8+r}, s_{12+r})
    int type;          // 0 sphere, 1 box, anything else: the kernels' switch has no case for it - never hit
};
struct CPURaytracer::Surface {
    float inv[16];     // mvInverse, column-major (s0..sF)
    float mv[16];
    float ambient[3], diffuse[3], specular[3];
    float absorption, shininess;
};

namespace {

struct F3 { float x, y, z; };
struct F4 { float x, y, z, w; };
struct Ray { F4 start, direction; };
struct Hit {
    float time;
    int index;
    F4 intersection;
    F3 normal, reflection;
};
struct Scene {
    const CPURaytracer::Instance* objs;
    const CPURaytracer::Surface* surf;
    size_t n_objs;
    const Light* lights;
    size_t n_lights;
};

RT_INLINE float fmuladd(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// transform() (.cl:60-65), one component: m[r]*v.x + m[4+r]*v.y + m[8+r]*v.z + m[12+r]*v.w
RT_INLINE float transform_row(const float* m, int r, const F4& v) {
    float t = m[4 + r] * v.y;
    t = fmuladd(m[r], v.x, t);
    t = fmuladd(m[8 + r], v.z, t);
    t = fmuladd(m[12 + r], v.w, t);
    return t;
}
RT_INLINE float row_of(const float* r, const F4& v) {  // the same component from a row stored contiguously
    float t = r[1] * v.y;
    t = fmuladd(r[0], v.x, t);
    t = fmuladd(r[2], v.z, t);
    t = fmuladd(r[3], v.w, t);
    return t;
}
RT_INLINE F4 transform(const float* m, const F4& v) {
    return F4{transform_row(m, 0, v), transform_row(m, 1, v), transform_row(m, 2, v), transform_row(m, 3, v)};
}
RT_INLINE float dot(const F3& a, const F3& b) {
    float s = a.x * b.x;
    s = s + a.y * b.y;
    s = s + a.z * b.z;
    return s;
}
RT_INLINE F3 normalize(const F3& v) {
    const float len = std::sqrt(dot(v, v));
    return F3{v.x / len, v.y / len, v.z / len};
}
// reflect() (.cl:68-70): incident - 2 dot(incident, normal) normal, the last step contracted
RT_INLINE F3 reflect(const F3& i, const F3& n) {
    const float k = dot(i, n) * -2.0f;
    return F3{fmuladd(k, n.x, i.x), fmuladd(k, n.y, i.y), fmuladd(k, n.z, i.z)};
}

// one slab of the unit box, intersectsWidthBoxSide() (.cl:33-58)
RT_INLINE bool box_side(float& tMin, float& tMax, float start, float dir) {
    float t1 = -0.5f - start;
    float t2 = 0.5f - start;
    if (dir == 0) {
        if (std::copysign(t1, t2) == t1) return false;  // both walls on the same side of the origin
        tMin = -MAX_FLOAT;
        tMax = MAX_FLOAT;
        return true;
    }
    t1 = t1 / dir;
    t2 = t2 / dir;
    if (dir < 0) { tMin = std::fmin(t1, t2); tMax = std::fmax(t1, t2); }
    else { tMin = t1; tMax = t2; }
    return true;
}

// The object loop of raycast() (.cl:72-171). The kernels rebuild the whole hit record on every improvement; only
// (time, object) decide the outcome, so the record is built once, after the loop, for the winner (finish_hit).
RT_INLINE void closest(const Scene& sc, const Ray& ray, float& time, int& index) {
    for (size_t k = 0; k < sc.n_objs; ++k) {
        const CPURaytracer::Instance& o = sc.objs[k];
        // transform(start), transform(direction) by mvInverse (.cl:78-79); the w components only matter to the hit record
        const F3 s{row_of(o.rows[0], ray.start), row_of(o.rows[1], ray.start), row_of(o.rows[2], ray.start)};
        const F3 d{row_of(o.rows[0], ray.direction), row_of(o.rows[1], ray.direction), row_of(o.rows[2], ray.direction)};
        if (o.type == 0) {  // unit sphere (.cl:82-121)
            float A = d.y * d.y; A = fmuladd(d.x, d.x, A); A = fmuladd(d.z, d.z, A);
            float B = s.y * d.y; B = fmuladd(d.x, s.x, B); B = fmuladd(d.z, s.z, B); B = B * 2.0f;
            float C = s.y * s.y; C = fmuladd(s.x, s.x, C); C = fmuladd(s.z, s.z, C); C = C + -1.0f;
            const float radical = fmuladd(B, B, (A * 4.0f) * (-C));
            if (radical < 0) continue;
            const float root = std::sqrt(radical);
            const float t1 = (-B - root) / (A * 2.0f);
            const float t2 = (-B + root) / (A * 2.0f);
            const float tMin = (t1 >= 0 && t2 >= 0) ? std::fmin(t1, t2) : std::fmax(t1, t2);
            if (tMin < 0) continue;
            if (time < tMin) continue;  // an equal time goes to the LATER sphere (.cl:108)
            time = tMin;
            index = (int)k;
        } else if (o.type == 1) {  // unit box (.cl:123-168)
            float txMin, txMax, tyMin, tyMax, tzMin, tzMax;
            if (!box_side(txMin, txMax, s.x, d.x)) continue;
            if (!box_side(tyMin, tyMax, s.y, d.y)) continue;
            if (!box_side(tzMin, tzMax, s.z, d.z)) continue;
            const float tMin = std::fmax(std::fmax(txMin, tyMin), tzMin);
            const float tMax = std::fmin(std::fmin(txMax, tyMax), tzMax);
            if (tMax < tMin) continue;
            const float tHit = (tMin >= 0 && tMax >= 0) ? std::fmin(tMin, tMax) : std::fmax(tMin, tMax);
            if (tHit < 0) continue;
            if (time <= tHit) continue;  // an equal time stays with the EARLIER object (.cl:147)
            time = tHit;
            index = (int)k;
        }
    }
}

// what raycast() leaves in the hit record for the winner (.cl:110-119 sphere, :149-166 box, :175 reflection)
RT_INLINE void finish_hit(const Scene& sc, const Ray& ray, Hit& h) {
    const CPURaytracer::Surface& o = sc.surf[h.index];
    const int type = sc.objs[h.index].type;
    const F4 s = transform(o.inv, ray.start), d = transform(o.inv, ray.direction);
    const F4 p{fmuladd(h.time, d.x, s.x), fmuladd(h.time, d.y, s.y), fmuladd(h.time, d.z, s.z), fmuladd(h.time, d.w, s.w)};
    F4 n{0.f, 0.f, 0.f, 0.f};
    if (type == 0) {
        n.x = p.x; n.y = p.y; n.z = p.z;
    } else {
        if (p.x > 0.4998f) n.x += 1.f; else if (p.x < -0.4998f) n.x -= 1.f;
        if (p.y > 0.4998f) n.y += 1.f; else if (p.y < -0.4998f) n.y -= 1.f;
        if (p.z > 0.4998f) n.z += 1.f; else if (p.z < -0.4998f) n.z -= 1.f;
    }
    h.intersection = transform(o.mv, p);
    const F4 nv = transform(o.mv, n);  // normals go through mv, not its inverse transpose (Q2)
    h.normal = normalize(F3{nv.x, nv.y, nv.z});
    h.reflection = reflect(F3{ray.direction.x, ray.direction.y, ray.direction.z}, h.normal);
}

// shade() / the body of __kernel shade (.cl:184-242, shade_kernel.cl:197-258). ACCUMULATE: shade_kernel.cl:252 sums the
// lights; shade_and_reflect's `fColor = ...` (.cl:238) keeps the last one. `specular` survives an iteration that is lit
// with nDotL <= 0 (Q1b).
template <bool ACCUMULATE>
RT_INLINE F3 shade(const Scene& sc, const Hit& hit, uint64_t& rays) {
    const CPURaytracer::Surface& mat = sc.surf[hit.index];
    const F3 P{hit.intersection.x, hit.intersection.y, hit.intersection.z};
    F3 color{0.f, 0.f, 0.f}, specular{0.f, 0.f, 0.f};
    for (size_t li = 0; li < sc.n_lights; ++li) {
        const Light& L = sc.lights[li];
        F3 lightVec;
        if (L.lightPosition.w != 0) lightVec = F3{L.lightPosition.x - P.x, L.lightPosition.y - P.y, L.lightPosition.z - P.z};
        else lightVec = F3{-L.lightPosition.x, -L.lightPosition.y, -L.lightPosition.z};
        // shadow ray: un-normalised direction, 0.01 of skin along it (.cl:201-205); a FULL closest-hit raycast (:209)
        const F3 nl = normalize(lightVec);
        Ray toLight;
        toLight.start = F4{fmuladd(nl.x, 0.01f, P.x), fmuladd(nl.y, 0.01f, P.y), fmuladd(nl.z, 0.01f, P.z), fmuladd(0.0f, 0.01f, 1.0f)};
        toLight.direction = F4{lightVec.x, lightVec.y, lightVec.z, 0.f};
        float st = MAX_FLOAT;
        int si = -1;
        closest(sc, toLight, st, si);
        rays += 1;
        const F3 normalView = normalize(hit.normal);  // (normalises an already normalised vector - the low bits move, Q12)
        const float nDotL = dot(normalView, nl);
        const F3 viewVec = normalize(F3{-P.x, -P.y, -P.z});
        const F3 reflectVec = normalize(reflect(F3{-nl.x, -nl.y, -nl.z}, normalView));
        const float rDotV = std::fmax(dot(reflectVec, viewVec), 0.0f);
        const F3 ambient{mat.ambient[0] * L.ambient.x, mat.ambient[1] * L.ambient.y, mat.ambient[2] * L.ambient.z};
        F3 diffuse;
        if (st >= 1.f || st < 0) {  // nothing between the point and the light (:229)
            const float nd = std::fmax(nDotL, 0.f);
            diffuse = F3{(mat.diffuse[0] * L.diffuse.x) * nd, (mat.diffuse[1] * L.diffuse.y) * nd, (mat.diffuse[2] * L.diffuse.z) * nd};
            if (nDotL > 0) {
                const float pw = std::pow(rDotV, std::fmax(mat.shininess, 1.f));
                specular = F3{(mat.specular[0] * L.specular.x) * pw, (mat.specular[1] * L.specular.y) * pw, (mat.specular[2] * L.specular.z) * pw};
            }
        } else {
            diffuse = F3{0.f, 0.f, 0.f};
            specular = F3{0.f, 0.f, 0.f};
        }
        if (ACCUMULATE) color = F3{((color.x + ambient.x) + diffuse.x) + specular.x, ((color.y + ambient.y) + diffuse.y) + specular.y, ((color.z + ambient.z) + diffuse.z) + specular.z};
        else color = F3{(ambient.x + diffuse.x) + specular.x, (ambient.y + diffuse.y) + specular.y, (ambient.z + diffuse.z) + specular.z};
    }
    return color;
}

// start = intersection + 0.001 normalize(reflection), direction = reflection (.cl:260-263, 275-277)
RT_INLINE Ray reflection_ray(const Hit& h) {
    const F3 n = normalize(h.reflection);
    Ray r;
    r.start = F4{fmuladd(n.x, 0.001f, h.intersection.x), fmuladd(n.y, 0.001f, h.intersection.y), fmuladd(n.z, 0.001f, h.intersection.z),
                 fmuladd(0.0f, 0.001f, h.intersection.w)};
    r.direction = F4{h.reflection.x, h.reflection.y, h.reflection.z, 0.f};
    return r;
}

// one work-item of the three kernels; false = the kernel returned without writing its output element
template <int KERNEL>
RT_INLINE bool work_item(const Scene& sc, const Ray3D& in, unsigned int max_bounces, float out[3], uint64_t& rays) {
    Ray ray;
    ray.start = F4{in.start.x, in.start.y, in.start.z, in.start.w};
    ray.direction = F4{in.direction.x, in.direction.y, in.direction.z, in.direction.w};
    Hit hit;
    hit.time = MAX_FLOAT;
    hit.index = -1;
    closest(sc, ray, hit.time, hit.index);
    rays += 1;
    // raycast()'s verdict: `time == MAX_FLOAT -> false` in shade_and_reflect (.cl:173), `time < MAX_FLOAT` in the two
    // older kernels (shade_kernel.cl:167, hittest_kernel.cl:149) - they part ways on a NaN time
    const bool is_hit = (KERNEL == 2) ? !(hit.time == MAX_FLOAT) : (hit.time < MAX_FLOAT);
    if (!is_hit) return false;
    if (KERNEL == 0) { out[0] = hit.time; return true; }
    finish_hit(sc, ray, hit);
    if (KERNEL == 1) {
        const F3 c = shade<true>(sc, hit, rays);
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
        return true;
    }
    // __kernel shade_and_reflect (.cl:253-284)
    const F3 first = shade<false>(sc, hit, rays);
    float absorptionPercent = sc.surf[hit.index].absorption;
    F3 absorbColor{first.x * absorptionPercent, first.y * absorptionPercent, first.z * absorptionPercent};
    F3 reflectColor{0.f, 0.f, 0.f};
    unsigned int bounces = max_bounces;
    Hit from = hit;
    // while (bounces-- > 0 && raycast(...) && absorptionPercent <= 0.999f)   - the unsigned post-decrement happens whether
    // or not the test passes, and the ray is cast before the absorption is looked at (Q8)
    for (;;) {
        const unsigned int before = bounces;
        bounces = bounces - 1u;
        if (!(before > 0u)) break;
        const Ray rr = reflection_ray(from);
        Hit rh;
        rh.time = MAX_FLOAT;
        rh.index = -1;
        closest(sc, rr, rh.time, rh.index);
        rays += 1;
        if (rh.time == MAX_FLOAT) break;
        if (!(absorptionPercent <= 0.999f)) break;
        finish_hit(sc, rr, rh);
        reflectColor = shade<false>(sc, rh, rays);
        const float reflectedAbsorption = (1.f - absorptionPercent) * sc.surf[rh.index].absorption;
        absorbColor = F3{fmuladd(reflectedAbsorption, reflectColor.x, absorbColor.x), fmuladd(reflectedAbsorption, reflectColor.y, absorbColor.y),
                         fmuladd(reflectedAbsorption, reflectColor.z, absorbColor.z)};
        absorptionPercent = absorptionPercent + reflectedAbsorption;
        from = rh;
    }
    if (bounces == 0u && absorptionPercent < 1.f) {  // (.cl:281-282) - only when the loop ended on its last permitted iteration
        const float w = 1.f - absorptionPercent;
        absorbColor = F3{fmuladd(w, reflectColor.x, absorbColor.x), fmuladd(w, reflectColor.y, absorbColor.y), fmuladd(w, reflectColor.z, absorbColor.z)};
    }
    out[0] = absorbColor.x; out[1] = absorbColor.y; out[2] = absorbColor.z;
    return true;
}

// a tile of consecutive work-items; compiled twice, the FMA3 clone is picked at load time where the CPU has it (the
// generic clone calls libm's fmaf: same bits, slower)
template <int KERNEL>
__attribute__((target_clones("fma", "default")))
void render_tile(const Scene& sc, const Ray3D* rays, size_t first, size_t last, unsigned int max_bounces, cl_float4* pixels,
                 uint64_t& traced, uint64_t& hits) {
    for (size_t i = first; i < last; ++i) {
        float out[3] = {0.f, 0.f, 0.f};
        if (work_item<KERNEL>(sc, rays[i], max_bounces, out, traced)) {
            hits += 1;
            if (KERNEL == 0) pixels[i].s[0] = out[0];
            else { pixels[i].s[0] = out[0]; pixels[i].s[1] = out[1]; pixels[i].s[2] = out[2]; pixels[i].s[3] = 1.0f; }
        }
    }
}

// the object loop alone for a tile of the caller's rays (CPURaytracer::QueryClosest); the clones as render_tile's
__attribute__((target_clones("fma", "default")))
void query_tile(const Scene& sc, const Ray3D* rays, size_t first, size_t last, float* t, int32_t* index) {
    for (size_t i = first; i < last; ++i) {
        Ray ray;
        ray.start = F4{rays[i].start.x, rays[i].start.y, rays[i].start.z, rays[i].start.w};
        ray.direction = F4{rays[i].direction.x, rays[i].direction.y, rays[i].direction.z, rays[i].direction.w};
        float time = MAX_FLOAT;
        int k = -1;
        closest(sc, ray, time, k);
        t[i] = time;
        index[i] = (time < MAX_FLOAT) ? k : -1;  // hittest's verdict (hittest_kernel.cl:149): a NaN time names nothing
    }
}

// the record stage for a tile of the caller's rays (CPURaytracer::HitRecords): finish_hit + reflection_ray for the winner index[i]
// at time t[i]; zero records where there is no winner. The clones as render_tile's.
__attribute__((target_clones("fma", "default")))
void record_tile(const Scene& sc, const Ray3D* rays, size_t first, size_t last, const float* t, const int32_t* index, rtm::vec4* point,
                 rtm::vec4* normal, Ray3D* reflected) {
    for (size_t i = first; i < last; ++i) {
        point[i] = rtm::vec4();
        normal[i] = rtm::vec4();
        reflected[i].start = rtm::vec4();
        reflected[i].direction = rtm::vec4();
        if (index[i] < 0 || (size_t)index[i] >= sc.n_objs) continue;
        Ray ray;
        ray.start = F4{rays[i].start.x, rays[i].start.y, rays[i].start.z, rays[i].start.w};
        ray.direction = F4{rays[i].direction.x, rays[i].direction.y, rays[i].direction.z, rays[i].direction.w};
        Hit h;
        h.time = t[i];
        h.index = index[i];
        finish_hit(sc, ray, h);
        const Ray r = reflection_ray(h);
        point[i] = rtm::vec4(h.intersection.x, h.intersection.y, h.intersection.z, h.intersection.w);
        normal[i] = rtm::vec4(h.normal.x, h.normal.y, h.normal.z, 0.f);
        reflected[i].start = rtm::vec4(r.start.x, r.start.y, r.start.z, r.start.w);
        reflected[i].direction = rtm::vec4(r.direction.x, r.direction.y, r.direction.z, r.direction.w);
    }
}

// one work-item per ray of the caller's (CPURaytracer::QueryShade): the pixel Render() would hold, and the primary (t, index) as the
// kernel takes them (a NaN time is a hit of shade_and_reflect only). A ray whose mask entry is negative reads as a miss. The clones
// as render_tile's.
template <int KERNEL>
__attribute__((target_clones("fma", "default")))
void shade_tile(const Scene& sc, const Ray3D* rays, const int32_t* mask, size_t first, size_t last, unsigned int max_bounces, rtm::vec4* rgba,
                float* t, int32_t* index, uint64_t& traced, uint64_t& hits, uint64_t& primaries) {
    for (size_t i = first; i < last; ++i) {
        rgba[i] = rtm::vec4(0.f, 0.f, 0.f, 1.f);
        t[i] = MAX_FLOAT;
        index[i] = -1;
        if (mask && mask[i] < 0) continue;
        primaries += 1;
        Ray ray;
        ray.start = F4{rays[i].start.x, rays[i].start.y, rays[i].start.z, rays[i].start.w};
        ray.direction = F4{rays[i].direction.x, rays[i].direction.y, rays[i].direction.z, rays[i].direction.w};
        float time = MAX_FLOAT;
        int k = -1;
        closest(sc, ray, time, k);
        t[i] = time;
        float out[3] = {0.f, 0.f, 0.f};
        if (work_item<KERNEL>(sc, rays[i], max_bounces, out, traced)) {
            hits += 1;
            index[i] = k;
            rgba[i] = rtm::vec4(out[0], out[1], out[2], 1.0f);
        }
    }
}

// what the kernels read of an object's two matrices: the surface's copies, and rows x, y, z of mvInverse for the object loop
void set_transform(CPURaytracer::Surface& d, CPURaytracer::Instance& h, const rtm::mat4& mv, const rtm::mat4& inv) {
    std::memcpy(d.inv, inv.data(), sizeof(d.inv));
    std::memcpy(d.mv, mv.data(), sizeof(d.mv));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) h.rows[r][c] = d.inv[4 * c + r];
}

void set_material(CPURaytracer::Surface& d, const Material& m) {  // what the kernels read of a material
    d.ambient[0] = m.ambient.x; d.ambient[1] = m.ambient.y; d.ambient[2] = m.ambient.z;
    d.diffuse[0] = m.diffuse.x; d.diffuse[1] = m.diffuse.y; d.diffuse[2] = m.diffuse.z;
    d.specular[0] = m.specular.x; d.specular[1] = m.specular.y; d.specular[2] = m.specular.z;
    d.absorption = m.absorption;
    d.shininess = m.shininess;
}

}  // namespace

CPURaytracer::CPURaytracer(const std::vector<ObjectData>& objects_, const std::vector<Light>& lights_, const std::vector<Ray3D>& rays_,
                           unsigned int MAX_BOUNCES, Kernel kernel_, unsigned int threads)
    : IRaytracer(objects_, lights_, rays_), max_bounces(MAX_BOUNCES), kernel(kernel_) {
    n_threads = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
    instances.resize(objects.size());
    surfaces.resize(objects.size());
    for (size_t i = 0; i < objects.size(); ++i) {  // what the reference's ctor does for the device (OpenCLRaytracer.cpp:16-24)
        const ObjectData& o = objects[i];
        Surface& d = surfaces[i];
        Instance& h = instances[i];
        set_transform(d, h, o.mv, o.mvInverse);
        set_material(d, o.mat);
        h.type = static_cast<int>(o.type);
    }
    pixels.resize(rays.size());
}

CPURaytracer::~CPURaytracer() {}

void CPURaytracer::SetSupersampling(unsigned int s, size_t sample_width) {
    if (s < 1 || s > 4) throw std::invalid_argument("the supersampling factor is 1, 2, 3 or 4");
    if (s > 1) {
        if (kernel == kHittest) throw std::invalid_argument("a time is not a colour: hittest frames are not filtered");
        if (sample_width == 0 || rays.size() % sample_width || sample_width % s || (rays.size() / sample_width) % s)
            throw std::invalid_argument("the rays must be whole rows of sample_width, width and height multiples of the factor");
    }
    ss = s;
    ss_width = sample_width;
}

void CPURaytracer::SetRays(const std::vector<Ray3D>& rays_) {
    if (rays_.size() != rays.size()) throw std::invalid_argument("SetRays: as many rays as the object was constructed with");
    own_rays = rays_;
    replaced = true;
}

void CPURaytracer::SetLights(const std::vector<Light>& lights_) {
    own_lights = lights_;
    lights_replaced = true;
}

void CPURaytracer::SetMaterials(uint32_t first, const std::vector<Material>& materials) {
    if ((uint64_t)first + materials.size() > surfaces.size()) throw std::invalid_argument("SetMaterials: first + count exceeds the object count");
    for (size_t i = 0; i < materials.size(); ++i) set_material(surfaces[first + i], materials[i]);
}

void CPURaytracer::SetTransforms(uint32_t first, const std::vector<Transform>& transforms) {
    if ((uint64_t)first + transforms.size() > surfaces.size()) throw std::invalid_argument("SetTransforms: first + count exceeds the object count");
    for (size_t i = 0; i < transforms.size(); ++i) set_transform(surfaces[first + i], instances[first + i], transforms[i].mv, transforms[i].mvInverse);
}

void CPURaytracer::SetVisibility(uint32_t first, const std::vector<uint8_t>& visible) {
    if ((uint64_t)first + visible.size() > instances.size()) throw std::invalid_argument("SetVisibility: first + count exceeds the object count");
    for (size_t i = 0; i < visible.size(); ++i) {
        const int created = static_cast<int>(objects[first + i].type);
        if (created > 1) continue;  // never hit as it is: left alone
        instances[first + i].type = visible[i] ? created : static_cast<int>(kTypeHidden);
    }
}

void CPURaytracer::SetPose(size_t width, size_t height, float z, const float m[9], const float origin[3]) {
    if (!m || !origin) throw std::invalid_argument("SetPose: the matrix or the origin is null");
    if (width > 0x1000000u || height > 0x1000000u || width * height != rays.size())
        throw std::invalid_argument("SetPose: width * height must be the number of rays the object was constructed with");
    std::vector<Ray3D> posed;
    posed.reserve(rays.size());
    const float half_w = (float)width / 2.0f, half_h = (float)height / 2.0f, height_f = (float)height;
    const rtm::vec3 start(origin[0], origin[1], origin[2]);
    for (size_t j = 0; j < height; ++j) {
        const float y = (height_f - (float)j) - half_h;
        for (size_t i = 0; i < width; ++i) {
            const float x = (float)i - half_w;
            float d[3];
            for (int r = 0; r < 3; ++r) {
                const float mx = m[3 * r] * x, my = m[3 * r + 1] * y, mz = m[3 * r + 2] * z;
                const float acc = mx + my;
                d[r] = acc + mz;
            }
            posed.emplace_back(start, rtm::vec3(d[0], d[1], d[2]));
        }
    }
    SetRays(posed);
}

void CPURaytracer::QueryClosest(const std::vector<Ray3D>& q, std::vector<float>& t, std::vector<int32_t>& index) const {
    const size_t n = q.size();
    t.assign(n, MAX_FLOAT);
    index.assign(n, -1);
    const Scene sc{instances.data(), surfaces.data(), instances.size(), nullptr, 0};
    const size_t tile = 256;
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const size_t first = next.fetch_add(tile);
            if (first >= n) break;
            query_tile(sc, q.data(), first, std::min(n, first + tile), t.data(), index.data());
        }
    };
    const unsigned int nt = (unsigned int)std::min<size_t>(n_threads, std::max<size_t>(1, (n + tile - 1) / tile));
    std::vector<std::thread> pool;
    for (unsigned int k = 1; k < nt; ++k) pool.emplace_back(worker);
    worker();
    for (std::thread& th : pool) th.join();
}

void CPURaytracer::QueryOccluded(const std::vector<Ray3D>& q, std::vector<uint8_t>& occluded) const {
    std::vector<float> t;
    std::vector<int32_t> index;
    QueryClosest(q, t, index);
    occluded.resize(q.size());
    for (size_t i = 0; i < q.size(); ++i) occluded[i] = (t[i] >= 1.f || t[i] < 0) ? 0 : 1;  // (.cl:229; a NaN reads occluded)
}

void CPURaytracer::HitRecords(const std::vector<Ray3D>& q, Hits& hits) const {
    const size_t n = q.size();
    if (hits.t.size() != n || hits.index.size() != n) throw std::invalid_argument("HitRecords: t and index must have one entry per ray");
    hits.point.assign(n, rtm::vec4());
    hits.normal.assign(n, rtm::vec4());
    hits.reflected.assign(n, Ray3D(rtm::vec3(0.f, 0.f, 0.f), rtm::vec3(0.f, 0.f, 0.f)));
    const Scene sc{instances.data(), surfaces.data(), instances.size(), nullptr, 0};
    record_tile(sc, q.data(), 0, n, hits.t.data(), hits.index.data(), hits.point.data(), hits.normal.data(), hits.reflected.data());
}

void CPURaytracer::QueryHits(const std::vector<Ray3D>& q, const std::vector<int32_t>& mask, Hits& hits) const {
    const size_t n = q.size();
    if (!mask.empty() && mask.size() != n) throw std::invalid_argument("QueryHits: the mask must be empty or have one entry per ray");
    QueryClosest(q, hits.t, hits.index);
    for (size_t i = 0; i < mask.size(); ++i)
        if (mask[i] < 0) { hits.t[i] = MAX_FLOAT; hits.index[i] = -1; }  // (not traced on the GPU; here the answer is dropped)
    HitRecords(q, hits);
}

void CPURaytracer::RenderGBuffer(GBuffer& out) const {
    Hits hits;
    QueryHits(Rays(), std::vector<int32_t>(), hits);
    const size_t n = hits.t.size();
    out.albedo.assign(n, rtm::vec4(0.f, 0.f, 0.f, 0.f));
    for (size_t i = 0; i < n; ++i) {
        const int32_t k = hits.index[i];
        if (k < 0 || (size_t)k >= surfaces.size()) continue;
        const Surface& s = surfaces[(size_t)k];
        out.albedo[i] = rtm::vec4(s.diffuse[0], s.diffuse[1], s.diffuse[2], 1.f);
    }
    out.t.swap(hits.t);
    out.index.swap(hits.index);
    out.point.swap(hits.point);
    out.normal.swap(hits.normal);
}

void CPURaytracer::RenderAO(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, AO& out) const {
    const unsigned int K = samples;
    if (K == 0 || K > 64 || (K & (K - 1))) throw std::invalid_argument("RenderAO: samples is one of 1, 2, 4, 8, 16, 32, 64");
    if (dirs.empty() || dirs.size() % K || dirs.size() / K > 4096) throw std::invalid_argument("RenderAO: dirs holds 1 .. 4096 whole sets of `samples` directions");
    if (!(bias >= 0.f) || !std::isfinite(bias)) throw std::invalid_argument("RenderAO: bias must be finite and not negative");
    const uint32_t n_sets = (uint32_t)(dirs.size() / K);
    GBuffer g;
    RenderGBuffer(g);
    const size_t n = g.t.size();
    std::vector<Ray3D> rays;
    std::vector<size_t> owner;   // the item of every traced ray
    for (size_t i = 0; i < n; ++i) {
        const rtm::vec4 &p = g.point[i], &nr = g.normal[i];
        const bool live = g.index[i] >= 0 && std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::isfinite(nr.x) &&
                          std::isfinite(nr.y) && std::isfinite(nr.z);
        if (!live) continue;
        const uint32_t h = (uint32_t)i * 0x9E3779B1u;
        const uint32_t set = (h >> 16) % n_sets;
        for (unsigned int k = 0; k < K; ++k) {
            rtm::vec4 d = dirs[(size_t)set * K + k];
            const float s = (d.x * nr.x + d.y * nr.y) + d.z * nr.z;   // (-ffp-contract=off: every product and sum rounded)
            if (s < 0.f) { d.x = -d.x; d.y = -d.y; d.z = -d.z; }
            rays.emplace_back(rtm::vec3(p.x + bias * nr.x, p.y + bias * nr.y, p.z + bias * nr.z), rtm::vec3(d.x, d.y, d.z));
            owner.push_back(i);
        }
    }
    std::vector<uint8_t> occluded;
    QueryOccluded(rays, occluded);
    out.unoccluded.assign(n, (uint8_t)K);
    for (size_t r = 0; r < rays.size(); ++r)
        if (occluded[r]) --out.unoccluded[owner[r]];
    const float inv_k = 1.0f / (float)K;
    out.ao.resize(n);
    for (size_t i = 0; i < n; ++i) out.ao[i] = (float)out.unoccluded[i] * inv_k;
}

void CPURaytracer::FilterAO(const std::vector<uint8_t>& unoccluded, const std::vector<rtm::vec4>& point, const std::vector<rtm::vec4>& normal,
                            const std::vector<int32_t>& index, size_t width, unsigned int samples, unsigned int radius, float normal_min,
                            float plane_max, FilteredAO& out) {
    const unsigned int K = samples;
    const size_t n = unoccluded.size();
    if (K == 0 || K > 64 || (K & (K - 1))) throw std::invalid_argument("FilterAO: samples is one of 1, 2, 4, 8, 16, 32, 64");
    if (radius < 1 || radius > 4) throw std::invalid_argument("FilterAO: radius is 1 .. 4");
    if (!(plane_max >= 0.f) || !std::isfinite(plane_max)) throw std::invalid_argument("FilterAO: plane_max must be finite and not negative");
    if (point.size() != n || normal.size() != n || (!index.empty() && index.size() != n))
        throw std::invalid_argument("FilterAO: unoccluded, point, normal and index have one entry per item");
    if (n != 0 && (width == 0 || n % width)) throw std::invalid_argument("FilterAO: the items are whole rows of `width`");
    out.ao.assign(n, 1.f);
    out.grey.assign(n, 255);
    out.taps.assign(n, 0);
    if (n == 0) return;
    const long rows = (long)(n / width), cols = (long)width, r = (long)radius;
    std::vector<uint8_t> live(n);
    for (size_t i = 0; i < n; ++i) {
        const rtm::vec4 &p = point[i], &nr = normal[i];
        live[i] = (index.empty() || index[i] >= 0) && std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::isfinite(nr.x) &&
                  std::isfinite(nr.y) && std::isfinite(nr.z);
    }
    for (long row = 0; row < rows; ++row)
        for (long col = 0; col < cols; ++col) {
            const size_t p = (size_t)row * width + (size_t)col;
            if (!live[p]) continue;
            const rtm::vec4 &pp = point[p], &np = normal[p];
            uint32_t taps = 1, sum = unoccluded[p];   // itself, untested
            for (long qr = std::max(0L, row - r); qr <= std::min(rows - 1, row + r); ++qr)
                for (long qc = std::max(0L, col - r); qc <= std::min(cols - 1, col + r); ++qc) {
                    const size_t q = (size_t)qr * width + (size_t)qc;
                    if (q == p || !live[q]) continue;
                    const rtm::vec4 &pq = point[q], &nq = normal[q];
                    const float c = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;   // (-ffp-contract=off: every product and sum rounded)
                    if (!(c >= normal_min)) continue;
                    const float dx = pq.x - pp.x, dy = pq.y - pp.y, dz = pq.z - pp.z;
                    const float e = (np.x * dx + np.y * dy) + np.z * dz;
                    if (!(std::fabs(e) <= plane_max)) continue;
                    ++taps;
                    sum += unoccluded[q];
                }
            const float a = (float)sum / (float)(taps * K);
            const float f = std::floor(a * 255.0f);
            out.ao[p] = a;
            out.grey[p] = !(f >= 0.f) ? 0 : (f >= 255.f ? 255 : (uint8_t)f);
            out.taps[p] = (uint8_t)taps;
        }
}

void CPURaytracer::RenderAOFiltered(const std::vector<rtm::vec4>& dirs, unsigned int samples, float bias, size_t width, unsigned int radius,
                                    float normal_min, float plane_max, FilteredAO& out) const {
    GBuffer g;
    RenderGBuffer(g);
    AO a;
    RenderAO(dirs, samples, bias, a);
    FilterAO(a.unoccluded, g.point, g.normal, g.index, width, samples, radius, normal_min, plane_max, out);
}

void CPURaytracer::QueryShade(const std::vector<Ray3D>& q, const std::vector<int32_t>& mask, Shade& out) const {
    const size_t n = q.size();
    if (!mask.empty() && mask.size() != n) throw std::invalid_argument("QueryShade: the mask must be empty or have one entry per ray");
    if (kernel == kHittest) throw std::invalid_argument("QueryShade: a time is not a colour (QueryClosest answers a hittest object)");
    out.rgba.assign(n, rtm::vec4(0.f, 0.f, 0.f, 1.f));
    out.t.assign(n, MAX_FLOAT);
    out.index.assign(n, -1);
    const Scene sc{instances.data(), surfaces.data(), instances.size(), Lights().data(), Lights().size()};
    const int32_t* m = mask.empty() ? nullptr : mask.data();
    const size_t tile = 64;
    std::atomic<size_t> next{0};
    std::atomic<uint64_t> total_rays{0}, total_hits{0}, total_primaries{0};
    auto worker = [&]() {
        uint64_t traced = 0, hits = 0, primaries = 0;
        for (;;) {
            const size_t first = next.fetch_add(tile);
            if (first >= n) break;
            const size_t last = std::min(n, first + tile);
            if (kernel == kShade) shade_tile<1>(sc, q.data(), m, first, last, max_bounces, out.rgba.data(), out.t.data(), out.index.data(), traced, hits, primaries);
            else shade_tile<2>(sc, q.data(), m, first, last, max_bounces, out.rgba.data(), out.t.data(), out.index.data(), traced, hits, primaries);
        }
        total_rays += traced;
        total_hits += hits;
        total_primaries += primaries;
    };
    const unsigned int nt = (unsigned int)std::min<size_t>(n_threads, std::max<size_t>(1, (n + tile - 1) / tile));
    std::vector<std::thread> pool;
    for (unsigned int k = 1; k < nt; ++k) pool.emplace_back(worker);
    worker();
    for (std::thread& th : pool) th.join();
    out.n_rays = total_primaries.load();
    out.rays_reference = total_rays.load();
    out.hit_rays = total_hits.load();
}

cl_float4* CPURaytracer::Render() {
    const std::vector<Ray3D>& rays = Rays();  // (the constructor's, or SetRays' copy: everything below reads these)
    const size_t n = rays.size();
    for (size_t i = 0; i < n; ++i) {  // the buffer as the reference uploads it: {0,0,0,1} (OpenCLRaytracer.cpp:32); hittest: "no hit"
        if (kernel == kHittest) pixels[i] = cl_float4{{MAX_FLOAT, 0.f, 0.f, 0.f}};
        else pixels[i] = cl_float4{{0.f, 0.f, 0.f, 1.f}};
    }
    const Scene sc{instances.data(), surfaces.data(), instances.size(), Lights().data(), Lights().size()};
    // row-tiles handed out from one counter: cost per tile varies with what the rays hit
    const size_t tile = std::max<size_t>(1, std::min<size_t>(256, n / ((size_t)n_threads * 8u)));
    std::atomic<size_t> next{0};
    std::atomic<uint64_t> total_rays{0}, total_hits{0};
    auto worker = [&]() {
        uint64_t traced = 0, hits = 0;
        for (;;) {
            const size_t first = next.fetch_add(tile);
            if (first >= n) break;
            const size_t last = std::min(n, first + tile);
            switch (kernel) {
                case kHittest: render_tile<0>(sc, rays.data(), first, last, max_bounces, pixels.data(), traced, hits); break;
                case kShade: render_tile<1>(sc, rays.data(), first, last, max_bounces, pixels.data(), traced, hits); break;
                default: render_tile<2>(sc, rays.data(), first, last, max_bounces, pixels.data(), traced, hits); break;
            }
        }
        total_rays += traced;
        total_hits += hits;
    };
    const unsigned int nt = (unsigned int)std::min<size_t>(n_threads, (n + tile - 1) / tile ? (n + tile - 1) / tile : 1);
    std::vector<std::thread> pool;
    for (unsigned int t = 1; t < nt; ++t) pool.emplace_back(worker);
    worker();
    for (std::thread& t : pool) t.join();
    rays_traced = total_rays.load();
    hit_pixels = total_hits.load();
    if (ss > 1) {  // the box filter of hip_raytracer.h: (b, a) order, every addition a rounded fp32 addition, one multiplication
        const size_t w = ss_width, pw = w / ss, ph = rays.size() / w / ss;
        const float k = 1.0f / (float)(ss * ss);
        filtered.resize(pw * ph);
        for (size_t j = 0; j < ph; ++j)
            for (size_t i = 0; i < pw; ++i) {
                const cl_float4* q = pixels.data() + j * ss * w + i * ss;
                cl_float4 acc = q[0];
                for (unsigned int b = 0; b < ss; ++b)
                    for (unsigned int a = 0; a < ss; ++a)
                        if (a | b)
                            for (int ch = 0; ch < 4; ++ch) acc.s[ch] = acc.s[ch] + q[b * w + a].s[ch];
                for (int ch = 0; ch < 4; ++ch) acc.s[ch] = acc.s[ch] * k;
                filtered[j * pw + i] = acc;
            }
        return filtered.data();
    }
    return pixels.data();
}
