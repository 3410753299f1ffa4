// host_shade_test.cpp - shaded queries through the C++ flavour of the boundary (HIPRaytracer::QueryShade / PickColours / PickColour):
//   host_shade_test <scene.txt> <W> <H> <D>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid, renders the frame on the GPU and asks
// both backends for the colour along the grid's own rays: the GPU's answer is its own frame, bit for bit, and agrees with the CPU
// backend's (t and index exactly, |dRGB| <= 1e-5); then rays of the caller's own - the grid's, turned about the y axis - with every
// third one masked; PickColours / PickColour against the frame; and the first comparison once more with the middle object hidden and
// recoloured on both. Prints one line per check for tests/test_host_shade_gpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

static bool same_number(float a, float b) { return a == b || (std::isnan(a) && std::isnan(b)); }
static bool same_bits(const rtm::vec4& a, const cl_float4& b) { return std::memcmp(&a, b.s, 16) == 0; }
static double colour_error(const HIPRaytracer::Shade& g, const CPURaytracer::Shade& c) {
    double worst = 0.0;
    for (size_t i = 0; i < g.rgba.size(); ++i) {
        const float a[3] = {g.rgba[i].x, g.rgba[i].y, g.rgba[i].z}, b[3] = {c.rgba[i].x, c.rgba[i].y, c.rgba[i].z};
        for (int k = 0; k < 3; ++k) {
            const double d = std::fabs((double)a[k] - (double)b[k]);
            if (!(d <= worst)) worst = (std::isnan(a[k]) && std::isnan(b[k])) ? worst : (std::isnan(d) ? 1.0e30 : d);
        }
    }
    return worst;
}
static bool same_primary(const HIPRaytracer::Shade& g, const CPURaytracer::Shade& c) {
    if (g.t.size() != c.t.size() || g.index != c.index) return false;
    for (size_t i = 0; i < g.t.size(); ++i)
        if (!same_number(g.t[i], c.t[i])) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: host_shade_test <scene.txt> <W> <H> <D>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]);
        const size_t n = (size_t)width * height;
        std::vector<Ray3D> rays, turned;
        rays.reserve(n);
        turned.reserve(n);
        const float co = std::cos(0.2f), si = std::sin(0.2f);
        for (int jj = 0; jj < height; ++jj)
            for (int ii = 0; ii < width; ++ii) {
                const float x = (float)ii - width / 2.0f, y = (float)(height - jj) - height / 2.0f, z = -(float)height;
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3(x, y, z));
                turned.emplace_back(rtm::vec3(0.5f, 0.25f, 0.f), rtm::vec3(co * x + si * z, y, co * z - si * x));
            }

        HIPRaytracer gpu(objects, lights, rays, depth);
        CPURaytracer cpu(objects, lights, rays, depth);
        IRaytracer* raytracer = &gpu;
        const cl_float4* first_frame = raytracer->Render();
        const std::vector<cl_float4> before(first_frame, first_frame + n);

        for (int round = 0; round < 2; ++round) {
            const char* tag = round ? "changed_" : "";
            std::vector<cl_float4> frame = before;
            if (round && objects.size() > 1) {
                const uint32_t where = (uint32_t)(objects.size() / 2);
                Material m = objects[0].mat;
                m.diffuse = rtm::vec3(0.9f, 0.1f, 0.2f);
                gpu.SetVisibility(where, std::vector<uint8_t>(1, 0));
                cpu.SetVisibility(where, std::vector<uint8_t>(1, 0));
                gpu.SetMaterials(0, std::vector<Material>(1, m));
                cpu.SetMaterials(0, std::vector<Material>(1, m));
                const cl_float4* now = raytracer->Render();
                frame.assign(now, now + n);
                std::printf("changed_frame_differs %d\n", std::memcmp(frame.data(), before.data(), sizeof(cl_float4) * n) != 0);
            }
            const HIPRaytracer::Shade g = gpu.QueryShade(rays);
            CPURaytracer::Shade c;
            cpu.QueryShade(rays, std::vector<int32_t>(), c);
            bool is_frame = g.rgba.size() == n;
            size_t hits = 0;
            for (size_t i = 0; i < n && is_frame; ++i) { is_frame = same_bits(g.rgba[i], frame[i]); hits += g.index[i] >= 0; }
            std::printf("%sis_the_frame %d\n", tag, is_frame);
            std::printf("%shits %zu\n", tag, hits);
            std::printf("%sprimary %d\n", tag, same_primary(g, c));
            std::printf("%scolour_error %.3e\n", tag, colour_error(g, c));
            const rt_query_shade_info_t info = gpu.QueryShadeInfo();
            std::printf("%sinfo %d\n", tag, info.n_rays == n && info.n_grid + info.n_brute == n && info.hit_rays == c.hit_rays && info.rays_reference == c.rays_reference);
        }
        // rays of the caller's own, every third one masked
        std::vector<int32_t> mask(n, 0);
        for (size_t i = 0; i < n; i += 3) mask[i] = -1;
        const HIPRaytracer::Shade g = gpu.QueryShade(turned, mask);
        CPURaytracer::Shade c;
        cpu.QueryShade(turned, mask, c);
        bool masked_ok = true;
        size_t hits = 0;
        for (size_t i = 0; i < n; ++i) {
            if (mask[i] < 0) masked_ok = masked_ok && g.index[i] == -1 && g.t[i] == 3.402823466e+38f && g.rgba[i].x == 0.f && g.rgba[i].y == 0.f && g.rgba[i].z == 0.f && g.rgba[i].w == 1.f;
            hits += g.index[i] >= 0;
        }
        std::printf("own_primary %d\n", same_primary(g, c));
        std::printf("own_colour_error %.3e\n", colour_error(g, c));
        std::printf("own_hits %zu\n", hits);
        std::printf("masked %d\n", masked_ok && gpu.QueryShadeInfo().n_rays == n - (n + 2) / 3);

        const cl_float4* now = raytracer->Render();
        const std::vector<cl_float4> frame(now, now + n);
        std::vector<uint64_t> items;
        for (size_t i = 0; i < n; i += 7) items.push_back(i);
        items.push_back(n - 1);
        const HIPRaytracer::Shade p = gpu.PickColours(items);
        bool pick_ok = p.rgba.size() == items.size();
        for (size_t k = 0; k < items.size() && pick_ok; ++k) pick_ok = same_bits(p.rgba[k], frame[items[k]]);
        std::printf("pick_colours %d\n", pick_ok);
        const unsigned pi = (unsigned)(width / 2), pj = (unsigned)(height / 2);
        std::printf("pick_colour %d\n", same_bits(gpu.PickColour(pi, pj), frame[(size_t)pj * width + pi]));
        const cl_float4* again = raytracer->Render();
        std::printf("frame_after_picks %d\n", std::memcmp(again, frame.data(), sizeof(cl_float4) * n) == 0);
        bool refused = false;
        try { gpu.PickColours(std::vector<uint64_t>(1, (uint64_t)n)); }
        catch (const std::exception&) { refused = true; }
        std::printf("pick_refused %d\n", refused);
        bool mask_refused = false;
        try { gpu.QueryShade(rays, std::vector<int32_t>(3, 0)); }
        catch (const std::exception&) { mask_refused = true; }
        std::printf("mask_refused %d\n", mask_refused);
        bool hittest_refused = false;
        try { HIPRaytracer h(objects, lights, rays, depth, 0, 0, RT_KERNEL_HITTEST); h.QueryShade(rays); }
        catch (const std::exception&) { hittest_refused = true; }
        std::printf("hittest_refused %d\n", hittest_refused);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
