// host_ao_filter_test.cpp - filtered ambient occlusion through the C++ flavour of the boundary (HIPRaytracer::RenderAOFiltered / FilterAO /
// AOFilterInfo):
//   host_ao_filter_test <scene.txt> <W> <H> <D> <K> <R> <NORMAL_MIN> <PLANE_MAX>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid and compares RenderAOFiltered of the two
// byte for byte (the default arithmetic is the CPU backend's) with host_ao_test's direction table (direction j is ((37 j) % 17 - 8,
// (53 j) % 19 - 9, (29 j) % 13 + 1) / 8: exact in float, the same in tests/test_host_ao_filter_gpu.py); once more with the middle object
// hidden on both; the pass alone (FilterAO) on the GPU backend's own G-buffer and counts against the frame form; that the frame is
// untouched; and that the several-GPU object refuses the frame form. Prints one line per check for tests/test_host_ao_filter_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

template <class A, class B>
static bool same(const A& a, const B& b) {
    return a.ao.size() == b.ao.size() && (a.ao.empty() || std::memcmp(a.ao.data(), b.ao.data(), a.ao.size() * sizeof(float)) == 0) &&
           a.grey == b.grey && a.taps == b.taps;
}

int main(int argc, char** argv) {
    if (argc < 9) { std::fprintf(stderr, "usage: host_ao_filter_test <scene.txt> <W> <H> <D> <K> <R> <NORMAL_MIN> <PLANE_MAX>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]), K = (unsigned)std::atoi(argv[5]), R = (unsigned)std::atoi(argv[6]);
        const float normal_min = (float)std::atof(argv[7]), plane_max = (float)std::atof(argv[8]);
        const size_t n = (size_t)width * height;
        std::vector<Ray3D> rays;
        rays.reserve(n);
        for (int jj = 0; jj < height; ++jj)
            for (int ii = 0; ii < width; ++ii)
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - width / 2.0f, (float)(height - jj) - height / 2.0f, -(float)height));
        const unsigned n_sets = 16;
        std::vector<rtm::vec4> dirs;
        for (unsigned j = 0; j < n_sets * K; ++j)
            dirs.emplace_back((float)((int)((37 * j) % 17) - 8) * 0.125f, (float)((int)((53 * j) % 19) - 9) * 0.125f, (float)((29 * j) % 13 + 1) * 0.125f, 0.f);
        const float bias = 1e-3f;

        HIPRaytracer gpu(objects, lights, rays, depth);
        CPURaytracer cpu(objects, lights, rays, depth);
        IRaytracer* raytracer = &gpu;
        const cl_float4* first_frame = raytracer->Render();
        const std::vector<cl_float4> before(first_frame, first_frame + n);

        for (int round = 0; round < 2; ++round) {
            const char* tag = round ? "changed_" : "";
            if (round && objects.size() > 1) {
                const uint32_t mid = (uint32_t)(objects.size() / 2);
                const std::vector<uint8_t> hide(1, 0);
                gpu.SetVisibility(mid, hide);
                cpu.SetVisibility(mid, hide);
            }
            const HIPRaytracer::FilteredAO g = gpu.RenderAOFiltered(dirs, K, bias, R, normal_min, plane_max);
            const rt_ao_filter_info_t info = gpu.AOFilterInfo();
            CPURaytracer::FilteredAO c;
            cpu.RenderAOFiltered(dirs, K, bias, (size_t)width, R, normal_min, plane_max, c);
            size_t taps = 0, grey = 0, blurred = 0;
            for (size_t i = 0; i < n; ++i) {
                taps += g.taps[i];
                grey += g.grey[i];
                blurred += g.taps[i] > 1;
            }
            std::printf("%ssame_as_cpu %d\n", tag, g.ao.size() == n && same(g, c));
            std::printf("%staps %zu\n", tag, taps);
            std::printf("%sgrey %zu\n", tag, grey);
            std::printf("%sblurred %zu\n", tag, blurred);
            std::printf("%sinfo %d\n", tag, info.n_items == n && info.accepted == taps && info.n_live > 0 && info.n_live <= n && info.filter_ms > 0.0 &&
                                                info.ao_ms > 0.0 && info.gbuffer_ms > 0.0 && gpu.AOInfo().n_items == n);
            // the pass alone on this backend's own records and counts
            const HIPRaytracer::GBuffer gb = gpu.RenderGBuffer();
            const HIPRaytracer::AO counts = gpu.RenderAO(dirs, K, bias);
            const HIPRaytracer::FilteredAO alone = gpu.FilterAO(counts.unoccluded, gb.point, gb.normal, gb.index, (size_t)width, K, R, normal_min, plane_max);
            const rt_ao_filter_info_t alone_info = gpu.AOFilterInfo();
            std::printf("%spass_alone_same %d\n", tag, same(alone, g) && alone_info.accepted == taps && alone_info.ao_ms == 0.0 && alone_info.gbuffer_ms == 0.0);
        }
        {
            HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
            bool refused = false;
            try {
                two.RenderAOFiltered(dirs, K, bias, R, normal_min, plane_max);
            } catch (const std::runtime_error&) { refused = true; }
            std::printf("two_shards_refused %d\n", refused);
        }
        if (objects.size() > 1) gpu.SetVisibility((uint32_t)(objects.size() / 2), std::vector<uint8_t>(1, 1));
        const cl_float4* again = raytracer->Render();
        std::printf("frame_untouched %d\n", std::memcmp(again, before.data(), sizeof(cl_float4) * n) == 0);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
