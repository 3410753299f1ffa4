// host_ao_test.cpp - ambient-occlusion frames through the C++ flavour of the boundary (HIPRaytracer::RenderAO / AOInfo):
//   host_ao_test <scene.txt> <W> <H> <D> <K>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid and compares the two results count for
// count (the default arithmetic is the CPU backend's) with a direction table of 16 sets made from small integers (direction j is
// ((37 j) % 17 - 8, (53 j) % 19 - 9, (29 j) % 13 + 1) / 8: exact in float, the same in tests/test_host_ao_gpu.py); once more with the
// middle object hidden on both; that the frame is untouched; and each shard of the two-shard object against its tiles of the whole
// (H a multiple of 16). Prints one line per check for tests/test_host_ao_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: host_ao_test <scene.txt> <W> <H> <D> <K>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]), K = (unsigned)std::atoi(argv[5]);
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

        HIPRaytracer::AO whole;
        for (int round = 0; round < 2; ++round) {
            const char* tag = round ? "changed_" : "";
            if (round && objects.size() > 1) {
                const uint32_t mid = (uint32_t)(objects.size() / 2);
                const std::vector<uint8_t> hide(1, 0);
                gpu.SetVisibility(mid, hide);
                cpu.SetVisibility(mid, hide);
            }
            const HIPRaytracer::AO g = gpu.RenderAO(dirs, K, bias);
            CPURaytracer::AO c;
            cpu.RenderAO(dirs, K, bias, c);
            const bool same = g.unoccluded == c.unoccluded && g.ao.size() == n && c.ao.size() == n &&
                              std::memcmp(g.ao.data(), c.ao.data(), n * sizeof(float)) == 0;
            size_t shaded = 0, sum = 0;
            for (size_t i = 0; i < n; ++i) {
                shaded += g.unoccluded[i] < K;
                sum += g.unoccluded[i];
            }
            std::printf("%ssame_as_cpu %d\n", tag, same);
            std::printf("%sshaded %zu\n", tag, shaded);
            std::printf("%ssum %zu\n", tag, sum);
            const rt_ao_info_t info = gpu.AOInfo();
            const rt_gbuffer_info_t gb = gpu.GBufferInfo();
            std::printf("%sinfo %d\n", tag, info.n_items == n && info.n_rays == (uint64_t)K * info.n_live && info.n_grid + info.n_brute == info.n_rays &&
                                                info.n_live > 0 && info.n_live <= gb.hits && info.ao_ms > 0.0 && info.gbuffer_ms > 0.0);
            if (round) whole = g;
        }
        // each shard of the several-GPU object delivers its own tiles of the whole (16-row tiles dealt round-robin)
        {
            HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
            if (objects.size() > 1) two.SetVisibility((uint32_t)(objects.size() / 2), std::vector<uint8_t>(1, 0));
            size_t total = 0;
            bool ok = true;
            const size_t tile = (size_t)16 * width;   // rt_create_multi's row tiles of a pinhole grid
            for (unsigned shard = 0; shard < 2; ++shard) {
                const HIPRaytracer::AO part = two.RenderAO(dirs, K, bias, shard);
                total += part.ao.size();
                for (size_t i = 0; i < part.ao.size() && ok; ++i) {
                    const size_t g = ((i / tile) * 2 + shard) * tile + i % tile;
                    if (g >= n) { ok = part.unoccluded[i] == K && part.ao[i] == 1.f; continue; }   // padding of a ragged last tile
                    ok = part.unoccluded[i] == whole.unoccluded[g] && part.ao[i] == whole.ao[g];
                }
                ok = ok && !part.ao.empty() && two.AOInfo(shard).n_items == part.ao.size();
            }
            std::printf("two_shards_same %d\n", ok && total >= n);
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
