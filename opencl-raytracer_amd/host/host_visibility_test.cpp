// host_visibility_test.cpp - replaceable visibility through the C++ flavour of the boundary (HIPRaytracer::SetVisibility):
//   host_visibility_test <scene.txt> <W> <H> <D> <mask.bin> <first> <out.bin>
// parses the scene, constructs the one-GPU and the several-GPU backend (two shards on device 0) with the W x H pinhole grid,
// renders, hides the objects first .. whose byte of mask.bin is 0, renders again and dumps the one-GPU frame (W * H float4) to
// out.bin. Prints one line per check for tests/test_host_visibility_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: host_visibility_test <scene.txt> <W> <H> <D> <mask.bin> <first> <out.bin>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]);
        const uint32_t first = (uint32_t)std::strtoul(argv[6], nullptr, 10);
        const size_t n = (size_t)width * height;
        std::vector<Ray3D> rays;
        rays.reserve(n);
        for (int jj = 0; jj < height; ++jj)
            for (int ii = 0; ii < width; ++ii)
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - width / 2.0f, (float)(height - jj) - height / 2.0f, -(float)height));
        std::vector<uint8_t> mask;
        {
            std::FILE* f = std::fopen(argv[5], "rb");
            if (!f) { std::printf("error cannot read %s\n", argv[5]); return 3; }
            uint8_t b;
            while (std::fread(&b, 1, 1, f) == 1) mask.push_back(b);
            std::fclose(f);
        }
        if ((size_t)first + mask.size() > objects.size()) { std::printf("error the range leaves the scene's %zu objects\n", objects.size()); return 3; }
        const std::vector<uint8_t> all_visible(mask.size(), 1), none_visible(mask.size(), 0);

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first_frame = raytracer->Render();
        std::vector<cl_float4> before(first_frame, first_frame + n);
        backend.SetVisibility(first, mask);
        const cl_float4* pixels = raytracer->Render();
        std::vector<cl_float4> after(pixels, pixels + n);
        std::printf("n_mask %zu\n", mask.size());
        std::printf("frames_differ %d\n", std::memcmp(before.data(), after.data(), sizeof(cl_float4) * n) != 0);
        bool reads_back = true;
        const std::vector<uint8_t> got = backend.ReadVisibility(0, (uint32_t)objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const bool in_range = i >= first && i < first + mask.size();
            reads_back = reads_back && got[i] == ((in_range && mask[i - first] == 0) ? 0 : 1);
        }
        std::printf("reads_back %d\n", reads_back);
        backend.SetVisibility(first, all_visible);  // ... and back: the constructor's frame
        const cl_float4* back = raytracer->Render();
        std::printf("back_to_first %d\n", std::memcmp(back, before.data(), sizeof(cl_float4) * n) == 0);
        backend.SetVisibility(first, none_visible);  // another way to the same mask
        (void)raytracer->Render();
        backend.SetVisibility(first, mask);
        const cl_float4* again = raytracer->Render();
        std::printf("history_free %d\n", std::memcmp(again, after.data(), sizeof(cl_float4) * n) == 0);
        bool refused = false;
        try { backend.SetVisibility((uint32_t)objects.size(), std::vector<uint8_t>(1, 0)); }
        catch (const std::exception&) { refused = true; }
        std::printf("range_refused %d\n", refused);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        two.SetVisibility(first, mask);
        const cl_float4* both = two.Render();
        std::printf("two_shards_same %d\n", std::memcmp(both, after.data(), sizeof(cl_float4) * n) == 0);

        std::FILE* f = std::fopen(argv[7], "wb");
        if (!f) return 3;
        std::fwrite(after.data(), sizeof(cl_float4), n, f);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
