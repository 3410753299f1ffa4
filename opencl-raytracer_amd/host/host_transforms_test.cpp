// host_transforms_test.cpp - replaceable transforms through the C++ flavour of the boundary (HIPRaytracer::SetTransforms):
//   host_transforms_test <scene.txt> <W> <H> <D> <transforms.bin> <first> <out.bin>
// parses the scene, constructs the one-GPU and the several-GPU backend (two shards on device 0) with the W x H pinhole grid,
// renders, moves objects first .. to the transforms of transforms.bin (records of 32 floats in rt_transform's layout: mv, then
// mvInverse, column-major), renders again and dumps the one-GPU frame (W * H float4) to out.bin. Prints one line per check for
// tests/test_host_transforms_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: host_transforms_test <scene.txt> <W> <H> <D> <transforms.bin> <first> <out.bin>\n"); return 1; }
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
        std::vector<Transform> moved;
        {
            std::FILE* f = std::fopen(argv[5], "rb");
            if (!f) { std::printf("error cannot read %s\n", argv[5]); return 3; }
            float rec[32];
            while (std::fread(rec, sizeof(float), 32, f) == 32) {
                Transform t;
                std::memcpy(t.mv.data(), rec, 64);
                std::memcpy(t.mvInverse.data(), rec + 16, 64);
                moved.push_back(t);
            }
            std::fclose(f);
        }
        if ((size_t)first + moved.size() > objects.size()) { std::printf("error the range leaves the scene's %zu objects\n", objects.size()); return 3; }
        std::vector<Transform> originals, others;
        for (size_t i = 0; i < moved.size(); ++i) {
            originals.push_back(Transform(objects[first + i].mv, objects[first + i].mvInverse));
            others.push_back(moved[moved.size() - 1 - i]);  // a third place: the new ones in reverse order
        }

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first_frame = raytracer->Render();
        std::vector<cl_float4> before(first_frame, first_frame + n);
        backend.SetTransforms(first, moved);
        const cl_float4* pixels = raytracer->Render();
        std::vector<cl_float4> after(pixels, pixels + n);
        std::printf("n_transforms %zu\n", moved.size());
        std::printf("frames_differ %d\n", std::memcmp(before.data(), after.data(), sizeof(cl_float4) * n) != 0);
        const rt_geometry_info_t info = backend.GeometryInfo();
        std::printf("grid_built %u\n", info.grid_built);
        std::printf("n_dynamic %u\n", info.n_dynamic);
        backend.SetTransforms(first, originals);  // ... and back: the constructor's frame
        const cl_float4* back = raytracer->Render();
        std::printf("back_to_first %d\n", std::memcmp(back, before.data(), sizeof(cl_float4) * n) == 0);
        backend.SetTransforms(first, others);  // another way to the same places
        (void)raytracer->Render();
        backend.SetTransforms(first, moved);
        const cl_float4* again = raytracer->Render();
        std::printf("history_free %d\n", std::memcmp(again, after.data(), sizeof(cl_float4) * n) == 0);
        std::printf("n_dynamic_after %u\n", backend.GeometryInfo().n_dynamic);
        bool refused = false;
        try { backend.SetTransforms((uint32_t)objects.size(), moved.empty() ? originals : std::vector<Transform>(1, moved[0])); }
        catch (const std::exception&) { refused = true; }
        std::printf("range_refused %d\n", moved.empty() || refused);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        two.SetTransforms(first, moved);
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
