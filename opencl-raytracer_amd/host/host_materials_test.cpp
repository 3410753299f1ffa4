// host_materials_test.cpp - replaceable materials through the C++ flavour of the boundary (HIPRaytracer::SetMaterials):
//   host_materials_test <scene.txt> <W> <H> <D> <materials.bin> <first> <out.bin>
// parses the scene, constructs the one-GPU and the several-GPU backend (two shards on device 0) with the W x H pinhole grid,
// renders, replaces the materials of objects first .. by those of materials.bin (records of 16 floats in rt_material's layout:
// ambient rgb + pad, diffuse rgb + pad, specular rgb + pad, absorption, reflection, transparency, shininess), renders again and
// dumps the one-GPU frame (W * H float4) to out.bin. Prints one line per check for tests/test_host_materials_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: host_materials_test <scene.txt> <W> <H> <D> <materials.bin> <first> <out.bin>\n"); return 1; }
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
        std::vector<Material> replaced;
        {
            std::FILE* f = std::fopen(argv[5], "rb");
            if (!f) { std::printf("error cannot read %s\n", argv[5]); return 3; }
            float rec[16];
            while (std::fread(rec, sizeof(float), 16, f) == 16) {
                Material m;
                m.ambient = rtm::vec3(rec[0], rec[1], rec[2]);
                m.diffuse = rtm::vec3(rec[4], rec[5], rec[6]);
                m.specular = rtm::vec3(rec[8], rec[9], rec[10]);
                m.absorption = rec[12]; m.reflection = rec[13]; m.transparency = rec[14]; m.shininess = rec[15];
                replaced.push_back(m);
            }
            std::fclose(f);
        }
        if ((size_t)first + replaced.size() > objects.size()) { std::printf("error the range leaves the scene's %zu objects\n", objects.size()); return 3; }
        std::vector<Material> originals, others;
        for (size_t i = 0; i < replaced.size(); ++i) {
            originals.push_back(objects[first + i].mat);
            Material o = replaced[replaced.size() - 1 - i];  // a third set: the replaced ones in reverse order, fully absorbing
            o.absorption = 1.f;
            others.push_back(o);
        }

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first_frame = raytracer->Render();
        std::vector<cl_float4> before(first_frame, first_frame + n);
        backend.SetMaterials(first, replaced);
        const cl_float4* pixels = raytracer->Render();
        std::vector<cl_float4> after(pixels, pixels + n);
        std::printf("n_materials %zu\n", replaced.size());
        std::printf("frames_differ %d\n", std::memcmp(before.data(), after.data(), sizeof(cl_float4) * n) != 0);
        backend.SetMaterials(first, originals);  // ... and back: the constructor's frame
        const cl_float4* back = raytracer->Render();
        std::printf("back_to_first %d\n", std::memcmp(back, before.data(), sizeof(cl_float4) * n) == 0);
        backend.SetMaterials(first, others);  // another way to the same materials
        (void)raytracer->Render();
        backend.SetMaterials(first, replaced);
        const cl_float4* again = raytracer->Render();
        std::printf("history_free %d\n", std::memcmp(again, after.data(), sizeof(cl_float4) * n) == 0);
        bool refused = false;
        try { backend.SetMaterials((uint32_t)objects.size(), replaced.empty() ? originals : std::vector<Material>(1, replaced[0])); }
        catch (const std::exception&) { refused = true; }
        std::printf("range_refused %d\n", replaced.empty() || refused);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        two.SetMaterials(first, replaced);
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
