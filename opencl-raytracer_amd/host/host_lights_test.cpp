// host_lights_test.cpp - replaceable lights through the C++ flavour of the boundary (HIPRaytracer::SetLights):
//   host_lights_test <scene.txt> <W> <H> <D> <lights.bin> <out.bin>
// parses the scene, constructs the one-GPU and the several-GPU backend (two shards on device 0) with the W x H pinhole grid,
// renders, replaces the lights by those of lights.bin (records of 7 floats: x y z w of the position, then one grey level each for
// ambient, diffuse and specular), renders again and dumps the one-GPU frame (W * H float4) to out.bin. Prints one line per check
// for tests/test_host_lights_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: host_lights_test <scene.txt> <W> <H> <D> <lights.bin> <out.bin>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]);
        const size_t n = (size_t)width * height;
        std::vector<Ray3D> rays;
        rays.reserve(n);
        for (int jj = 0; jj < height; ++jj)
            for (int ii = 0; ii < width; ++ii)
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - width / 2.0f, (float)(height - jj) - height / 2.0f, -(float)height));
        std::vector<Light> replaced;
        {
            std::FILE* f = std::fopen(argv[5], "rb");
            if (!f) { std::printf("error cannot read %s\n", argv[5]); return 3; }
            float rec[7];
            while (std::fread(rec, sizeof(float), 7, f) == 7) {
                LightProperties props;
                props.ambient = rtm::vec3(rec[4], rec[4], rec[4]);
                props.diffuse = rtm::vec3(rec[5], rec[5], rec[5]);
                props.specular = rtm::vec3(rec[6], rec[6], rec[6]);
                Light l(props, rtm::mat4(1.0f));
                l.lightPosition = rtm::vec4(rec[0], rec[1], rec[2], rec[3]);
                replaced.push_back(l);
            }
            std::fclose(f);
        }

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first = raytracer->Render();
        std::vector<cl_float4> before(first, first + n);
        backend.SetLights(replaced);
        const cl_float4* pixels = raytracer->Render();
        std::vector<cl_float4> after(pixels, pixels + n);
        std::printf("n_lights %zu\n", replaced.size());
        std::printf("frames_differ %d\n", std::memcmp(before.data(), after.data(), sizeof(cl_float4) * n) != 0);
        const rt_light_tiles_info_t info = backend.LightTilesInfo();
        std::printf("tiles %u %u %u\n", info.enabled, info.source, info.refused);
        backend.SetLights(lights);  // ... and back: the constructor's frame
        const cl_float4* back = raytracer->Render();
        std::printf("back_to_first %d\n", std::memcmp(back, before.data(), sizeof(cl_float4) * n) == 0);
        backend.SetLights(std::vector<Light>());  // no lights at all is a frame too
        (void)raytracer->Render();
        backend.SetLights(replaced);
        const cl_float4* again = raytracer->Render();
        std::printf("history_free %d\n", std::memcmp(again, after.data(), sizeof(cl_float4) * n) == 0);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        two.SetLights(replaced);
        const cl_float4* both = two.Render();
        std::printf("two_shards_same %d\n", std::memcmp(both, after.data(), sizeof(cl_float4) * n) == 0);

        std::FILE* f = std::fopen(argv[6], "wb");
        if (!f) return 3;
        std::fwrite(after.data(), sizeof(cl_float4), n, f);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
