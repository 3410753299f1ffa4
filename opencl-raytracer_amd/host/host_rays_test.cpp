// host_rays_test.cpp - replaceable rays through the C++ flavour of the boundary (HIPRaytracer::SetRays):
//   host_rays_test <scene.txt> <W> <H> <D> <z-bits> <rays.bin> <out.bin>
// parses the scene, constructs the backend with the W x H pinhole grid at z (a float bit pattern, hex), renders, replaces the
// rays by the W * H records of 32 bytes in rays.bin, renders again and dumps that frame (W * H float4) to out.bin. Prints one line
// per check for tests/test_host_rays_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: host_rays_test <scene.txt> <W> <H> <D> <z-bits> <rays.bin> <out.bin>\n"); return 1; }
    try {
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[1], objects, lights);
        const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
        const unsigned depth = (unsigned)std::atoi(argv[4]);
        const size_t n = (size_t)width * height;
        float z;
        const uint32_t bits = (uint32_t)std::strtoul(argv[5], nullptr, 16);
        std::memcpy(&z, &bits, 4);
        std::vector<Ray3D> rays;
        rays.reserve(n);
        for (int jj = 0; jj < height; ++jj)
            for (int ii = 0; ii < width; ++ii)
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - width / 2.0f, (float)(height - jj) - height / 2.0f, z));
        static_assert(sizeof(Ray3D) == 32, "Ray3D is the 32-byte device record");
        std::vector<Ray3D> replaced(n, Ray3D(rtm::vec3(0, 0, 0), rtm::vec3(0, 0, 0)));
        std::FILE* f = std::fopen(argv[6], "rb");
        if (!f || std::fread(replaced.data(), sizeof(Ray3D), n, f) != n) { std::printf("error cannot read %s\n", argv[6]); return 3; }
        std::fclose(f);

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first = raytracer->Render();
        std::vector<cl_float4> before(first, first + n);
        rt_stats_t st = backend.Stats();
        std::printf("pinhole_before %u %u %u\n", st.pinhole, st.width, st.height);
        backend.SetRays(replaced);
        const cl_float4* pixels = raytracer->Render();
        st = backend.Stats();
        std::printf("pinhole_after %u %u %u\n", st.pinhole, st.width, st.height);
        std::printf("frames_differ %d\n", std::memcmp(before.data(), pixels, sizeof(cl_float4) * n) != 0);
        rt_rays_info_t info;
        if (rt_get_rays_info(backend.Context(), &info) != RT_OK) return 4;
        std::printf("source %u\n", info.source);
        bool refused = false;  // another count is refused and changes nothing
        try { backend.SetRays(std::vector<Ray3D>(n + 1, replaced[0])); } catch (const std::runtime_error&) { refused = true; }
        const cl_float4* again = raytracer->Render();
        std::printf("wrong_count_refused %d\n", refused && std::memcmp(again, pixels, sizeof(cl_float4) * n) == 0);
        f = std::fopen(argv[7], "wb");
        if (!f) return 3;
        std::fwrite(again, sizeof(cl_float4), n, f);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
