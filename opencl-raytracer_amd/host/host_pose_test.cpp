// host_pose_test.cpp - posed cameras through the C++ flavour of the boundary (HIPRaytracer::SetPose):
//   host_pose_test <scene.txt> <W> <H> <D> <z-bits> <pose.bin> <out.bin>
// parses the scene, constructs the one-GPU and the several-GPU backend (two shards on device 0) with the W x H pinhole grid at z
// (a float bit pattern, hex), renders, sets the pose of pose.bin (12 floats: the matrix row-major, then the origin), renders again
// and dumps the one-GPU frame (W * H float4) to out.bin. Prints one line per check for tests/test_host_pose_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: host_pose_test <scene.txt> <W> <H> <D> <z-bits> <pose.bin> <out.bin>\n"); return 1; }
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
        float pose[12];
        std::FILE* f = std::fopen(argv[6], "rb");
        if (!f || std::fread(pose, sizeof(float), 12, f) != 12) { std::printf("error cannot read %s\n", argv[6]); return 3; }
        std::fclose(f);

        HIPRaytracer backend(objects, lights, rays, depth);
        IRaytracer* raytracer = &backend;
        const cl_float4* first = raytracer->Render();
        std::vector<cl_float4> before(first, first + n);
        backend.SetPose((unsigned)width, (unsigned)height, z, pose, pose + 9);
        const cl_float4* pixels = raytracer->Render();
        std::vector<cl_float4> posed(pixels, pixels + n);
        const rt_stats_t st = backend.Stats();
        std::printf("pinhole_after %u %u %u\n", st.pinhole, st.width, st.height);
        std::printf("frames_differ %d\n", std::memcmp(before.data(), posed.data(), sizeof(cl_float4) * n) != 0);
        rt_rays_info_t info;
        if (rt_get_rays_info(backend.Context(), &info) != RT_OK) return 4;
        std::printf("source %u\n", info.source);
        bool refused = false;  // another grid size is refused and changes nothing
        try { backend.SetPose((unsigned)width + 1, (unsigned)height, z, pose, pose + 9); } catch (const std::runtime_error&) { refused = true; }
        const cl_float4* again = raytracer->Render();
        std::printf("wrong_size_refused %d\n", refused && std::memcmp(again, posed.data(), sizeof(cl_float4) * n) == 0);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        two.SetPose((unsigned)width, (unsigned)height, z, pose, pose + 9);
        const cl_float4* both = two.Render();
        std::printf("two_shards_same %d\n", std::memcmp(both, posed.data(), sizeof(cl_float4) * n) == 0);

        f = std::fopen(argv[7], "wb");
        if (!f) return 3;
        std::fwrite(posed.data(), sizeof(cl_float4), n, f);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
