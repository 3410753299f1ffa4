// host_query_test.cpp - ray queries through the C++ flavour of the boundary (HIPRaytracer::QueryClosest / QueryOccluded / Pick):
//   host_query_test <scene.txt> <W> <H> <D>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid, and asks both the same questions:
// the grid's own rays as a query, a few rays of another kind (from outside, NaN, zero direction), occlusion, and - on the GPU - Pick
// of work-items against the query of their rays; then the same once more with the middle object hidden on both. Prints one line
// per check for tests/test_host_query_gpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

// two backends' times: equal numbers, or NaN on both sides (a NaN's bits are the hardware's)
static bool same_times(const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(a[i] == b[i] || (std::isnan(a[i]) && std::isnan(b[i])))) return false;
    return true;
}
// one backend twice: the same bits
static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: host_query_test <scene.txt> <W> <H> <D>\n"); return 1; }
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
        // rays that are not the frame's: towards the origin from four sides, a NaN start, a zero direction, and unit-length
        // segments from the camera (occlusion: does the segment reach an object?)
        std::vector<Ray3D> other;
        const float far_ = 4.0f * (float)height;
        other.emplace_back(rtm::vec3(far_, 0, -(float)height), rtm::vec3(-1, 0, 0));
        other.emplace_back(rtm::vec3(-far_, 0, -(float)height), rtm::vec3(1, 0, 0));
        other.emplace_back(rtm::vec3(0, far_, -(float)height), rtm::vec3(0, -1, 0));
        other.emplace_back(rtm::vec3(0, 0, -far_), rtm::vec3(0, 0, 1));
        other.emplace_back(rtm::vec3(std::numeric_limits<float>::quiet_NaN(), 0, 0), rtm::vec3(0, 0, -1));
        other.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3(0, 0, 0));
        for (int k = 0; k < 32; ++k) other.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)(k - 16) * 4.0f, 0, -(float)(8 * k)));

        HIPRaytracer gpu(objects, lights, rays, depth);
        CPURaytracer cpu(objects, lights, rays, depth);
        IRaytracer* raytracer = &gpu;
        const cl_float4* first_frame = raytracer->Render();
        const std::vector<cl_float4> before(first_frame, first_frame + n);

        for (int round = 0; round < 2; ++round) {
            const char* tag = round ? "hidden_" : "";
            if (round && objects.size() > 1) {
                const std::vector<uint8_t> hide(1, 0);
                gpu.SetVisibility((uint32_t)(objects.size() / 2), hide);
                cpu.SetVisibility((uint32_t)(objects.size() / 2), hide);
            }
            std::vector<float> gt, ct, pt;
            std::vector<int32_t> gi, ci, pi;
            gpu.QueryClosest(rays, gt, gi);
            cpu.QueryClosest(rays, ct, ci);
            size_t hits = 0;
            for (size_t i = 0; i < n; ++i) hits += gi[i] >= 0;
            std::printf("%sframe_rays_t %d\n", tag, same_times(gt, ct));
            std::printf("%sframe_rays_index %d\n", tag, gi == ci);
            std::printf("%sframe_rays_hits %zu\n", tag, hits);
            std::vector<uint64_t> items;
            for (size_t i = 0; i < n; i += 7) items.push_back(i);
            items.push_back(n - 1);
            gpu.Pick(items, pt, pi);
            bool pick_ok = true;
            for (size_t k = 0; k < items.size(); ++k)
                pick_ok = pick_ok && std::memcmp(&pt[k], &gt[items[k]], 4) == 0 && pi[k] == gi[items[k]];
            std::printf("%spick %d\n", tag, pick_ok);
            gpu.QueryClosest(other, gt, gi);
            cpu.QueryClosest(other, ct, ci);
            std::printf("%sother_rays_t %d\n", tag, same_times(gt, ct));
            std::printf("%sother_rays_index %d\n", tag, gi == ci);
            std::vector<uint8_t> go, co;
            gpu.QueryOccluded(other, go);
            cpu.QueryOccluded(other, co);
            size_t blocked = 0;
            for (uint8_t b : go) blocked += b;
            std::printf("%soccluded %d\n", tag, go == co);
            std::printf("%soccluded_count %zu\n", tag, blocked);
            const rt_query_info_t info = gpu.QueryInfo();
            std::printf("%sinfo_rays %llu\n", tag, (unsigned long long)info.n_rays);
            std::printf("%sinfo_routes %d\n", tag, info.n_grid + info.n_brute == info.n_rays);
        }
        const std::vector<uint8_t> show(1, 1);
        if (objects.size() > 1) gpu.SetVisibility((uint32_t)(objects.size() / 2), show);
        const cl_float4* again = raytracer->Render();
        std::printf("frame_untouched %d\n", std::memcmp(again, before.data(), sizeof(cl_float4) * n) == 0);
        bool refused = false;
        try { std::vector<float> t; std::vector<int32_t> i; gpu.Pick(std::vector<uint64_t>(1, (uint64_t)n), t, i); }
        catch (const std::exception&) { refused = true; }
        std::printf("pick_refused %d\n", refused);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        std::vector<float> t1, t2;
        std::vector<int32_t> i1, i2;
        gpu.QueryClosest(rays, t1, i1);
        two.QueryClosest(rays, t2, i2);
        std::printf("two_shards_same %d\n", same_bits(t1, t2) && i1 == i2);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
