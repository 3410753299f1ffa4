// host_hits_test.cpp - hit-record queries through the C++ flavour of the boundary (HIPRaytracer::QueryHits / PickHits / PickHit):
//   host_hits_test <scene.txt> <W> <H> <D>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid, and asks both for the records of the
// grid's own rays, then follows the reflection chain for two more bounces with the mask on both; on the GPU, PickHits / PickHit of
// work-items against the query of their rays; then the same once more with the middle object hidden on both. The default arithmetic
// is the CPU backend's, so the records are compared number for number (a NaN on both sides counts as equal: its bits are the
// hardware's). Prints one line per check for tests/test_host_hits_gpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "SceneLoader.hpp"

static bool same_number(float a, float b) { return a == b || (std::isnan(a) && std::isnan(b)); }
static bool same_vec(const rtm::vec4& a, const rtm::vec4& b) {
    return same_number(a.x, b.x) && same_number(a.y, b.y) && same_number(a.z, b.z) && same_number(a.w, b.w);
}
// the GPU's records against the CPU backend's, field by field
template <class A, class B>
static bool same_hits(const A& g, const B& c) {
    const size_t n = g.t.size();
    if (c.t.size() != n || g.index != c.index || g.point.size() != n || c.point.size() != n || g.normal.size() != n || c.normal.size() != n ||
        g.reflected.size() != n || c.reflected.size() != n)
        return false;
    for (size_t i = 0; i < n; ++i)
        if (!same_number(g.t[i], c.t[i]) || !same_vec(g.point[i], c.point[i]) || !same_vec(g.normal[i], c.normal[i]) ||
            !same_vec(g.reflected[i].start, c.reflected[i].start) || !same_vec(g.reflected[i].direction, c.reflected[i].direction))
            return false;
    return true;
}
static bool zero_vec(const rtm::vec4& v) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    return std::memcmp(&v, zero, 16) == 0;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: host_hits_test <scene.txt> <W> <H> <D>\n"); return 1; }
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
            // three bounces of the chain on both backends, each bounce masked by the one before
            HIPRaytracer::Hits g = gpu.QueryHits(rays);
            CPURaytracer::Hits c;
            cpu.QueryHits(rays, std::vector<int32_t>(), c);
            const HIPRaytracer::Hits first = g;
            size_t hits = 0;
            for (size_t i = 0; i < n; ++i) hits += g.index[i] >= 0;
            std::printf("%sbounce1 %d\n", tag, same_hits(g, c));
            std::printf("%sbounce1_hits %zu\n", tag, hits);
            bool zero_ok = true;
            for (size_t i = 0; i < n; ++i)
                if (g.index[i] < 0) zero_ok = zero_ok && zero_vec(g.point[i]) && zero_vec(g.normal[i]) && zero_vec(g.reflected[i].start) && zero_vec(g.reflected[i].direction);
            std::printf("%smisses_zero %d\n", tag, zero_ok);
            for (int bounce = 2; bounce <= 3; ++bounce) {
                const size_t traced = hits;
                const HIPRaytracer::Hits gn = gpu.QueryHits(g.reflected, g.index);
                CPURaytracer::Hits cn;
                cpu.QueryHits(c.reflected, c.index, cn);
                g = gn;
                c = cn;
                hits = 0;
                for (size_t i = 0; i < n; ++i) hits += g.index[i] >= 0;
                std::printf("%sbounce%d %d\n", tag, bounce, same_hits(g, c));
                std::printf("%sbounce%d_hits %zu\n", tag, bounce, hits);
                std::printf("%sbounce%d_traced %d\n", tag, bounce, gpu.QueryInfo().n_rays == traced);
            }
            std::vector<uint64_t> items;
            for (size_t i = 0; i < n; i += 7) items.push_back(i);
            items.push_back(n - 1);
            const HIPRaytracer::Hits p = gpu.PickHits(items);
            HIPRaytracer::Hits want;
            for (uint64_t k : items) {
                want.t.push_back(first.t[k]);
                want.index.push_back(first.index[k]);
                want.point.push_back(first.point[k]);
                want.normal.push_back(first.normal[k]);
                want.reflected.push_back(first.reflected[k]);
            }
            std::printf("%spick_hits %d\n", tag, same_hits(p, want));
            const unsigned pi = (unsigned)(width / 2), pj = (unsigned)(height / 2);
            const HIPRaytracer::Hits one = gpu.PickHit(pi, pj);
            const size_t k = (size_t)pj * width + pi;
            std::printf("%spick_hit %d\n", tag, one.t.size() == 1 && same_number(one.t[0], first.t[k]) && one.index[0] == first.index[k] &&
                                                    same_vec(one.point[0], first.point[k]) && same_vec(one.normal[0], first.normal[k]) &&
                                                    same_vec(one.reflected[0].start, first.reflected[k].start) &&
                                                    same_vec(one.reflected[0].direction, first.reflected[k].direction));
            std::printf("%spick_hit_index %d\n", tag, one.index[0]);
        }
        const std::vector<uint8_t> show(1, 1);
        if (objects.size() > 1) gpu.SetVisibility((uint32_t)(objects.size() / 2), show);
        const cl_float4* again = raytracer->Render();
        std::printf("frame_untouched %d\n", std::memcmp(again, before.data(), sizeof(cl_float4) * n) == 0);
        bool refused = false;
        try { gpu.PickHits(std::vector<uint64_t>(1, (uint64_t)n)); }
        catch (const std::exception&) { refused = true; }
        std::printf("pick_refused %d\n", refused);
        bool mask_refused = false;
        try { gpu.QueryHits(rays, std::vector<int32_t>(3, 0)); }
        catch (const std::exception&) { mask_refused = true; }
        std::printf("mask_refused %d\n", mask_refused);

        HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
        std::printf("two_shards_same %d\n", same_hits(two.QueryHits(rays), gpu.QueryHits(rays)));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
