// host_gbuffer_test.cpp - G-buffer frames through the C++ flavour of the boundary (HIPRaytracer::RenderGBuffer / GBufferInfo):
//   host_gbuffer_test <scene.txt> <W> <H> <D>
// parses the scene, constructs the GPU backend and the CPU backend with the W x H pinhole grid and compares the two G-buffers number
// for number (the default arithmetic is the CPU backend's; a NaN on both sides counts as equal), then the GPU's records with
// HIPRaytracer::PickHits over all work-items; once more with the middle object hidden and recoloured on both; that the frame is
// untouched; and each shard of the two-shard object against its tiles of the whole
// (H a multiple of 16). Prints one line per check for
// tests/test_host_gbuffer_gpu.py.
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
template <class A, class B>
static bool same_gbuffer(const A& g, const B& c) {
    const size_t n = g.t.size();
    if (c.t.size() != n || g.index != c.index || g.point.size() != n || c.point.size() != n || g.normal.size() != n || c.normal.size() != n ||
        g.albedo.size() != n || c.albedo.size() != n)
        return false;
    for (size_t i = 0; i < n; ++i)
        if (!same_number(g.t[i], c.t[i]) || !same_vec(g.point[i], c.point[i]) || !same_vec(g.normal[i], c.normal[i]) || !same_vec(g.albedo[i], c.albedo[i]))
            return false;
    return true;
}
static bool zero_vec(const rtm::vec4& v) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    return std::memcmp(&v, zero, 16) == 0;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: host_gbuffer_test <scene.txt> <W> <H> <D>\n"); return 1; }
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
        std::vector<uint64_t> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = i;

        HIPRaytracer::GBuffer whole;
        for (int round = 0; round < 2; ++round) {
            const char* tag = round ? "changed_" : "";
            if (round && objects.size() > 1) {
                const uint32_t mid = (uint32_t)(objects.size() / 2);
                const std::vector<uint8_t> hide(1, 0);
                gpu.SetVisibility(mid, hide);
                cpu.SetVisibility(mid, hide);
                std::vector<Material> paint(1, objects[0].mat);
                paint[0].diffuse = rtm::vec3(0.125f, 0.75f, 0.375f);
                gpu.SetMaterials(0, paint);
                cpu.SetMaterials(0, paint);
            }
            const HIPRaytracer::GBuffer g = gpu.RenderGBuffer();
            CPURaytracer::GBuffer c;
            cpu.RenderGBuffer(c);
            size_t hits = 0, painted = 0;
            bool zero_ok = true;
            for (size_t i = 0; i < n; ++i) {
                hits += g.index[i] >= 0;
                painted += g.index[i] == 0 && g.albedo[i].x == 0.125f && g.albedo[i].y == 0.75f && g.albedo[i].z == 0.375f && g.albedo[i].w == 1.0f;
                if (g.index[i] < 0) zero_ok = zero_ok && zero_vec(g.point[i]) && zero_vec(g.normal[i]) && zero_vec(g.albedo[i]);
            }
            std::printf("%ssame_as_cpu %d\n", tag, same_gbuffer(g, c));
            std::printf("%shits %zu\n", tag, hits);
            std::printf("%spainted %zu\n", tag, painted);
            std::printf("%smisses_zero %d\n", tag, zero_ok);
            const rt_gbuffer_info_t info = gpu.GBufferInfo();
            std::printf("%sinfo %d\n", tag, info.n_items == n && info.hits == hits && info.trace_ms > 0.0 && info.records_ms > 0.0);
            const HIPRaytracer::Hits p = gpu.PickHits(items);
            bool pick_ok = p.t.size() == n && p.index == g.index;
            for (size_t i = 0; pick_ok && i < n; ++i)
                pick_ok = same_number(p.t[i], g.t[i]) && same_vec(p.point[i], g.point[i]) && same_vec(p.normal[i], g.normal[i]);
            std::printf("%ssame_as_pick_hits %d\n", tag, pick_ok);
            if (round) whole = g;
        }
        // each shard of the several-GPU object delivers its own tiles of the whole (16-row tiles dealt round-robin)
        {
            HIPRaytracer two(objects, lights, rays, depth, std::vector<int>{0, 0});
            if (objects.size() > 1) {
                const uint32_t mid = (uint32_t)(objects.size() / 2);
                two.SetVisibility(mid, std::vector<uint8_t>(1, 0));
                std::vector<Material> paint(1, objects[0].mat);
                paint[0].diffuse = rtm::vec3(0.125f, 0.75f, 0.375f);
                two.SetMaterials(0, paint);
            }
            size_t total = 0;
            bool ok = true;
            const size_t tile = (size_t)16 * width;   // rt_create_multi's row tiles of a pinhole grid
            for (unsigned shard = 0; shard < 2; ++shard) {
                const HIPRaytracer::GBuffer part = two.RenderGBuffer(shard);
                total += part.t.size();
                for (size_t i = 0; i < part.t.size() && ok; ++i) {
                    const size_t g = ((i / tile) * 2 + shard) * tile + i % tile;
                    if (g >= n) { ok = part.index[i] == -1 && zero_vec(part.point[i]); continue; }   // padding of a ragged last tile
                    ok = same_number(part.t[i], whole.t[g]) && part.index[i] == whole.index[g] && same_vec(part.point[i], whole.point[g]) &&
                         same_vec(part.normal[i], whole.normal[g]) && same_vec(part.albedo[i], whole.albedo[g]);
                }
                ok = ok && !part.t.empty() && two.GBufferInfo(shard).n_items == part.t.size();
            }
            std::printf("two_shards_same %d\n", ok && total >= n);
        }
        const std::vector<uint8_t> show(1, 1);
        if (objects.size() > 1) {
            gpu.SetVisibility((uint32_t)(objects.size() / 2), show);
            gpu.SetMaterials(0, std::vector<Material>(1, objects[0].mat));
        }
        const cl_float4* again = raytracer->Render();
        std::printf("frame_untouched %d\n", std::memcmp(again, before.data(), sizeof(cl_float4) * n) == 0);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    return 0;
}
