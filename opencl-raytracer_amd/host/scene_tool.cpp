// scene_tool.cpp - the reference's main() without the window (OpenCL-Raytracer.cpp:28-104):
//   scene_tool records <scene.txt> <out.bin>          parse the scene, dump the device records (no GPU needed)
//   scene_tool render  <scene.txt> <W> <H> <D> <out.ppm> [z-bits|-] [hip|cpu]
//                       parse, build rays, render, write a PPM. Backend: `hip` (default) = HIPRaytracer on the GPU;
//                       `cpu` = CPURaytracer, no GPU (the reference's main() has both lines, OpenCL-Raytracer.cpp:74-75)
//   scene_tool render8 <scene.txt> <W> <H> <D> <out.ppm> [z-bits|-] [p3|p6] [rgba8|rgb8]
//                       the same frame as 8-bit pixels quantised on the GPU (HIPRaytracer::RenderPacked), written from the
//                       bytes: `p3` (default) the reference's ASCII file, `p6` the binary PPM
//   render and render8 take `--ss S` (S = 2, 3, 4) anywhere behind the command: S x S samples per pixel, box-filtered by the
//                       backend (SetSupersampling). The picture stays W x H; the sample grid is S W x S H at S z.
//   render and render8 take `--pose m00,m01,m02,m10,m11,m12,m20,m21,m22,ox,oy,oz` likewise: the camera seen through the 3 x 3
//                       matrix (row-major) from the origin (ox, oy, oz) - the backend's SetPose on the (sample) grid; also with --ss.
//   scene_tool pick    <scene.txt> <W> <H> <i> <j> [hip|cpu] [z-bits|-]
//                       the object under pixel (column i, row j) of the W x H picture: prints "pick <object index or -1> <t>
//                       <backend>" as its last line, behind "point <x> <y> <z> <w>" and "normal <x> <y> <z>" - where the ray
//                       meets the object, in view space, and the unit normal there (zeros on a miss). HIPRaytracer::PickHits on
//                       the GPU; with `cpu`, or where no GPU backend can be made, CPURaytracer::QueryHits of that pixel's ray -
//                       the same answer; z-bits as for render
//   scene_tool gbuffer <scene.txt> <W> <H> <out-prefix> [hip|cpu] [z-bits|-]
//                       the primary hits of the W x H picture as two binary PPMs (HIPRaytracer::RenderGBuffer; with `cpu`, or where
//                       no GPU backend can be made, CPURaytracer::RenderGBuffer - the same records): <out-prefix>_normal.ppm, the
//                       unit normal mapped as 0.5 n + 0.5, and <out-prefix>_depth.ppm, t divided by the largest finite t of the
//                       frame; a miss is black in both. Bytes by the rule of ppm.format_p6 (floor(255 v), clamped)
//   scene_tool ao      <scene.txt> <W> <H> <K> <out.ppm> [hip|cpu] [radius] [--filter R,NORMAL_MIN,PLANE_MAX]
//                       ambient occlusion of the W x H picture as a grey binary PPM (HIPRaytracer::RenderAO; with `cpu`, or where no
//                       GPU backend can be made, CPURaytracer::RenderAO - the same counts): K = 1, 2, 4 ... 64 rays per pixel of
//                       length `radius` (default 1) from 16 sets of cosine-weighted directions made here from a fixed seed; a pixel
//                       is floor(255 ao), a miss white. With --filter (anywhere behind <out.ppm>) the picture is the FILTERED grey:
//                       the edge-aware blur of the counts over a (2R + 1)^2 window (HIPRaytracer::RenderAOFiltered, or
//                       CPURaytracer::RenderAOFiltered - the same bytes); without it the output is unchanged
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "CPURaytracer.hpp"
#include "HIPRaytracer.hpp"
#include "PPMExporter.hpp"
#include "SceneLoader.hpp"
#include "rt_records.h"

static void dump_records(const std::vector<ObjectData>& objects, const std::vector<Light>& lights, const char* path) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error("cannot write records");
    const uint32_t n[2] = {(uint32_t)objects.size(), (uint32_t)lights.size()};
    std::fwrite(n, 4, 2, f);
    for (const ObjectData& o : objects) {
        rt_object_data d;
        std::memset(&d, 0, sizeof(d));
        const float amb[4] = {o.mat.ambient.x, o.mat.ambient.y, o.mat.ambient.z, 0}, dif[4] = {o.mat.diffuse.x, o.mat.diffuse.y, o.mat.diffuse.z, 0},
                    spe[4] = {o.mat.specular.x, o.mat.specular.y, o.mat.specular.z, 0};
        std::memcpy(d.mat.ambient, amb, 16); std::memcpy(d.mat.diffuse, dif, 16); std::memcpy(d.mat.specular, spe, 16);
        d.mat.absorption = o.mat.absorption; d.mat.reflection = o.mat.reflection; d.mat.transparency = o.mat.transparency; d.mat.shininess = o.mat.shininess;
        std::memcpy(d.mv, o.mv.data(), 64); std::memcpy(d.mvInverse, o.mvInverse.data(), 64); std::memcpy(d.mvInverseTranspose, o.mvInverseTranspose.data(), 64);
        d.type = (uint32_t)o.type;
        std::fwrite(&d, sizeof(d), 1, f);
    }
    for (const Light& l : lights) {
        const float rec[16] = {l.ambient.x, l.ambient.y, l.ambient.z, 0, l.diffuse.x, l.diffuse.y, l.diffuse.z, 0,
                               l.specular.x, l.specular.y, l.specular.z, 0, l.lightPosition.x, l.lightPosition.y, l.lightPosition.z, l.lightPosition.w};
        std::fwrite(rec, 64, 1, f);
    }
    std::fclose(f);
}

int main(int argc, char** argv) {
    try {
        unsigned ss = 1;  // --ss S: taken out of the argument list, whatever its position
        for (int k = 2; k + 1 < argc; ++k)
            if (std::strcmp(argv[k], "--ss") == 0) {
                ss = (unsigned)std::atoi(argv[k + 1]);
                for (int q = k; q + 2 < argc; ++q) argv[q] = argv[q + 2];
                argc -= 2;
                break;
            }
        if (ss < 1 || ss > 4) { std::fprintf(stderr, "--ss takes 1, 2, 3 or 4\n"); return 1; }
        bool posed = false;  // --pose twelve numbers: taken out likewise
        float pose[12];
        for (int k = 2; k + 1 < argc; ++k)
            if (std::strcmp(argv[k], "--pose") == 0) {
                const char* q = argv[k + 1];
                int got = 0;
                while (got < 12) {
                    char* end = nullptr;
                    pose[got] = std::strtof(q, &end);
                    if (end == q) break;
                    ++got;
                    q = end;
                    if (*q != ',') break;
                    ++q;
                }
                if (got != 12 || *q) { std::fprintf(stderr, "--pose takes m00,m01,m02,m10,m11,m12,m20,m21,m22,ox,oy,oz\n"); return 1; }
                posed = true;
                for (int r = k; r + 2 < argc; ++r) argv[r] = argv[r + 2];
                argc -= 2;
                break;
            }
        if (argc < 4) { std::fprintf(stderr, "usage: scene_tool records|render|render8 ...\n"); return 1; }
        std::vector<ObjectData> objects;
        std::vector<Light> lights;
        SceneLoader loader;
        loader.Load(argv[2], objects, lights);
        std::printf("Scene file loaded without any errors.\n");
        if (std::strcmp(argv[1], "records") == 0) { dump_records(objects, lights, argv[3]); return 0; }
        if (std::strcmp(argv[1], "pick") == 0) {
            if (argc < 7) { std::fprintf(stderr, "usage: scene_tool pick <scene.txt> <W> <H> <i> <j>\n"); return 1; }
            const int pw = std::atoi(argv[3]), ph = std::atoi(argv[4]), pi = std::atoi(argv[5]), pj = std::atoi(argv[6]);
            if (pw <= 0 || ph <= 0 || pi < 0 || pj < 0 || pi >= pw || pj >= ph) { std::fprintf(stderr, "pick: 0 <= i < W, 0 <= j < H\n"); return 1; }
            float pfov = rtm::radians(60.f);
            pfov *= 0.5f;
            float pz = -((ph / 2.0f) / tanf(pfov));
            if (argc > 8 && std::strcmp(argv[8], "-") != 0) { const uint32_t bits = (uint32_t)std::strtoul(argv[8], nullptr, 16); std::memcpy(&pz, &bits, 4); }
            std::vector<Ray3D> grid;
            grid.reserve((size_t)pw * ph);
            for (int jj = 0; jj < ph; ++jj)
                for (int ii = 0; ii < pw; ++ii)
                    grid.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - pw / 2.0f, (float)(ph - jj) - ph / 2.0f, pz));
            const uint64_t item = (uint64_t)pj * (uint64_t)pw + (uint64_t)pi;
            std::vector<float> t;
            std::vector<int32_t> index;
            rtm::vec4 point, normal, colour;
            const char* backend_name = (argc > 7 && std::strcmp(argv[7], "cpu") == 0) ? "cpu" : "hip";
            if (std::strcmp(backend_name, "hip") == 0) {
                try {
                    HIPRaytracer backend(objects, lights, grid, 0);
                    const HIPRaytracer::Hits hit = backend.PickHits(std::vector<uint64_t>(1, item));
                    t = hit.t; index = hit.index; point = hit.point[0]; normal = hit.normal[0];
                    colour = backend.PickColours(std::vector<uint64_t>(1, item)).rgba[0];
                } catch (const std::exception& e) {  // (no GPU: the CPU backend's loop over the same ray - said on stderr and in the line)
                    std::fprintf(stderr, "pick: %s; using the CPU backend\n", e.what());
                    backend_name = "cpu";
                }
            }
            if (std::strcmp(backend_name, "cpu") == 0) {
                CPURaytracer backend(objects, lights, grid, 0);
                CPURaytracer::Hits hit;
                backend.QueryHits(std::vector<Ray3D>(1, grid[item]), std::vector<int32_t>(), hit);
                t = hit.t; index = hit.index; point = hit.point[0]; normal = hit.normal[0];
                CPURaytracer::Shade shade;
                backend.QueryShade(std::vector<Ray3D>(1, grid[item]), std::vector<int32_t>(), shade);
                colour = shade.rgba[0];
            }
            std::printf("colour %.9g %.9g %.9g %.9g\n", (double)colour.x, (double)colour.y, (double)colour.z, (double)colour.w);
            std::printf("point %.9g %.9g %.9g %.9g\n", (double)point.x, (double)point.y, (double)point.z, (double)point.w);
            std::printf("normal %.9g %.9g %.9g\n", (double)normal.x, (double)normal.y, (double)normal.z);
            std::printf("pick %d %.9g %s\n", (int)index[0], (double)t[0], backend_name);
            return 0;
        }
        if (std::strcmp(argv[1], "gbuffer") == 0) {
            if (argc < 6) { std::fprintf(stderr, "usage: scene_tool gbuffer <scene.txt> <W> <H> <out-prefix> [hip|cpu] [z-bits|-]\n"); return 1; }
            const int gw = std::atoi(argv[3]), gh = std::atoi(argv[4]);
            if (gw <= 0 || gh <= 0) { std::fprintf(stderr, "gbuffer: W > 0, H > 0\n"); return 1; }
            float gfov = rtm::radians(60.f);
            gfov *= 0.5f;
            float gz = -((gh / 2.0f) / tanf(gfov));
            if (argc > 7 && std::strcmp(argv[7], "-") != 0) { const uint32_t bits = (uint32_t)std::strtoul(argv[7], nullptr, 16); std::memcpy(&gz, &bits, 4); }
            std::vector<Ray3D> grid;
            grid.reserve((size_t)gw * gh);
            for (int jj = 0; jj < gh; ++jj)
                for (int ii = 0; ii < gw; ++ii)
                    grid.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - gw / 2.0f, (float)(gh - jj) - gh / 2.0f, gz));
            const size_t n = grid.size();
            std::vector<float> t;
            std::vector<int32_t> index;
            std::vector<rtm::vec4> normal;
            const char* backend_name = (argc > 6 && std::strcmp(argv[6], "cpu") == 0) ? "cpu" : "hip";
            if (std::strcmp(backend_name, "hip") == 0) {
                try {
                    HIPRaytracer backend(objects, lights, grid, 0);
                    HIPRaytracer::GBuffer g = backend.RenderGBuffer();
                    t.swap(g.t); index.swap(g.index); normal.swap(g.normal);
                } catch (const std::exception& e) {  // (no GPU: the CPU backend's records - said on stderr and in the last line)
                    std::fprintf(stderr, "gbuffer: %s; using the CPU backend\n", e.what());
                    backend_name = "cpu";
                }
            }
            if (std::strcmp(backend_name, "cpu") == 0) {
                CPURaytracer backend(objects, lights, grid, 0);
                CPURaytracer::GBuffer g;
                backend.RenderGBuffer(g);
                t.swap(g.t); index.swap(g.index); normal.swap(g.normal);
            }
            float t_max = 0.f;
            size_t hits = 0;
            for (size_t i = 0; i < n; ++i)
                if (index[i] >= 0) { ++hits; if (std::isfinite(t[i]) && t[i] > t_max) t_max = t[i]; }
            // floor(255 v) clamped to 0 .. 255, NaN -> 0: ppm.quantise_bytes
            auto level = [](float v) { const float f = std::floor(v * 255.0f); return (uint8_t)(f >= 0.0f ? (f >= 255.0f ? 255.0f : f) : 0.0f); };
            std::vector<uint8_t> nb(3 * n, 0), db(3 * n, 0);
            for (size_t i = 0; i < n; ++i) {
                if (index[i] < 0) continue;
                nb[3 * i] = level(0.5f * normal[i].x + 0.5f);
                nb[3 * i + 1] = level(0.5f * normal[i].y + 0.5f);
                nb[3 * i + 2] = level(0.5f * normal[i].z + 0.5f);
                db[3 * i] = db[3 * i + 1] = db[3 * i + 2] = t_max > 0.f ? level(t[i] / t_max) : (uint8_t)0;
            }
            const std::string prefix(argv[5]);
            PPMExporter::ExportP6(prefix + "_normal.ppm", (size_t)gw, (size_t)gh, nb.data(), 3);
            PPMExporter::ExportP6(prefix + "_depth.ppm", (size_t)gw, (size_t)gh, db.data(), 3);
            std::printf("gbuffer %zu hits of %zu, largest t %.9g, %s\n", hits, n, (double)t_max, backend_name);
            return 0;
        }
        if (std::strcmp(argv[1], "ao") == 0) {
            // --filter R,NORMAL_MIN,PLANE_MAX is taken out of the arguments; the positional ones read as ever
            bool filtered = false;
            unsigned filter_radius = 0;
            float filter_normal_min = 0.f, filter_plane_max = 0.f;
            for (int a = 7; a < argc; ++a) {
                if (std::strcmp(argv[a], "--filter") != 0) continue;
                if (a + 1 >= argc || std::sscanf(argv[a + 1], "%u,%f,%f", &filter_radius, &filter_normal_min, &filter_plane_max) != 3 ||
                    filter_radius < 1 || filter_radius > 4 || !(filter_plane_max >= 0.f) || !std::isfinite(filter_plane_max)) {
                    std::fprintf(stderr, "ao: --filter R,NORMAL_MIN,PLANE_MAX with R 1 .. 4 and PLANE_MAX finite, >= 0\n");
                    return 1;
                }
                filtered = true;
                for (int b = a + 2; b < argc; ++b) argv[b - 2] = argv[b];
                argc -= 2;
                break;
            }
            if (argc < 7) { std::fprintf(stderr, "usage: scene_tool ao <scene.txt> <W> <H> <K> <out.ppm> [hip|cpu] [radius] [--filter R,NORMAL_MIN,PLANE_MAX]\n"); return 1; }
            const int aw = std::atoi(argv[3]), ah = std::atoi(argv[4]);
            const unsigned K = (unsigned)std::atoi(argv[5]);
            const float radius = argc > 8 ? (float)std::atof(argv[8]) : 1.0f;
            if (aw <= 0 || ah <= 0 || K == 0 || K > 64 || (K & (K - 1)) || !(radius > 0.f)) {
                std::fprintf(stderr, "ao: W > 0, H > 0, K one of 1, 2, 4, 8, 16, 32, 64, radius > 0\n");
                return 1;
            }
            float afov = rtm::radians(60.f);
            afov *= 0.5f;
            const float az = -((ah / 2.0f) / tanf(afov));
            std::vector<Ray3D> grid;
            grid.reserve((size_t)aw * ah);
            for (int jj = 0; jj < ah; ++jj)
                for (int ii = 0; ii < aw; ++ii)
                    grid.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - aw / 2.0f, (float)(ah - jj) - ah / 2.0f, az));
            // 16 sets of K cosine-weighted directions about +z (the pass mirrors each to the normal's side), from a fixed seed
            std::vector<rtm::vec4> dirs;
            uint32_t state = 0x2545F491u;
            auto uniform = [&state]() { state ^= state << 13; state ^= state >> 17; state ^= state << 5; return (float)(state >> 8) * (1.0f / 16777216.0f); };
            for (unsigned j = 0; j < 16 * K; ++j) {
                const float u = uniform(), phi = 6.2831853f * uniform(), r = std::sqrt(u);
                dirs.emplace_back(radius * r * std::cos(phi), radius * r * std::sin(phi), radius * std::sqrt(1.0f - u), 0.f);
            }
            const size_t n = grid.size();
            std::vector<uint8_t> unoccluded;
            std::vector<float> ao;
            std::vector<uint8_t> filtered_grey;   // --filter: the picture's bytes
            const char* backend_name = (argc > 7 && std::strcmp(argv[7], "cpu") == 0) ? "cpu" : "hip";
            if (std::strcmp(backend_name, "hip") == 0) {
                try {
                    HIPRaytracer backend(objects, lights, grid, 0);
                    HIPRaytracer::AO a = backend.RenderAO(dirs, K);
                    unoccluded.swap(a.unoccluded); ao.swap(a.ao);
                    if (filtered) filtered_grey = backend.RenderAOFiltered(dirs, K, 1e-3f, filter_radius, filter_normal_min, filter_plane_max).grey;
                } catch (const std::exception& e) {  // (no GPU: the CPU backend's counts - said on stderr and in the last line)
                    std::fprintf(stderr, "ao: %s; using the CPU backend\n", e.what());
                    backend_name = "cpu";
                }
            }
            if (std::strcmp(backend_name, "cpu") == 0) {
                CPURaytracer backend(objects, lights, grid, 0);
                CPURaytracer::AO a;
                backend.RenderAO(dirs, K, 1e-3f, a);
                unoccluded.swap(a.unoccluded); ao.swap(a.ao);
                if (filtered) {
                    CPURaytracer::FilteredAO f;
                    backend.RenderAOFiltered(dirs, K, 1e-3f, (size_t)aw, filter_radius, filter_normal_min, filter_plane_max, f);
                    filtered_grey.swap(f.grey);
                }
            }
            std::vector<uint8_t> grey(3 * n, 0);
            size_t sum = 0;
            for (size_t i = 0; i < n; ++i) {
                const float f = std::floor(ao[i] * 255.0f);
                grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = (uint8_t)(f >= 0.0f ? (f >= 255.0f ? 255.0f : f) : 0.0f);
                if (filtered) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = filtered_grey[i];
                sum += unoccluded[i];
            }
            PPMExporter::ExportP6(argv[6], (size_t)aw, (size_t)ah, grey.data(), 3);
            std::printf("ao %zu of %zu rays unoccluded, %s\n", sum, n * K, backend_name);
            return 0;
        }
        if (argc < 7) return 1;
        const int width = std::atoi(argv[3]), height = std::atoi(argv[4]);
        const unsigned depth = (unsigned)std::atoi(argv[5]);
        float fov = rtm::radians(60.f);
        fov *= 0.5f;
        float z = -((height / 2.0f) / tanf(fov));
        if (argc > 7 && std::strcmp(argv[7], "-") != 0) { const uint32_t bits = (uint32_t)std::strtoul(argv[7], nullptr, 16); std::memcpy(&z, &bits, 4); }
        const bool cpu = argc > 8 && std::strcmp(argv[8], "cpu") == 0;
        // the sample grid: (ss W, ss H, fl(ss z)) - the picture's own grid for ss = 1
        const int sw = (int)ss * width, sh = (int)ss * height;
        const float sz = (float)ss * z;
        std::vector<Ray3D> rays;
        rays.reserve((size_t)sw * sh);
        for (int jj = 0; jj < sh; ++jj)
            for (int ii = 0; ii < sw; ++ii)
                rays.emplace_back(rtm::vec3(0, 0, 0), rtm::vec3((float)ii - sw / 2.0f, (float)(sh - jj) - sh / 2.0f, sz));
        if (std::strcmp(argv[1], "render8") == 0) {
            const bool p6 = argc > 8 && std::strcmp(argv[8], "p6") == 0;
            const rt_pixel_format format = (argc > 9 && std::strcmp(argv[9], "rgb8") == 0) ? RT_PIXEL_RGB8 : RT_PIXEL_RGBA8;
            HIPRaytracer raytracer8(objects, lights, rays, depth);
            if (ss > 1) raytracer8.SetSupersampling(ss);
            if (posed) raytracer8.SetPose((unsigned)sw, (unsigned)sh, sz, pose, pose + 9);
            const uint8_t* bytes = raytracer8.RenderPacked(format);
            const size_t stride = rt_packed_pixel_bytes(format);
            if (p6) PPMExporter::ExportP6(argv[6], (size_t)width, (size_t)height, bytes, stride);
            else PPMExporter::ExportP3(argv[6], (size_t)width, (size_t)height, bytes, stride);
            std::printf("wrote %s\n", argv[6]);
            return 0;
        }
        std::unique_ptr<IRaytracer> raytracer;
        if (cpu) {
            CPURaytracer* backend = new CPURaytracer(objects, lights, rays, depth);
            raytracer.reset(backend);
            if (ss > 1) backend->SetSupersampling(ss, (size_t)sw);
            if (posed) backend->SetPose((size_t)sw, (size_t)sh, sz, pose, pose + 9);
        } else {
            HIPRaytracer* backend = new HIPRaytracer(objects, lights, rays, depth);
            raytracer.reset(backend);
            if (ss > 1) backend->SetSupersampling(ss);
            if (posed) backend->SetPose((unsigned)sw, (unsigned)sh, sz, pose, pose + 9);
        }
        cl_float4* pixels = raytracer->Render();
        PPMExporter::ExportP3(argv[6], (size_t)width, (size_t)height, PPMExporter::RGBAtoRGB(reinterpret_cast<const float*>(pixels), (size_t)width * height));
        std::printf("wrote %s\n", argv[6]);
        return 0;
    } catch (const std::out_of_range& e) {
        std::printf("out_of_range %s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 2;
    }
}
