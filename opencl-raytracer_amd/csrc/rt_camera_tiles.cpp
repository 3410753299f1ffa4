// rt_camera_tiles.cpp - screen rectangles and the primary rays' screen tiles: a camera's table built on the host, a pose's on the
// device (rt_tiles.hip).
#include "rt_context.h"

namespace rt::host {

// Conservative projection of a bounding sphere onto the pinhole image plane, in ray-direction units
// (direction = (x, y, z), z < 0 fixed): [xmin, xmax] from the two tangent planes that contain the camera's y
// axis, [ymin, ymax] likewise. Unbounded when the sphere reaches the plane z = 0 through the camera; empty when
// it lies entirely behind it. Padded by one pixel plus 1e-6 relative before rounding outwards to float.
float4 screen_rect(const Sphere& s, double z) {
    const float inf = std::numeric_limits<float>::infinity();
    const float4 all = make_float4(-inf, inf, -inf, inf), none = make_float4(inf, -inf, inf, -inf);
    if (s.r == -std::numeric_limits<double>::infinity()) return none;
    if (!std::isfinite(s.r) || !(z < 0)) return all;
    if (s.z - s.r >= 0) return none;          // entirely behind the camera: every root is negative
    if (s.z + s.r >= 0) return all;           // reaches the camera plane: silhouette unbounded
    auto extent = [&](double cu, float& lo, float& hi) {
        // tangent planes through the origin containing the other image axis: (z cu - u cz)^2 = R^2 (u^2 + z^2)
        const double a = s.z * s.z - s.r * s.r, b = -2.0 * z * cu * s.z, c = z * z * (cu * cu - s.r * s.r);
        const double disc = b * b - 4.0 * a * c;
        if (!(a > 0) || !(disc >= 0)) { lo = -inf; hi = inf; return; }
        const double sq = std::sqrt(disc);
        double u0 = (-b - sq) / (2.0 * a), u1 = (-b + sq) / (2.0 * a);
        if (u0 > u1) std::swap(u0, u1);
        u0 -= 1.0 + 1e-6 * std::fabs(u0);
        u1 += 1.0 + 1e-6 * std::fabs(u1);
        lo = std::nextafter((float)u0, -inf);
        hi = std::nextafter((float)u1, inf);
    };
    float4 r;
    extent(s.x, r.x, r.y);
    extent(s.y, r.z, r.w);
    return r;
}

// Is the uploaded ray list bit-for-bit the reference's pinhole grid (OpenCL-Raytracer.cpp:18-26,68-72)?
bool detect_pinhole(const rt_ray* rays, uint64_t n, uint32_t& W, uint32_t& H, float& z) {
    if (n == 0 || n > 0xffffffffull) return false;
    const float y0 = rays[0].direction[1];
    uint64_t w = n;
    for (uint64_t i = 1; i < n; ++i) {
        if (rays[i].direction[1] != y0) { w = i; break; }
    }
    if (w == 0 || n % w != 0) return false;
    const uint64_t h = n / w;
    if (w > 0x1000000ull || h > 0x1000000ull) return false;  // exact integer -> float conversion range
    const float zz = rays[0].direction[2];
    const float half_w = (float)w / 2.0f, half_h = (float)h / 2.0f, hf = (float)h;
    for (uint64_t j = 0; j < h; ++j) {
        const float dy = (hf - (float)j) - half_h;
        const rt_ray* row = rays + j * w;
        for (uint64_t i = 0; i < w; ++i) {
            const rt_ray& r = row[i];
            const float expect[8] = {0.f, 0.f, 0.f, 1.f, (float)i - half_w, dy, zz, 0.f};
            if (std::memcmp(&r, expect, sizeof(expect)) != 0) return false;
        }
    }
    W = (uint32_t)w;
    H = (uint32_t)h;
    z = zz;
    return true;
}

// Primary rays of a pinhole grid: per screen tile the objects whose conservative screen rectangle (projection of the grid
// sphere, i.e. with the same error-bound inflation) overlaps the tile, each with its depth key (rt_grid.h: ScreenTiles - a
// lower bound on the t the object can report on a primary ray of this camera), nearest key first. A wave of the first trace round
// holds the 64 pixels of ONE tile - an 8 x 8 block (col_shift 3) when the work-items walk the frame in such blocks, else 64
// consecutive pixels of a row inside a 64 x 8 tile (col_shift 6) - so it walks that list with wave-uniform scalar loads
// instead of 64 separate grid walks. (Round 2: 8 x 8 tiles instead of 64 x 8 wherever the order allows - a wave no longer
// tests what only the seven other blocks of its 64 x 8 tile can see. Depth order: with the list by nearest possible t a wave
// stops at the first entry that lies behind what all of its lanes have already hit - about 2 exact tests per 8 x 8 tile of
// the cfg4 frame instead of its whole list of ~10.)
static int build_pose_tiles(rt_context* c, hipStream_t stream);

static int build_screen_tiles(rt_context* c, hipStream_t stream, uint32_t col_shift) {
    c->tiles = rt::ScreenTiles{};
    c->tiles_dirty = false;
    c->primary_outside = false;  // (only an accepted table of a pose outside the box sets it again: build_pose_tiles)
    if (!c->pinhole && c->have_rays && c->pose_w) return build_pose_tiles(c, stream);  // the rays in use come from a pose
    const uint32_t tile_w = 1u << col_shift;
    if (!c->grid.enabled || !c->pinhole || !(c->z < 0.f) || c->width % tile_w != 0 || c->h_grid_spheres.empty()) return RT_OK;
    const uint32_t tx = c->width / tile_w, ty = (c->height + 7u) / 8u;
    const size_t n_tiles = (size_t)tx * ty;
    const uint32_t n = c->n_objs;
    const double half_w = (double)((float)c->width / 2.0f), half_h = (double)((float)c->height / 2.0f), H = (double)c->height;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<uint32_t> start(n_tiles + 1, 0), entries, fill, global;
    std::vector<float> key(n, -std::numeric_limits<float>::infinity());
    struct Range { int x0, x1, y0, y1; };
    std::vector<Range> rng(n);
    // (object, tile) pairs are counted in 64 bits against the budget BEFORE any per-tile loop runs: an object whose
    // sphere reaches the camera plane projects onto the whole screen (131 072 tiles at 8192^2), and a few ten
    // thousand of those would wrap a 32-bit prefix sum. Such objects go to a per-camera global list that every tile
    // wave tests (at most kMaxGlobal of them; beyond that the grid walk is the better tool for primary rays too).
    constexpr size_t kMaxGlobal = 64;
    const uint64_t budget = 256ull * n + 4096ull;
    uint64_t total = 0;
    // every object's tile rectangle (the expensive part: screen_rect), on several threads; what depends on the order - the budget,
    // the global list, the counts - in a second, serial sweep
    parallel_for(n, 8192, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const double r = c->h_grid_spheres[4 * i + 3];
            Range& q = rng[i];
            q.x0 = 0; q.x1 = -1; q.y0 = 0; q.y1 = -1;
            if (!(r >= 0) || r == inf) continue;  // never hit / always-list (handled by the kernel)
            const float4 rect = screen_rect(Sphere{c->h_grid_spheres[4 * i], c->h_grid_spheres[4 * i + 1], c->h_grid_spheres[4 * i + 2], r}, (double)c->z);
            if (!(rect.x <= rect.y) || !(rect.z <= rect.w)) continue;  // empty: behind the camera
            // direction x = col - W/2  ->  col range; direction y = (H - row) - H/2  ->  row range
            const double c0 = (double)rect.x + half_w, c1 = (double)rect.y + half_w;
            const double r0 = H - half_h - (double)rect.w, r1 = H - half_h - (double)rect.z;
            const double cx0 = std::max(0.0, std::floor(c0)), cx1 = std::min((double)c->width - 1, std::ceil(c1));
            const double ry0 = std::max(0.0, std::floor(r0)), ry1 = std::min((double)c->height - 1, std::ceil(r1));
            if (cx0 > cx1 || ry0 > ry1) continue;
            q.x0 = (int)(cx0 / tile_w); q.x1 = (int)(cx1 / tile_w); q.y0 = (int)(ry0 / 8); q.y1 = (int)(ry1 / 8);
            // depth key, rounded down (bound and margin: rt_grid.h, ScreenTiles)
            const double kd = (c->h_grid_spheres[4 * i + 2] + r) / (double)c->z;
            if (kd == kd) key[i] = std::nextafter((float)(kd - std::fabs(kd) * 0x1p-40), -std::numeric_limits<float>::infinity());
        }
    });
    for (uint32_t i = 0; i < n; ++i) {
        Range& q = rng[i];
        if (q.x1 < q.x0 || q.y1 < q.y0) continue;
        const uint64_t covered = (uint64_t)(q.x1 - q.x0 + 1) * (uint64_t)(q.y1 - q.y0 + 1);
        if (covered == (uint64_t)n_tiles && n_tiles > 1) {  // the whole screen
            if (global.size() >= kMaxGlobal) return RT_OK;
            global.push_back(i);
            q.x0 = 0; q.x1 = -1; q.y0 = 0; q.y1 = -1;
            continue;
        }
        total += covered;
        if (total > budget) return RT_OK;  // objects cover most of the screen: the grid walk is the better tool
        for (int y = q.y0; y <= q.y1; ++y)
            for (int x = q.x0; x <= q.x1; ++x) start[(size_t)y * tx + x + 1] += 1;
    }
    for (size_t k = 0; k < n_tiles; ++k) start[k + 1] += start[k];  // total <= budget < 2^32 (n_objs is a uint32, budget clamps below)
    if (total > 0xfffffff0ull) return RT_OK;
    entries.assign((size_t)total + global.size(), 0);
    fill.assign(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < n; ++i) {
        const Range& q = rng[i];
        for (int y = q.y0; y <= q.y1; ++y)
            for (int x = q.x0; x <= q.x1; ++x) entries[fill[(size_t)y * tx + x]++] = i;
    }
    for (size_t k = 0; k < n_tiles; ++k)
        if (fill[k] != start[k + 1]) return fail(c, RT_ERR_STATE, "internal: screen-tile fill does not match its count");
    for (size_t k = 0; k < global.size(); ++k) entries[(size_t)total + k] = global[k];  // the global list sits behind the last tile's
    // a tile's entries by ascending key, equal keys by ascending index (a deterministic table; the update is order-free), then
    // index and key side by side: one scalar load brings both. One zeroed entry of padding behind the last.
    std::vector<uint2> keyed(entries.size() + 1, make_uint2(0u, 0u));
    parallel_for(n_tiles, 1024, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
            std::sort(entries.begin() + start[t], entries.begin() + start[t + 1],
                      [&](uint32_t a, uint32_t b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
            for (size_t e = start[t]; e < start[t + 1]; ++e) {
                keyed[e].x = entries[e];
                std::memcpy(&keyed[e].y, &key[entries[e]], 4);
            }
        }
    });
    for (size_t k = 0; k < global.size(); ++k) keyed[(size_t)total + k].x = global[k];  // (tested by every wave: no key)
    if (c->d_tile_start) (void)hipFree(c->d_tile_start);
    if (c->d_tile_entries) (void)hipFree(c->d_tile_entries);
    c->d_tile_start = nullptr;
    c->d_tile_entries = nullptr;
    RT_HIP(c, hipMalloc((void**)&c->d_tile_start, sizeof(uint32_t) * (n_tiles + 1)));
    RT_HIP(c, hipMalloc((void**)&c->d_tile_entries, sizeof(uint2) * keyed.size()));
    RT_HIP(c, hipMemcpyAsync(c->d_tile_start, start.data(), sizeof(uint32_t) * (n_tiles + 1), hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipMemcpyAsync(c->d_tile_entries, keyed.data(), sizeof(uint2) * keyed.size(), hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    c->tiles.tile_start = c->d_tile_start;
    c->tiles.entries = c->d_tile_entries;
    c->tiles.tiles_x = tx;
    c->tiles.col_shift = col_shift;
    c->tiles.global_begin = (uint32_t)total;
    c->tiles.n_global = (uint32_t)global.size();
    c->tiles.enabled = 1u;
    return RT_OK;
}

// The build a frame (do_launch) or rt_get_tiles_info asks for when the rays changed, and what rt_get_tiles_info reports of it.
int refresh_screen_tiles(rt_context* c, hipStream_t stream, uint32_t col_shift) {
    c->tiles_info = rt_tiles_info_t{};
    int rc = build_screen_tiles(c, stream, col_shift);
    if (rc) return rc;
    // objects that cover much of the screen can exceed the pair budget at 8 x 8: the 64 x 8 tiles of round 1 serve an
    // 8 x 8 wave as well (its block lies inside one of them)
    if (!c->tiles.enabled && col_shift == 3u && c->pinhole) {
        rc = build_screen_tiles(c, stream, 6u);
        if (rc) return rc;
    }
    c->tiles_built_for = col_shift;
    RT_HIP(c, hipStreamSynchronize(stream));
    if (c->pinhole) {  // the camera's table (a pose's build fills the record itself; any other buffer has none)
        rt_tiles_info_t& ti = c->tiles_info;
        ti.enabled = c->tiles.enabled;
        ti.source = c->tiles.enabled ? 1u : 0u;
        ti.col_shift = c->tiles.enabled ? c->tiles.col_shift : col_shift;
        ti.tiles_x = c->width >> ti.col_shift;
        ti.tiles_y = (c->height + 7u) / 8u;
        ti.n_global = c->tiles.n_global;
        ti.n_entries = c->tiles.global_begin;
        if (!c->tiles.enabled)
            ti.refused = (!c->grid.enabled || c->h_grid_spheres.empty()) ? RT_TILES_REFUSED_NO_GRID
                         : (!(c->z < 0.f) ? RT_TILES_REFUSED_Z : (c->width % 64u != 0 ? RT_TILES_REFUSED_WIDTH : RT_TILES_REFUSED_BUDGET));
    } else if (!c->pose_w) {
        c->tiles_info.refused = RT_TILES_REFUSED_NO_GRID;
    }
    return RT_OK;
}

// sigma_max of a 3 x 3 matrix: sqrt of the largest eigenvalue of N N^T in object_bound's closed form (same padding and clamps)
static double sigma_max3(const double N[3][3]) {
    double S[3][3], fro2 = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            S[i][j] = N[i][0] * N[j][0] + N[i][1] * N[j][1] + N[i][2] * N[j][2];
            fro2 += N[i][j] * N[i][j];
        }
    double lam_max = fro2;
    const double q = (S[0][0] + S[1][1] + S[2][2]) / 3.0;
    const double p1 = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
    const double p2 = (S[0][0] - q) * (S[0][0] - q) + (S[1][1] - q) * (S[1][1] - q) + (S[2][2] - q) * (S[2][2] - q) + 2.0 * p1;
    const double pp = std::sqrt(p2 / 6.0);
    if (pp > 0 && std::isfinite(pp)) {
        double B[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) B[i][j] = (S[i][j] - (i == j ? q : 0.0)) / pp;
        double r = (B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0]) +
                    B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0])) / 2.0;
        r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        const double lam = q + 2.0 * pp * std::cos(std::acos(r) / 3.0);
        if (std::isfinite(lam) && lam > 0) lam_max = lam * (1.0 + 1e-6);
    } else if (pp == 0) {
        lam_max = q * (1.0 + 1e-6);
    }
    if (lam_max > fro2) lam_max = fro2;
    if (lam_max < fro2 / 3.0) lam_max = fro2 / 3.0;
    return std::sqrt(lam_max);
}

// A posed camera's table, built on the device (rt_tiles.hip; tiles.py: pose_screen_tiles is the definition, rt_grid.h has the
// derivation). The host computes what depends on the pose alone, in double - N = M^-1, sigma_max(N), eps, pad, z - eps - and
// the refusals that need no object; the device projects the registration spheres, counts, scans, fills and sorts. One
// synchronise in the middle: the host reads the record (pairs, whole-screen objects, longest list), accepts or refuses the
// table and grows the entry arrays. Refused: c->tiles stays disabled and the frame goes through the grid walk as before.
static int build_pose_tiles(rt_context* c, hipStream_t stream) {
    rt_tiles_info_t& ti = c->tiles_info;
    ti = rt_tiles_info_t{};
    const rt::PoseGrid& g = c->pose;
    const uint32_t W = g.width, H = g.height, n = c->n_objs;
    ti.col_shift = 6u;
    ti.tiles_x = W >> 6;
    ti.tiles_y = (H + 7u) / 8u;
    uint32_t refused = 0;
    if (const char* env = std::getenv("RT_POSE_TILES"))  // measurement knob: "0" keeps a posed frame on the grid walk
        if (env[0] == '0') refused |= RT_TILES_REFUSED_KNOB;
    // the grid serves the pose's rays - or, from outside its box, would serve every later ray if this table takes the primary ones
    const bool outside = c->pose_outside && c->rays_off_grid;
    const bool served = c->grid.enabled && (!c->rays_off_grid || (outside && !(c->flags & RT_FLAG_MONOLITHIC) &&
                                                                  c->h_obj_bound6.size() == rt::kBoundDoubles * (size_t)n));
    if (!served || (c->flags & RT_FLAG_LITERAL) || c->h_grid_spheres.size() != 4 * (size_t)n || n == 0) refused |= RT_TILES_REFUSED_NO_GRID;
    const double origin_d[3] = {(double)g.origin[0], (double)g.origin[1], (double)g.origin[2]};
    if (outside && served && !pose_within_reach(c, origin_d)) refused |= RT_TILES_REFUSED_FAR;
    // Compatibility, not speed: a frame of fewer than kPoseOutsideMinTiles tiles of a scene of fewer than kWavefrontMinObjects objects
    // keeps the route it had before poses outside the box were served - refused, the small-scene kernel - because the suite pins that
    // route on a 64 x 48 frame of 300 objects. MEASURED: the tiles would be faster there too (0.26 against 0.58 ms); the
    // knob RT_POSE_OUTSIDE_MIN_TILES=0 serves such frames. Larger scenes are served at every size.
    {
        uint64_t min_tiles = rt::kPoseOutsideMinTiles;
        if (const char* env = std::getenv("RT_POSE_OUTSIDE_MIN_TILES")) min_tiles = (uint64_t)std::max(0, std::atoi(env));
        if (outside && served && n < kWavefrontMinObjects && (uint64_t)ti.tiles_x * ti.tiles_y < min_tiles) refused |= RT_TILES_REFUSED_SMALL;
    }
    if (W % 64u != 0 || W == 0) refused |= RT_TILES_REFUSED_WIDTH;
    if (!(g.z < 0.f)) refused |= RT_TILES_REFUSED_Z;
    const uint64_t n_tiles64 = (uint64_t)ti.tiles_x * ti.tiles_y;
    if (n_tiles64 > rt::kPoseMaxTiles) refused |= RT_TILES_REFUSED_TILES;
    rt::PoseTileArgs a;
    std::memset(&a, 0, sizeof(a));
    {
        double M[3][3], N[3][3], norm2 = 0;
        bool finite = true;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {
                M[r][k] = (double)g.m[3 * r + k];
                norm2 += M[r][k] * M[r][k];
                finite = finite && std::isfinite(M[r][k]);
            }
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(g.origin[k]);
        const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
        if (!finite || !std::isfinite(det) || !(std::fabs(det) > 1e-12 * std::pow(norm2, 1.5))) {
            refused |= RT_TILES_REFUSED_MATRIX;
        } else {
            N[0][0] = (M[1][1] * M[2][2] - M[1][2] * M[2][1]) / det;
            N[0][1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) / det;
            N[0][2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) / det;
            N[1][0] = (M[1][2] * M[2][0] - M[1][0] * M[2][2]) / det;
            N[1][1] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) / det;
            N[1][2] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) / det;
            N[2][0] = (M[1][0] * M[2][1] - M[1][1] * M[2][0]) / det;
            N[2][1] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) / det;
            N[2][2] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) / det;
            double nrow = 0, worst = 0;
            const double zd = (double)g.z, vmax[3] = {(double)W / 2.0, (double)H / 2.0, std::fabs(zd)};
            double mv[3];
            for (int r = 0; r < 3; ++r) mv[r] = std::fabs(M[r][0]) * vmax[0] + std::fabs(M[r][1]) * vmax[1] + std::fabs(M[r][2]) * vmax[2];
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) { a.n[3 * r + k] = N[r][k]; finite = finite && std::isfinite(N[r][k]); }
                nrow = std::max(nrow, std::fabs(N[r][0]) + std::fabs(N[r][1]) + std::fabs(N[r][2]));
                worst = std::max(worst, std::fabs(N[r][0]) * mv[0] + std::fabs(N[r][1]) * mv[1] + std::fabs(N[r][2]) * mv[2]);
            }
            if (!finite) {
                refused |= RT_TILES_REFUSED_MATRIX;
            } else if (g.z < 0.f) {
                const double sigma = sigma_max3(N);
                const double eps = 3.1 * 0x1p-24 * worst + 0x1p-140 * nrow;  // rt_grid.h: |v' - v|_inf
                ti.eps = eps;
                if (!std::isfinite(eps) || !std::isfinite(sigma) || eps >= std::fabs(zd) / 2.0) {
                    refused |= RT_TILES_REFUSED_EPS;
                } else {
                    const double pad = eps * (1.0 + (double)std::max(W, H) / (2.0 * std::fabs(zd))) / (1.0 - eps / std::fabs(zd));
                    ti.pad = pad;
                    if (!(pad <= 1.0)) refused |= RT_TILES_REFUSED_EPS;
                    a.sig1 = sigma * (1.0 + 0x1p-40);
                    a.absk = 0x1p-40 * sigma;
                    a.z = zd;
                    a.zme = zd - eps;
                    a.pad = pad;
                }
            }
        }
    }
    if (refused) {
        ti.refused = refused | (outside ? RT_TILES_REFUSED_NO_GRID : 0u);  // (refused from outside the box: the grid does not serve the frame)
        return RT_OK;
    }
    for (int k = 0; k < 3; ++k) a.o[k] = (double)g.origin[k];
    a.o1 = (std::fabs(a.o[0]) + std::fabs(a.o[1])) + std::fabs(a.o[2]);
    a.half_w = (double)((float)W / 2.0f);
    a.top = (double)H - (double)((float)H / 2.0f);
    a.width = W;
    a.height = H;
    a.tiles_x = ti.tiles_x;
    a.tiles_y = ti.tiles_y;
    a.n_objs = n;
    a.budget = 256ull * n + 4096ull;
    a.whole_r = outside ? 0.25 * c->grid_diag : std::numeric_limits<double>::infinity();
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    rt::PoseTileBuffers& b = c->ptb;
    if (!c->d_pose_spheres) {  // once per context: the spheres the grid registered its objects with, as doubles
        RT_HIP(c, hipMalloc((void**)&c->d_pose_spheres, sizeof(double) * 4 * (size_t)n));
        RT_HIP(c, hipMemcpy(c->d_pose_spheres, c->h_grid_spheres.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice));
    }
    b.spheres = c->d_pose_spheres;
    if (outside) {  // spheres made for this pose's origin, from the objects' bounds (uploaded when first needed)
        if (!c->d_obj_bound6) {
            RT_HIP(c, hipMalloc((void**)&c->d_obj_bound6, sizeof(double) * rt::kBoundDoubles * (size_t)n));
            RT_HIP(c, hipMemcpy(c->d_obj_bound6, c->h_obj_bound6.data(), sizeof(double) * rt::kBoundDoubles * (size_t)n, hipMemcpyHostToDevice));
        }
        if (!c->d_outside_spheres) RT_HIP(c, hipMalloc((void**)&c->d_outside_spheres, sizeof(double) * 4 * (size_t)n));
        b.spheres = c->d_outside_spheres;
    }
    if (!b.record) {  // (the spheres may be there already: the light tiles' builder shares them)
        RT_HIP(c, hipMalloc((void**)&b.rect, sizeof(uint4) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.key, sizeof(float) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.sums, sizeof(uint32_t) * 1024));
        RT_HIP(c, hipMalloc((void**)&b.record, sizeof(rt::PoseTileRecord)));
        RT_HIP(c, hipHostMalloc((void**)&c->h_pose_record, sizeof(rt::PoseTileRecord), hipHostMallocDefault));
    }
    for (hipEvent_t& ev : c->ev_tiles)
        if (!ev) RT_HIP(c, hipEventCreate(&ev));
    if (c->ptb_tiles < n_tiles) {
        const size_t have = c->ptb_tiles;
        c->ptb_tiles = 0;
        if (int rc = grow_array(c, b.count, have, n_tiles)) return rc;
        if (int rc = grow_array(c, b.cursor, have, n_tiles)) return rc;
        if (int rc = grow_array(c, b.tile_start, have + 1, (size_t)n_tiles + 1)) return rc;
        c->ptb_tiles = n_tiles;
    }
    RT_HIP(c, hipEventRecord(c->ev_tiles[0], stream));
    hipError_t e = hipSuccess;
    if (outside) {
        rt::PoseSphereArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        for (int k = 0; k < 3; ++k) { sa.lo[k] = c->grid_box_lo[k]; sa.hi[k] = c->grid_box_hi[k]; sa.o[k] = origin_d[k]; }
        sa.cell = c->grid_cell;
        sa.S_max = c->grid_s_max;
        sa.n_objs = n;
        e = rt::launch_pose_spheres(sa, c->d_obj_bound6, c->d_pose_spheres, c->d_outside_spheres, stream);
        if (e != hipSuccess) return fail_hip(c, e, "pose spheres launch");
    }
    e = rt::launch_pose_tile_count(a, b, stream);
    if (e != hipSuccess) return fail_hip(c, e, "pose tile count launch");
    RT_HIP(c, hipEventRecord(c->ev_tiles[1], stream));
    RT_HIP(c, hipMemcpyAsync(c->h_pose_record, b.record, sizeof(rt::PoseTileRecord), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    const rt::PoseTileRecord rec = *c->h_pose_record;
    ti.n_entries = rec.pairs;
    ti.n_global = rec.n_global;
    ti.max_list = rec.max_list;
    if (rec.n_global > rt::kPoseMaxGlobal) refused |= RT_TILES_REFUSED_GLOBAL;
    if (rec.pairs > a.budget || rec.pairs > 0xfffffff0ull) refused |= RT_TILES_REFUSED_BUDGET;
    if (rec.max_list > rt::kPoseMaxList) refused |= RT_TILES_REFUSED_LIST;
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev_tiles[0], c->ev_tiles[1]));
    ti.build_device_ms = (double)ms;
    if (refused) {
        ti.refused = refused | (outside ? RT_TILES_REFUSED_NO_GRID : 0u);
        return RT_OK;
    }
    if ((unsigned long long)rec.total != rec.pairs) return fail(c, RT_ERR_STATE, "internal: the pose tiles' scan does not match their count");
    const size_t need = (size_t)rec.total + rt::kPoseMaxGlobal + 1;
    if (c->ptb_entries < need) {
        const size_t have = c->ptb_entries, cap = need + need / 4;  // grow-only, with headroom: a viewer's next pose has a few more or fewer pairs
        c->ptb_entries = 0;
        if (int rc = grow_array(c, b.scratch, have, cap)) return rc;
        if (int rc = grow_array(c, b.entries, have, cap)) return rc;
        c->ptb_entries = cap;
    }
    RT_HIP(c, hipEventRecord(c->ev_tiles[2], stream));
    e = rt::launch_pose_tile_fill(a, b, rec.total, rec.n_global, rec.max_list, stream);
    if (e != hipSuccess) return fail_hip(c, e, "pose tile fill launch");
    RT_HIP(c, hipEventRecord(c->ev_tiles[3], stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev_tiles[2], c->ev_tiles[3]));
    ti.build_device_ms += (double)ms;
    c->tiles.tile_start = b.tile_start;
    c->tiles.entries = b.entries;
    c->tiles.tiles_x = ti.tiles_x;
    c->tiles.col_shift = 6u;
    c->tiles.global_begin = rec.total;
    c->tiles.n_global = rec.n_global;
    c->tiles.width = W;
    c->tiles.posed = 1u;
    c->tiles.outside = outside ? 1u : 0u;
    c->tiles.enabled = 1u;
    ti.enabled = 1u;
    ti.source = outside ? 3u : 2u;
    c->primary_outside = outside;
    return RT_OK;
}

// The FAR condition of a pose outside the box: a primary hit point fl(o + t d) - where the secondary rays start - is off
// its exact place by at most 3e-6 (|o| + far), far = the largest distance from o to a corner of the box (no hit lies farther); that
// must stay within the 0.01 cell of slack every registration radius carries for the kernels' cell arithmetic.
bool pose_within_reach(const rt_context* c, const double o[3]) {
    double far2 = 0;
    for (int a = 0; a < 3; ++a) {
        const double d = std::max(std::fabs(o[a] - c->grid_box_lo[a]), std::fabs(c->grid_box_hi[a] - o[a]));
        far2 += d * d;
    }
    const double ol = std::sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
    const double lhs = 3e-6 * (ol + std::sqrt(far2));
    return std::isfinite(lhs) && lhs <= 0.01 * c->grid_cell;
}

// A pose outside the box renders through the grid only if its table is accepted, so the table is built BEFORE the path is chosen
// (do_launch, rt_get_rays_info, rt_get_tiles_info): afterwards primary_outside - and with it grid_in_use - is settled for the frame.
int settle_outside_pose(rt_context* c, hipStream_t stream) {
    if (c->pinhole || !c->have_rays || !c->pose_w || !c->pose_outside || !c->rays_off_grid) return RT_OK;
    if (!c->tiles_dirty && c->tiles_built_for == 6u) return RT_OK;
    RT_DEVICE(c);
    StopWatch sw;
    const int rc = refresh_screen_tiles(c, stream, 6u);
    if (rc == RT_OK) c->setup.screen_tiles_ms += sw.lap_ms();
    return rc;
}

}  // namespace rt::host
