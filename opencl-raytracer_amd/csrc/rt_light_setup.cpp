// rt_light_setup.cpp - what follows the lights: RT_FLAG_DEVICE_OPENCL's predicate on them, and the last light's tiles - built on the host
// for rt_create, on the device (rt_light_tiles.hip) for rt_set_lights, from one host plan.
#include "rt_context.h"

namespace rt::host {

// RT_FLAG_DEVICE_OPENCL's predicate on the lights (rt_create has the reasons): a directional light whose direction is outside the
// walks' domain, or a positional light within the padded bound of an object, makes the frame's outcome depend on the order of the
// reference's loop, which only the literal loops follow. h_obj_bounds holds object_bound's x, y, z, r per object.
bool lights_need_literal(const rt_context* c, const rt_light* L, uint32_t n_lights) {
    if (!n_lights) return false;
    for (uint32_t l = 0; l < n_lights; ++l)
        if (L[l].position[3] == 0.f && !direction_in_domain(L[l].position[0], L[l].position[1], L[l].position[2])) return true;
    std::atomic<bool> near{false};
    parallel_for(c->n_objs, 8192, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1 && !near.load(std::memory_order_relaxed); ++i) {
            const double bx = c->h_obj_bounds[4 * i], by = c->h_obj_bounds[4 * i + 1], bz = c->h_obj_bounds[4 * i + 2], br = c->h_obj_bounds[4 * i + 3];
            if (!(br >= 0.0)) continue;  // never hit
            if (!c->h_hidden.empty() && c->h_hidden[i]) continue;  // hidden (rt_set_visibility): a fresh context gives it no bound
            const double reach = br * (1.0 + 1e-4) + 1e-4 * (std::fabs(bx) + std::fabs(by) + std::fabs(bz) + br);
            for (uint32_t l = 0; l < n_lights; ++l) {
                if (L[l].position[3] == 0.f) continue;
                const double dx = (double)L[l].position[0] - bx, dy = (double)L[l].position[1] - by, dz = (double)L[l].position[2] - bz;
                if (!(dx * dx + dy * dy + dz * dz > reach * reach)) { near.store(true, std::memory_order_relaxed); break; }
            }
        }
    });
    return near.load();
}

// ---- What the two builders below decide alike, one definition each: their tables must agree to the last bit. ----
namespace {

// The block form's lattice - 16 bits per axis over the grid box - and the box's diagonal, the D of the radius' cross term.
struct Lattice { float lo[3], step; double Dbox; };
Lattice light_lattice(const rt::GridDesc& g) {
    const double ext = (double)g.cell * std::max(g.nx, std::max(g.ny, g.nz));
    const volatile float stepv = (float)(ext / 65535.0 * (1.0 + 1e-6));
    const double Dbox = std::sqrt((double)g.cell * g.nx * (double)g.cell * g.nx + (double)g.cell * g.ny * (double)g.cell * g.ny +
                                  (double)g.cell * g.nz * (double)g.cell * g.nz);
    return Lattice{{g.lox, g.loy, g.loz}, stepv, Dbox};
}

// tile count: ~1.6 sqrt(n) per axis, halved while the lists would hold more than 24 entries per object (never below 16)
uint32_t first_tile_count(uint32_t n) {
    double tile_factor = 1.6;
    if (const char* env = std::getenv("RT_LT_TILE_FACTOR")) {  // tuning knob (results do not depend on it)
        const double v = std::atof(env);
        if (v >= 0.1 && v <= 8.0) tile_factor = v;
    }
    return (uint32_t)std::min(1024.0, std::max(16.0, tile_factor * std::sqrt((double)n)));
}
bool tile_count_taken(uint64_t pairs, uint32_t T, uint32_t n) { return pairs <= 24ull * n + 4096ull || T <= 16u; }
// (object, tile) pairs a table may hold: beyond, the objects are too wide as seen from the light / the table leaves 32-bit byte offsets
uint64_t pair_budget(uint32_t n) { return 64ull * n + 4096ull; }
bool pairs_fit(uint64_t pairs, uint32_t n) { return pairs <= pair_budget(n) && pairs * 32ull < 0xffffffffull; }

// The fp32 shadow ray - start fl(P + 0.01 n), direction fl(L - P) - misses the exact line through the light by about
// 1e-7 x (the coordinates involved + the distance to the light): the pad every registration sphere gets for it, and the
// absolute slack of the kernels' distance cut, scale with the scene like the grid's own radii do (a fixed
// 1e-3 is too little once coordinates or light distances reach 1e4).
double light_pad(double coord_max, double reach_max) { return std::max(1e-3, 4e-7 * (2.0 * coord_max + reach_max)); }
float light_cut_pad(double coord_max, double reach_max) { return (float)std::max(1e-4, 4e-7 * (2.0 * coord_max + reach_max)); }

// tile origin (rounded towards -inf) and inverse tile widths (the widths 1e-6 generous) of T x T tiles over [U0, U1] x [V0, V1]
struct TileFrame { float u0, v0, inv_du, inv_dv; };
TileFrame tile_frame(double U0, double U1, double V0, double V1, uint32_t T) {
    const double du = (U1 - U0) / T * (1.0 + 1e-6), dv = (V1 - V0) / T * (1.0 + 1e-6);
    return TileFrame{std::nextafter((float)U0, -std::numeric_limits<float>::infinity()),
                     std::nextafter((float)V0, -std::numeric_limits<float>::infinity()), (float)(1.0 / du), (float)(1.0 / dv)};
}

// the 8-bit steps of the block entries' radius and key
void byte_steps(double rmax, double kmax, float& rstep, float& kstep) {
    const volatile float rstepv = (float)(rmax / 255.0 * (1.0 + 1e-5)), kstepv = (float)(std::max(kmax, 1e-3) / 255.0 * (1.0 + 1e-5));
    rstep = rstepv;
    kstep = kstepv;
}

// An enabled table as the kernels (rt::LightTiles) and rt_get_light_tiles_info see it. blocks == nullptr: no block form (the host
// builder's record form follows).
struct LightTilePlan {
    uint32_t light, T, ax, ay, az;
    double best_sign, kPad;
    float cut_pad;
    TileFrame f;
    unsigned long long n_entries;
    uint32_t max_list;
    uint4* blocks;
    uint32_t* block_ids;
    uint32_t n_blocks;
    Lattice lat;
    float rstep, kstep;
};
void publish_light_tiles(rt_context* c, const float* lp, const LightTilePlan& p, uint32_t source) {
    rt::LightTiles& lt = c->light_tiles;
    rt_light_tiles_info_t& info = c->lt_info;
    lt.lx = lp[0]; lt.ly = lp[1]; lt.lz = lp[2];
    lt.u0 = p.f.u0; lt.v0 = p.f.v0; lt.inv_du = p.f.inv_du; lt.inv_dv = p.f.inv_dv;
    lt.tiles_u = p.T; lt.tiles_v = p.T;
    lt.ax = p.ax; lt.ay = p.ay; lt.az = p.az;
    lt.sx = 1.f; lt.sy = 1.f; lt.sz = (float)-p.best_sign;
    lt.light = p.light;
    lt.cut_pad = p.cut_pad;
    lt.enabled = 1u;
    info.enabled = 1u;
    info.source = source;
    info.light = p.light;   // (light, axis and sign describe a table in use: a refused build leaves them 0)
    info.axis = p.az;
    info.sign = p.best_sign > 0 ? 1 : -1;
    info.tiles_u = info.tiles_v = p.T;
    info.n_entries = p.n_entries;
    info.max_list = p.max_list;
    info.k_pad = p.kPad;
    info.cut_pad = (double)lt.cut_pad;
    info.u0 = p.f.u0; info.v0 = p.f.v0; info.inv_du = p.f.inv_du; info.inv_dv = p.f.inv_dv;
    if (!p.blocks) return;
    lt.blocks = p.blocks;
    lt.block_ids = p.block_ids;
    lt.lat_lox = p.lat.lo[0]; lt.lat_loy = p.lat.lo[1]; lt.lat_loz = p.lat.lo[2];
    lt.lat_step = p.lat.step; lt.rstep = p.rstep; lt.kstep = p.kstep;
    lt.blocks_enabled = 1u;
    info.n_blocks = p.n_blocks;
    info.box_diagonal = p.lat.Dbox;
    info.pretest_alpha = c->grid.pretest_alpha;
    for (int a = 0; a < 3; ++a) info.lat_lo[a] = p.lat.lo[a];
    info.lat_step = p.lat.step; info.rstep = p.rstep; info.kstep = p.kstep;
}

// The lists are all a shadow ray towards the last light consults (rt_wavefront.hip: last_light_blocked), so every object that can be
// hit must be in them: one without a finite registration radius is in none. Such objects are on the grid's always-list - but so are
// rt_set_transforms' dynamic objects, which have a sphere and are listed like any other: the list's length alone says nothing.
bool has_unlisted_object(const rt_context* c) {
    if (c->grid.n_always == 0) return false;  // (every object without a finite radius is on that list)
    const double inf = std::numeric_limits<double>::infinity();
    for (size_t i = 0; i < (size_t)c->n_objs; ++i)
        if (c->h_grid_spheres[4 * i + 3] == inf) return true;
    return false;
}

}  // namespace

// Light tiles (rt_grid.h: LightTiles): the objects a shadow ray towards the LAST positional light can meet, binned by
// direction as seen from that light. shade_and_reflect's colour comes from the last light (Q1), so outside literal
// mode nearly every shadow ray goes there; rays towards other lights (stale-specular scans) keep using the grid walk.
// Needs: the conservative grid (its registration radii are the ones used here, + 1e-3 for the ray's own rounding: the
// line of a shadow ray passes the light within ~1e-5), no object without a finite registration radius, and an axis-aligned plane through the
// light with every object strictly (by its radius + 0.05) on one side - else nothing is built and the grid walk serves.
int build_light_tiles(rt_context* c, const rt_light* lights) {
    // (rt_set_lights' builder for a live context is build_light_tiles_device below: the same rules on the device, block form only)
    c->light_tiles = rt::LightTiles{};
    rt_light_tiles_info_t& info = c->lt_info;  // what rt_get_light_tiles_info reports of this build
    info = rt_light_tiles_info_t{};
    auto refuse = [&](uint32_t bit) { info.refused |= bit; return RT_OK; };
    if (!c->grid.enabled || c->kernel != RT_KERNEL_SHADE_AND_REFLECT || (c->flags & RT_FLAG_LITERAL) ||
        c->n_lights == 0 || c->h_grid_spheres.size() != 4 * (size_t)c->n_objs || c->h_grid_pre.size() != c->n_objs || has_unlisted_object(c))
        return refuse(RT_LTILES_REFUSED_NO_GRID);
    if (std::getenv("RT_NO_LIGHT_TILES")) return refuse(RT_LTILES_REFUSED_KNOB);  // measurement knob
    const uint32_t li = c->n_lights - 1u;
    const float* lp = lights[li].position;
    if (!(lp[3] != 0.f) || !std::isfinite(lp[0] + lp[1] + lp[2])) return refuse(RT_LTILES_REFUSED_LIGHT);  // directional (or garbage): no centre of projection
    const double L[3] = {lp[0], lp[1], lp[2]};
    SetupTrace lap("light tiles");
    const uint32_t n = c->n_objs;
    const double inf = std::numeric_limits<double>::infinity();
    double coord_max = std::sqrt(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]), reach_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const double r = c->h_grid_spheres[4 * i + 3];
        if (!(r >= 0) || r == inf) continue;
        double cl = 0, dl = 0;
        for (int a = 0; a < 3; ++a) {
            cl += c->h_grid_spheres[4 * i + a] * c->h_grid_spheres[4 * i + a];
            dl += (c->h_grid_spheres[4 * i + a] - L[a]) * (c->h_grid_spheres[4 * i + a] - L[a]);
        }
        coord_max = std::max(coord_max, std::sqrt(cl) + r);
        reach_max = std::max(reach_max, std::sqrt(dl) + r);
    }
    const double kPad = light_pad(coord_max, reach_max), kFront = 0.05;
    // projection axis: every registered object strictly in front of the plane through the light
    int best_axis = -1;
    double best_sign = 0, best_clear = 0;
    for (int a = 0; a < 3; ++a)
        for (double sg : {-1.0, 1.0}) {
            double clear = inf;  // min over objects of (signed depth - radius)
            for (uint32_t i = 0; i < n && clear > kFront; ++i) {
                const double r = c->h_grid_spheres[4 * i + 3];
                if (!(r >= 0) || r == inf) continue;
                clear = std::min(clear, sg * (c->h_grid_spheres[4 * i + a] - L[a]) - (r + kPad));
            }
            if (clear > kFront && clear != inf && clear > best_clear) { best_clear = clear; best_axis = a; best_sign = sg; }
        }
    if (best_axis < 0) return refuse(RT_LTILES_REFUSED_PLANE);
    // light-local frame: z' = -sign * (p - L)[axis] (objects at z' < 0), x', y' = the other two components
    const uint32_t az = (uint32_t)best_axis, ax = (az + 1u) % 3u, ay = (az + 2u) % 3u;
    const double szn = -best_sign;
    struct Rect { double u0, u1, v0, v1; };
    std::vector<Rect> rect(n, Rect{1, -1, 1, -1});
    double U0 = inf, U1 = -inf, V0 = inf, V1 = -inf;
    auto span = [&](double cx, double cz, double r, double& lo, double& hi) -> bool {
        // directions (x', z') through the origin that meet the disc (cx, cz; r), as x' / -z': tan of [phi - alpha, phi + alpha]
        const double rho = std::sqrt(cx * cx + cz * cz);
        if (!(rho > r)) return false;
        const double phi = std::atan2(cx, -cz), alpha = std::asin(std::min(1.0, r / rho));
        if (!(std::fabs(phi) + alpha < 1.5533)) return false;  // within 89 degrees of the axis, or no usable tangent
        lo = std::tan(phi - alpha);
        hi = std::tan(phi + alpha);
        // + what the kernel's fp32 (u, v) of a ray can be off by (~3e-7 (1 + |u|)), 30 times over
        lo -= 1e-5 * (1.0 + std::fabs(lo));
        hi += 1e-5 * (1.0 + std::fabs(hi));
        return true;
    };
    std::atomic<bool> no_span{false};  // an object without a usable tangent: no light tiles for this scene
    parallel_for(n, 8192, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1 && !no_span.load(std::memory_order_relaxed); ++i) {
            const double r0 = c->h_grid_spheres[4 * i + 3];
            if (!(r0 >= 0) || r0 == inf) continue;  // can never be hit
            const double r = r0 + kPad;
            const double q[3] = {c->h_grid_spheres[4 * i] - L[0], c->h_grid_spheres[4 * i + 1] - L[1], c->h_grid_spheres[4 * i + 2] - L[2]};
            const double qx = q[ax], qy = q[ay], qz = szn * q[az];
            Rect rc;
            if (!span(qx, qz, r, rc.u0, rc.u1) || !span(qy, qz, r, rc.v0, rc.v1)) { no_span.store(true, std::memory_order_relaxed); break; }
            rect[i] = rc;
        }
    });
    if (no_span.load()) return refuse(RT_LTILES_REFUSED_TANGENT);
    for (uint32_t i = 0; i < n; ++i) {
        const Rect& rc = rect[i];
        if (!(rc.u1 >= rc.u0)) continue;
        U0 = std::min(U0, rc.u0); U1 = std::max(U1, rc.u1); V0 = std::min(V0, rc.v0); V1 = std::max(V1, rc.v1);
    }
    if (!(U1 > U0) || !(V1 > V0) || !std::isfinite(U0 + U1 + V0 + V1)) return refuse(RT_LTILES_REFUSED_BOUNDS);
    lap("axis + rectangles");
    uint32_t T = first_tile_count(n);
    std::vector<uint32_t> start, entries, fill;
    uint64_t total = 0;
    TileFrame f{};
    auto tile_span = [&](double lo, double hi, float base, float inv, uint32_t& t0, uint32_t& t1) {
        // the fp32 expression the kernel evaluates, in double, with 0.01 tile of slack for the kernel's own rounding of it
        // (its (u, v) error is already inside the rectangle's padding; the product and the subtraction add < 1e-3 tile)
        const double a = std::floor((lo - (double)base) * (double)inv - 0.01), b = std::floor((hi - (double)base) * (double)inv + 0.01);
        t0 = (uint32_t)std::max(0.0, a);
        t1 = (uint32_t)std::min((double)T - 1.0, std::max(0.0, b));
    };
    for (;;) {
        f = tile_frame(U0, U1, V0, V1, T);
        start.assign((size_t)T * T + 1, 0);
        total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (!(rect[i].u1 >= rect[i].u0)) continue;
            uint32_t a0, a1, b0, b1;
            tile_span(rect[i].u0, rect[i].u1, f.u0, f.inv_du, a0, a1);
            tile_span(rect[i].v0, rect[i].v1, f.v0, f.inv_dv, b0, b1);
            total += (uint64_t)(a1 - a0 + 1) * (b1 - b0 + 1);
        }
        if (tile_count_taken(total, T, n)) break;
        T /= 2u;
    }
    if (!pairs_fit(total, n)) return refuse(RT_LTILES_REFUSED_BUDGET);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            for (size_t k = 0; k < (size_t)T * T; ++k) start[k + 1] += start[k];
            entries.assign((size_t)total, 0);
            fill.assign(start.begin(), start.end() - 1);
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (!(rect[i].u1 >= rect[i].u0)) continue;
            uint32_t a0, a1, b0, b1;
            tile_span(rect[i].u0, rect[i].u1, f.u0, f.inv_du, a0, a1);
            tile_span(rect[i].v0, rect[i].v1, f.v0, f.inv_dv, b0, b1);
            for (uint32_t b = b0; b <= b1; ++b)
                for (uint32_t a = a0; a <= a1; ++a) {
                    if (pass == 0) start[(size_t)b * T + a + 1] += 1;
                    else entries[fill[(size_t)b * T + a]++] = i;
                }
        }
    }
    std::vector<uint2> ranges((size_t)T * T);
    lap("count + fill");
    for (size_t k = 0; k < ranges.size(); ++k) ranges[k] = make_uint2(start[k], start[k + 1] - start[k]);
    // a tile's entries ordered by how far from the light the object starts: a ray's list ends at the first one that starts
    // beyond its own origin (an occluder's hit point lies between origin and light, within the registration radius of its centre)
    std::vector<float> key(n, 0.f);
    for (uint32_t i = 0; i < n; ++i) {
        const double r0 = c->h_grid_spheres[4 * i + 3];
        if (!(r0 >= 0) || r0 == inf) continue;
        const double q[3] = {c->h_grid_spheres[4 * i] - L[0], c->h_grid_spheres[4 * i + 1] - L[1], c->h_grid_spheres[4 * i + 2] - L[2]};
        const double d = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - (r0 + kPad);
        key[i] = std::nextafter((float)(d * (1.0 - 1e-6)), -std::numeric_limits<float>::infinity());
    }
    parallel_for(ranges.size(), 1024, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t)
            std::sort(entries.begin() + start[t], entries.begin() + start[t + 1], [&](uint32_t a, uint32_t b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
    });
    lap("keys + per-tile sorts");
    // The lists as RECORDS (tile_range + two float4 per entry) are what the kernels read where the block form below is not
    // built; with blocks they are never touched, and 56 MB of them (cfg4) are neither made nor uploaded.
    std::vector<float4> recs;
    auto upload_records = [&]() -> int {
        recs.resize(2 * (size_t)total);
        for (size_t k = 0; k < (size_t)total; ++k) {
            const uint32_t i = entries[k];
            float id_bits;
            std::memcpy(&id_bits, &i, 4);
            recs[2 * k] = make_float4((float)c->h_grid_spheres[4 * i], (float)c->h_grid_spheres[4 * i + 1], (float)c->h_grid_spheres[4 * i + 2], c->h_grid_pre[i]);
            recs[2 * k + 1] = make_float4(key[i], id_bits, 0.f, 0.f);
        }
        RT_HIP(c, hipMalloc((void**)&c->d_lt_range, sizeof(uint2) * ranges.size()));
        RT_HIP(c, hipMalloc((void**)&c->d_lt_records, sizeof(float4) * (recs.size() + 2)));
        RT_HIP(c, hipMemcpy(c->d_lt_range, ranges.data(), sizeof(uint2) * ranges.size(), hipMemcpyHostToDevice));
        if (total) RT_HIP(c, hipMemcpy(c->d_lt_records, recs.data(), sizeof(float4) * recs.size(), hipMemcpyHostToDevice));
        c->light_tiles.tile_range = c->d_lt_range;
        c->light_tiles.records = c->d_lt_records;
        return RT_OK;
    };
    rt::LightTiles& lt = c->light_tiles;
    LightTilePlan plan{li, T, ax, ay, az, best_sign, kPad, light_cut_pad(coord_max, reach_max), f, total, 0u, nullptr, nullptr, 0u, Lattice{}, 0.f, 0.f};
    for (const uint2& r : ranges) plan.max_list = std::max(plan.max_list, r.y);
    if ((!c->has_triangles || !std::getenv("RT_NO_TRI_BLOCKS")) && total && !std::getenv("RT_NO_LT_BLOCKS")) {
        // ... and as 32-byte blocks of three candidates (LightTiles::blocks). Lattice: 16 bits per axis over the grid box; every
        // sphere rounded outwards exactly as build_walk_blocks does it (the device's own fma for the centre, the known
        // quantisation error d added to the radius with the cross term of the distance-dependent tolerance:
        // w'^2 = (w + d)^2 + 2 d sqrt(a) D + a (2 d D + d^2), a = the pre-test's alpha, D = the grid box's diagonal).
        const Lattice lat = light_lattice(c->grid);
        const float* lof = lat.lo;
        const float stepf = lat.step;
        const double Dbox = lat.Dbox, a0 = (double)c->grid.pretest_alpha, sa0 = std::sqrt(a0);
        std::vector<uint16_t> q(3 * (size_t)n, 0);
        std::vector<double> wq(n, 0.0);
        double rmax = 0.0, kmax = 0.0;
        bool ok = stepf > 0.f && std::isfinite(stepf);
        for (uint32_t i = 0; i < n && ok; ++i) {
            if (!(rect[i].u1 >= rect[i].u0)) continue;
            double d2 = 0;
            for (int a = 0; a < 3; ++a) {
                const double cc = c->h_grid_spheres[4 * i + a];
                double u = std::floor((cc - (double)lof[a]) / (double)stepf + 0.5);
                if (!(u >= 0.0) || !(u <= 65535.0)) { ok = false; break; }  // (a centre outside the grid box: cannot happen for registered objects)
                q[3 * i + a] = (uint16_t)u;
                const double dec = (double)std::fmaf((float)u, stepf, lof[a]);
                d2 += (cc - dec) * (cc - dec);
            }
            const double w = std::fabs((double)c->h_grid_pre[i]), d = std::sqrt(d2);  // (the ray is not transformed here: no further term)
            const double w2 = (w + d) * (w + d) + 2.0 * d * sa0 * Dbox + a0 * (2.0 * d * Dbox + d * d);
            wq[i] = std::sqrt(w2) * (1.0 + 2e-6);
            rmax = std::max(rmax, wq[i]);
            kmax = std::max(kmax, (double)key[i]);
        }
        float rstepf, kstepf;
        byte_steps(rmax, kmax, rstepf, kstepf);
        // Block indices travel in 24 bits: the walks keep the position inside a block they come back to in bits 24+ of their
        // cursor (rt_grid.h: kLtBlockIndexBits; trace_segment / walk_segment mask with kLtBlockIndexMask). Count the blocks the
        // table will hold EXACTLY - a head per tile plus the further blocks of every chain - and keep the record form beyond
        // that (round 3 checked heads + total / 3 against 2^30, which the masks do not honour: ADVICE r3).
        uint64_t n_lt_blocks = ranges.size();
        for (size_t t = 0; t < ranges.size(); ++t) n_lt_blocks += ranges[t].y > 3u ? (ranges[t].y - 1u) / 3u : 0u;
        ok = ok && rstepf > 0.f && std::isfinite(rstepf) && std::isfinite(kstepf) && rt::light_tile_blocks_fit(n_lt_blocks);
        if (ok) {
            const size_t heads = ranges.size();
            // what an entry's two words hold depends on its object alone: the centre on the lattice, the radius rounded UP and
            // the key rounded DOWN to their 8-bit steps - once per object, not once per entry (1.75 M entries for 100 k objects)
            std::vector<uint2> packed(n, make_uint2(0u, 0u));
            for (uint32_t i = 0; i < n; ++i) {
                if (!(rect[i].u1 >= rect[i].u0)) continue;
                uint32_t r8 = (uint32_t)std::ceil(wq[i] / (double)rstepf);
                while (r8 < 255u && (double)((float)r8 * rstepf) < wq[i]) ++r8;  // (the device's own product must not fall short)
                if (r8 > 255u) r8 = 255u;
                double kk = std::floor(std::max((double)key[i], 0.0) / (double)kstepf * (1.0 - 1e-6));
                uint32_t k8 = (uint32_t)std::min(255.0, std::max(0.0, kk));
                while (k8 > 0u && (double)((float)k8 * kstepf) > (double)key[i]) --k8;  // (rounded DOWN: an entry may only look nearer to the light)
                packed[i] = make_uint2((uint32_t)q[3 * i] | ((uint32_t)q[3 * i + 1] << 16), (uint32_t)q[3 * i + 2] | (r8 << 16) | (k8 << 24));
            }
            // tile t's head is block t; the further blocks of the chains follow the heads in tile order
            std::vector<uint32_t> chain_at(heads + 1, 0u);
            for (size_t t = 0; t < heads; ++t) chain_at[t + 1] = chain_at[t] + (ranges[t].y > 3u ? (ranges[t].y - 1u) / 3u : 0u);
            const size_t n_blocks = heads + chain_at[heads];
            std::vector<uint32_t> blk(8 * n_blocks, 0u), bid(4 * n_blocks, c->n_objs);
            const uint32_t empty_hi = 0xff000000u;
            parallel_for(n_blocks, 1u << 12, [&](size_t b0, size_t b1) {
                for (size_t b = b0; b < b1; ++b) blk[8 * b + 3] = blk[8 * b + 5] = blk[8 * b + 7] = empty_hi;
            });
            parallel_for(heads, 1024, [&](size_t t0, size_t t1) {
                for (size_t t = t0; t < t1; ++t) {
                    size_t at = t, next = heads + chain_at[t];
                    for (uint32_t j = 0; j < ranges[t].y; ++j) {
                        const uint32_t slot = j % 3u;
                        if (j && slot == 0u) {  // the chain goes on in its next block behind the heads
                            blk[8 * at] = (uint32_t)next;
                            at = next++;
                        }
                        const uint32_t i = entries[(size_t)ranges[t].x + j];
                        blk[8 * at + 2 + 2 * slot] = packed[i].x;
                        blk[8 * at + 3 + 2 * slot] = packed[i].y;
                        bid[4 * at + slot] = i;
                    }
                }
            });
            RT_HIP(c, hipMalloc((void**)&c->d_lt_blocks, sizeof(uint32_t) * blk.size()));
            RT_HIP(c, hipMalloc((void**)&c->d_lt_block_ids, sizeof(uint32_t) * bid.size()));
            RT_HIP(c, hipMemcpy(c->d_lt_blocks, blk.data(), sizeof(uint32_t) * blk.size(), hipMemcpyHostToDevice));
            RT_HIP(c, hipMemcpy(c->d_lt_block_ids, bid.data(), sizeof(uint32_t) * bid.size(), hipMemcpyHostToDevice));
            plan.blocks = c->d_lt_blocks;
            plan.block_ids = c->d_lt_block_ids;
            plan.n_blocks = (uint32_t)n_blocks;
            plan.lat = lat;
            plan.rstep = rstepf; plan.kstep = kstepf;
            lap("blocks + uploads");
            if (std::getenv("RT_WALK_STATS"))
                std::fprintf(stderr, "[light tiles] %u x %u tiles, %llu entries, %zu blocks (%zu behind the heads), lattice step %g, radius step %g, key step %g\n",
                             T, T, (unsigned long long)total, blk.size() / 8, blk.size() / 8 - heads, (double)stepf, (double)rstepf, (double)kstepf);
        }
    }
    publish_light_tiles(c, lp, plan, 1u);
    if (!lt.blocks_enabled) {
        const int rc = upload_records();
        if (rc != RT_OK) return rc;
        lap("records + uploads");
    }
    if (!c->h_walk.empty() && total && !lt.blocks_enabled) {  // (no blocks - RT_NO_LT_BLOCKS: the lists as records of the unified walk, each tile's chained to its end)
        const uint64_t base = c->h_walk.size() / 2;
        if ((base + total) * 32ull < 0xf0000000ull) {
            c->h_walk.resize(2 * (size_t)(base + total));
            for (size_t t = 0; t < ranges.size(); ++t)
                for (uint32_t j = 0; j < ranges[t].y; ++j) {
                    const size_t k = (size_t)ranges[t].x + j;
                    c->h_walk[2 * (base + k)] = walk_sphere(recs[2 * k]);
                    c->h_walk[2 * (base + k) + 1] = walk_link(entries[k], j + 1u < ranges[t].y ? (uint32_t)(base + k + 1) : 0u, recs[2 * k + 1].x);
                }
            lt.walk_base = (uint32_t)base;
        }
    }
    return RT_OK;
}

// A live context's light tiles, rebuilt on the device for new lights (rt_set_lights; rt_light_tiles.hip has the passes,
// light_tiles.py the definition). The host keeps what build_light_tiles decides between its loops - kPad and the projection axis
// from eight reduced numbers, the tile count T from the pair totals of every candidate of the halving rule, the tile origin and
// the 8-bit steps from the reduced bounds, every refusal - and synchronises four times to read them. Block form only; refused:
// c->light_tiles stays disabled and the last light's shadow rays go through the grid walk, same bits.
int build_light_tiles_device(rt_context* c, const rt_light* lights) {
    c->light_tiles = rt::LightTiles{};
    rt_light_tiles_info_t& info = c->lt_info;
    info = rt_light_tiles_info_t{};
    auto refuse = [&](uint32_t bit) { info.enabled = 0; info.source = 0; info.refused |= bit; return RT_OK; };
    const uint32_t n = c->n_objs;
    if (!c->grid.enabled || c->kernel != RT_KERNEL_SHADE_AND_REFLECT || (c->base_flags & RT_FLAG_LITERAL) ||
        c->n_lights == 0 || n == 0 || c->h_grid_spheres.size() != 4 * (size_t)n || c->h_grid_pre.size() != n || has_unlisted_object(c))
        return refuse(RT_LTILES_REFUSED_NO_GRID);
    if (std::getenv("RT_NO_LIGHT_TILES")) return refuse(RT_LTILES_REFUSED_KNOB);
    if (const char* env = std::getenv("RT_LIGHT_TILES_DEVICE"))  // measurement knob: "0" leaves a replaced light to the grid walk
        if (env[0] == '0') return refuse(RT_LTILES_REFUSED_KNOB);
    const uint32_t li = c->n_lights - 1u;
    const float* lp = lights[li].position;
    if (!(lp[3] != 0.f) || !std::isfinite(lp[0] + lp[1] + lp[2])) return refuse(RT_LTILES_REFUSED_LIGHT);
    if ((c->has_triangles && std::getenv("RT_NO_TRI_BLOCKS")) || std::getenv("RT_NO_LT_BLOCKS")) return refuse(RT_LTILES_REFUSED_BLOCKS);
    const Lattice lat = light_lattice(c->grid);
    if (!(lat.step > 0.f) || !std::isfinite(lat.step) || !std::isfinite(lat.Dbox)) return refuse(RT_LTILES_REFUSED_BLOCKS);

    hipStream_t stream = c->stream;
    rt::LightTileBuffers& b = c->ltb;
    if (!c->d_pose_spheres) {  // the registration spheres as doubles: shared with the pose tiles' builder
        RT_HIP(c, hipMalloc((void**)&c->d_pose_spheres, sizeof(double) * 4 * (size_t)n));
        RT_HIP(c, hipMemcpy(c->d_pose_spheres, c->h_grid_spheres.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice));
    }
    if (!b.record) {  // once per context: everything sized by the object count
        RT_HIP(c, hipMalloc((void**)&c->d_lt_pre, sizeof(float) * (size_t)n));
        RT_HIP(c, hipMemcpy(c->d_lt_pre, c->h_grid_pre.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
        RT_HIP(c, hipMalloc((void**)&b.span, sizeof(double4) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.wq, sizeof(double) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.packed, sizeof(uint2) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.lists.rect, sizeof(uint4) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.lists.key, sizeof(float) * (size_t)n));
        RT_HIP(c, hipMalloc((void**)&b.lists.sums, sizeof(uint32_t) * 1024));
        RT_HIP(c, hipMalloc((void**)&b.chains.sums, sizeof(uint32_t) * 1024));
        RT_HIP(c, hipMalloc((void**)&b.lists.record, sizeof(rt::PoseTileRecord)));
        RT_HIP(c, hipMalloc((void**)&b.chains.record, sizeof(rt::PoseTileRecord)));
        RT_HIP(c, hipHostMalloc((void**)&c->h_lt_record, sizeof(rt::LightTileRecord), hipHostMallocDefault));
        RT_HIP(c, hipHostMalloc((void**)&c->h_lt_lists, 2 * sizeof(rt::PoseTileRecord), hipHostMallocDefault));
        RT_HIP(c, hipMalloc((void**)&b.record, sizeof(rt::LightTileRecord)));
    }
    b.spheres = c->d_pose_spheres;
    b.pre = c->d_lt_pre;
    for (hipEvent_t& ev : c->ev_lt)
        if (!ev) RT_HIP(c, hipEventCreate(&ev));
    double device_ms = 0.0;
    auto stage_ms = [&](int k) -> int {
        float ms = 0.f;
        RT_HIP(c, hipEventElapsedTime(&ms, c->ev_lt[2 * k], c->ev_lt[2 * k + 1]));
        device_ms += (double)ms;
        info.build_device_ms = device_ms;
        return RT_OK;
    };

    rt::LightTileArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_objs = n;
    for (int k = 0; k < 3; ++k) { a.L[k] = (double)lp[k]; a.lat_lo[k] = lat.lo[k]; }
    a.lat_step = lat.step;
    a.Dbox = lat.Dbox;
    a.alpha = (double)c->grid.pretest_alpha;
    a.budget = pair_budget(n);

    // stage 1: the eight numbers kPad and the projection axis come from
    {
        rt::LightTileRecord& r = *c->h_lt_record;
        std::memset(&r, 0, sizeof(r));
        const unsigned long long lowest = rt::lt_key_of(-std::numeric_limits<double>::infinity()), highest = rt::lt_key_of(std::numeric_limits<double>::infinity());
        r.coord_max = r.reach_max = r.U1 = r.V1 = r.rmax = r.kmax = lowest;
        r.U0 = r.V0 = highest;
        for (int k = 0; k < 6; ++k) r.clear[k] = highest;
    }
    RT_HIP(c, hipMemcpyAsync(b.record, c->h_lt_record, sizeof(rt::LightTileRecord), hipMemcpyHostToDevice, stream));
    RT_HIP(c, hipEventRecord(c->ev_lt[0], stream));
    hipError_t e = rt::launch_light_tile_reduce(a, b, stream);
    if (e != hipSuccess) return fail_hip(c, e, "light tile reduction launch");
    RT_HIP(c, hipEventRecord(c->ev_lt[1], stream));
    RT_HIP(c, hipMemcpyAsync(c->h_lt_record, b.record, sizeof(rt::LightTileRecord), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (int rc = stage_ms(0)) return rc;
    const double inf = std::numeric_limits<double>::infinity();
    double coord_max, reach_max, kPad;
    int best_axis = -1;
    double best_sign = 0, best_clear = 0;
    {
        const rt::LightTileRecord r = *c->h_lt_record;
        coord_max = std::max(std::sqrt(a.L[0] * a.L[0] + a.L[1] * a.L[1] + a.L[2] * a.L[2]), rt::lt_unkey(r.coord_max));
        reach_max = std::max(0.0, rt::lt_unkey(r.reach_max));
        kPad = light_pad(coord_max, reach_max);
        const double kFront = 0.05;
        for (int ax = 0; ax < 3; ++ax)
            for (int s = 0; s < 2; ++s) {  // (the host builder's order: -1, then +1)
                const double m = rt::lt_unkey(r.clear[2 * ax + s]);
                const double clear = m - kPad;
                if (m != inf && clear > kFront && clear != inf && clear > best_clear) { best_clear = clear; best_axis = ax; best_sign = s ? 1.0 : -1.0; }
            }
    }
    info.k_pad = kPad;
    info.cut_pad = (double)light_cut_pad(coord_max, reach_max);
    if (best_axis < 0) return refuse(RT_LTILES_REFUSED_PLANE);
    const uint32_t az = (uint32_t)best_axis, ax = (az + 1u) % 3u, ay = (az + 2u) % 3u;
    const double szn = -best_sign;

    // stage 2: spans, keys, radii; the pair totals of every candidate T
    a.kPad = kPad;
    a.sz = szn;
    a.ax = ax; a.ay = ay; a.az = az;
    for (uint32_t T = first_tile_count(n);; T /= 2u) {
        a.cand[a.n_cand++] = T;
        if (T <= 16u || a.n_cand == rt::kLtMaxCandidates) break;
    }
    RT_HIP(c, hipEventRecord(c->ev_lt[2], stream));
    e = rt::launch_light_tile_spans(a, b, stream);
    if (e != hipSuccess) return fail_hip(c, e, "light tile span launch");
    RT_HIP(c, hipEventRecord(c->ev_lt[3], stream));
    RT_HIP(c, hipMemcpyAsync(c->h_lt_record, b.record, sizeof(rt::LightTileRecord), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (int rc = stage_ms(1)) return rc;
    const rt::LightTileRecord rec = *c->h_lt_record;
    if (rec.flags & rt::kLtFlagNoTangent) return refuse(RT_LTILES_REFUSED_TANGENT);
    const double U0 = rt::lt_unkey(rec.U0), U1 = rt::lt_unkey(rec.U1), V0 = rt::lt_unkey(rec.V0), V1 = rt::lt_unkey(rec.V1);
    if (rec.n_listed == 0 || !(U1 > U0) || !(V1 > V0) || !std::isfinite(U0 + U1 + V0 + V1)) return refuse(RT_LTILES_REFUSED_BOUNDS);
    uint32_t T = a.cand[a.n_cand - 1u];
    unsigned long long pairs = rec.pairs[a.n_cand - 1u];
    for (uint32_t k = 0; k < a.n_cand; ++k)
        if (tile_count_taken(rec.pairs[k], a.cand[k], n)) { T = a.cand[k]; pairs = rec.pairs[k]; break; }
    info.tiles_u = info.tiles_v = T;
    info.n_entries = pairs;
    if (pairs == 0 || !pairs_fit(pairs, n)) return refuse(RT_LTILES_REFUSED_BUDGET);
    const TileFrame f = tile_frame(U0, U1, V0, V1, T);
    a.T = T;
    a.u0 = f.u0; a.v0 = f.v0; a.inv_du = f.inv_du; a.inv_dv = f.inv_dv;
    byte_steps(std::max(0.0, rt::lt_unkey(rec.rmax)), std::max(0.0, rt::lt_unkey(rec.kmax)), a.rstep, a.kstep);
    info.u0 = a.u0; info.v0 = a.v0; info.inv_du = a.inv_du; info.inv_dv = a.inv_dv;
    if ((rec.flags & rt::kLtFlagOffLattice) || !(a.rstep > 0.f) || !std::isfinite(a.rstep) || !(a.kstep > 0.f) || !std::isfinite(a.kstep) ||
        !std::isfinite(a.inv_du) || !std::isfinite(a.inv_dv))
        return refuse(RT_LTILES_REFUSED_BLOCKS);

    // stage 3: tile rectangles at T, count, scan, chain blocks
    const uint32_t n_tiles = T * T;  // <= 2^20
    if (c->ltb_tiles < n_tiles) {
        const size_t have = c->ltb_tiles;
        c->ltb_tiles = 0;
        for (uint32_t** p : {&b.lists.count, &b.lists.cursor, &b.lists.tile_start, &b.chains.count, &b.chains.cursor, &b.chains.tile_start})
            if (int rc = grow_array(c, *p, have + 1, (size_t)n_tiles + 1)) return rc;
        c->ltb_tiles = n_tiles;
    }
    RT_HIP(c, hipEventRecord(c->ev_lt[4], stream));
    e = rt::launch_light_tile_count(a, b, stream);
    if (e != hipSuccess) return fail_hip(c, e, "light tile count launch");
    RT_HIP(c, hipEventRecord(c->ev_lt[5], stream));
    RT_HIP(c, hipMemcpyAsync(&c->h_lt_lists[0], b.lists.record, sizeof(rt::PoseTileRecord), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipMemcpyAsync(&c->h_lt_lists[1], b.chains.record, sizeof(rt::PoseTileRecord), hipMemcpyDeviceToHost, stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (int rc = stage_ms(2)) return rc;
    const rt::PoseTileRecord lists = c->h_lt_lists[0], chains = c->h_lt_lists[1];
    info.n_entries = lists.pairs;
    info.max_list = lists.max_list;
    if (lists.pairs == 0 || !pairs_fit(lists.pairs, n)) return refuse(RT_LTILES_REFUSED_BUDGET);
    if (lists.max_list > rt::kLtMaxList) return refuse(RT_LTILES_REFUSED_LIST);
    if ((unsigned long long)lists.total != lists.pairs) return fail(c, RT_ERR_STATE, "internal: the light tiles' scan does not match their count");
    const uint64_t n_blocks64 = (uint64_t)n_tiles + chains.total;
    if (!rt::light_tile_blocks_fit(n_blocks64)) return refuse(RT_LTILES_REFUSED_BLOCKS);
    const uint32_t n_blocks = (uint32_t)n_blocks64;

    // stage 4: fill, rank sort, pack, heads and chains
    const size_t need = (size_t)lists.total + 1;
    if (c->ltb_entries < need) {
        const size_t have = c->ltb_entries, cap = need + need / 4;  // grow-only, with headroom: a dragged light's next table is about as large
        c->ltb_entries = 0;
        if (int rc = grow_array(c, b.lists.scratch, have, cap)) return rc;
        if (int rc = grow_array(c, b.lists.entries, have, cap)) return rc;
        c->ltb_entries = cap;
    }
    if (c->ltb_blocks < n_blocks) {
        const size_t have = c->ltb_blocks, cap = (size_t)n_blocks + n_blocks / 4;
        c->ltb_blocks = 0;
        if (int rc = grow_array(c, b.blocks, 2 * have, 2 * cap)) return rc;
        if (int rc = grow_array(c, b.block_ids, 4 * have, 4 * cap)) return rc;
        c->ltb_blocks = cap;
    }
    RT_HIP(c, hipEventRecord(c->ev_lt[6], stream));
    e = rt::launch_light_tile_fill(a, b, lists.total, lists.max_list, n_blocks, stream);
    if (e != hipSuccess) return fail_hip(c, e, "light tile fill launch");
    RT_HIP(c, hipEventRecord(c->ev_lt[7], stream));
    RT_HIP(c, hipStreamSynchronize(stream));
    if (int rc = stage_ms(3)) return rc;

    publish_light_tiles(c, lp, LightTilePlan{li, T, ax, ay, az, best_sign, kPad, light_cut_pad(coord_max, reach_max), f, lists.pairs, lists.max_list,
                                             b.blocks, b.block_ids, n_blocks, lat, a.rstep, a.kstep}, 2u);
    return RT_OK;
}

}  // namespace rt::host
