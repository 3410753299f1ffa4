// rt_scene.cpp - what rt_create derives from the objects: the re-packed records, bounding spheres, the conservative grid with its walk
// records, and the closest-hit walk's block grid (rt_grid.h has the derivations).
#include "rt_context.h"

namespace rt::host {

// traversal stream: objects order[2p] and order[2p+1] (no order: 2p, 2p+1) interleaved entry by entry (rows x,y,z of mvInverse)
void pack_pairs(const rt_object_data* objs, const uint32_t* order, uint32_t n, std::vector<rt::HotPair>& pairs) {
    pairs.assign((n + 1) / 2, rt::HotPair{});
    parallel_for(pairs.size(), 8192, [&](size_t p0, size_t p1) {
        for (size_t p = p0; p < p1; ++p)
            for (uint32_t i = (uint32_t)(2 * p); i < n && i < 2 * p + 2; ++i) {
                rt::HotPair& hp = pairs[p];
                const rt_object_data& o = objs[order ? order[i] : i];
                const float* m = o.mvInverse;
                const int half = (int)(i & 1u);
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 4; ++c) hp.m[4 * r + c][half] = m[4 * c + r];
                (half ? hp.type_b : hp.type_a) = o.type;
            }
    });
    if (n & 1u) pairs[n / 2].type_b = 0xffffffffu;  // odd count: the missing partner can never be hit
}

// ObjectData[] (320 B AoS, as uploaded by the reference) -> hot traversal stream + cold shading records
void repack_objects(const rt_object_data* objs, uint32_t n, std::vector<rt::HotPair>& pairs,
                    std::vector<rt::HotObject>& hot, std::vector<rt::ColdObject>& cold) {
    hot.resize(n);
    cold.resize(n);
    pack_pairs(objs, nullptr, n, pairs);
    parallel_for(n, 16384, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
        const rt_object_data& o = objs[i];
        const float* m = o.mvInverse;
        rt::HotObject& h = hot[i];
        h.row0 = make_float4(m[0], m[4], m[8], m[12]);
        h.row1 = make_float4(m[1], m[5], m[9], m[13]);
        h.row2 = make_float4(m[2], m[6], m[10], m[14]);
        h.type = o.type;
        h.pad[0] = h.pad[1] = h.pad[2] = 0;
        if (o.type == 2u) {
            // triangle (extension): mv columns 0..2 = vertices, mvInverse column 0 = guard
            // sphere; the edges are single fp32 subtractions, exactly what the CPU statement computes per ray
            const float* v = o.mv;
            const volatile float e1x = v[4] - v[0], e1y = v[5] - v[1], e1z = v[6] - v[2];
            const volatile float e2x = v[8] - v[0], e2y = v[9] - v[1], e2z = v[10] - v[2];
            h.row0 = make_float4(v[0], v[1], v[2], m[0]);
            h.row1 = make_float4(e1x, e1y, e1z, m[1]);
            h.row2 = make_float4(e2x, e2y, e2z, m[2]);
            std::memcpy(&h.pad[0], &m[3], 4);
        }
        rt::ColdObject& c = cold[i];
        for (int r = 0; r < 4; ++r) c.mv_row[r] = make_float4(o.mv[r], o.mv[4 + r], o.mv[8 + r], o.mv[12 + r]);
        c.inv_row3 = make_float4(m[3], m[7], m[11], m[15]);
        c.amb_absorb = make_float4(o.mat.ambient[0], o.mat.ambient[1], o.mat.ambient[2], o.mat.absorption);
        c.dif_shine = make_float4(o.mat.diffuse[0], o.mat.diffuse[1], o.mat.diffuse[2], o.mat.shininess);
        float type_bits;
        std::memcpy(&type_bits, &o.type, 4);
        c.spec_type = make_float4(o.mat.specular[0], o.mat.specular[1], o.mat.specular[2], type_bits);
    }
    });
}

Bound object_bound(const rt_object_data& o) {
    const double inf = std::numeric_limits<double>::infinity();
#define make_float4(X, Y, Z, R) Bound{(double)(X), (double)(Y), (double)(Z), (double)(R), 1.0}
    if (o.type == 2u) {  // triangle: the record's guard sphere bounds every hit (the test itself demands it)
        const float* gs = o.mvInverse;
        if (!std::isfinite(gs[0] + gs[1] + gs[2]) || !(gs[3] >= 0.f)) return make_float4(0.f, 0.f, 0.f, -inf);  // never passes its guard
        if (!std::isfinite(gs[3])) return make_float4(0.f, 0.f, 0.f, inf);
        return make_float4(gs[0], gs[1], gs[2], gs[3]);
    }
    if (o.type > 2u) return make_float4(0.f, 0.f, 0.f, -inf);
    const float* m = o.mvInverse;
    double A[3][3] = {{m[0], m[4], m[8]}, {m[1], m[5], m[9]}, {m[2], m[6], m[10]}};
    const double b[3] = {m[12], m[13], m[14]};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(A[i][j]) || !std::isfinite(b[i])) return make_float4(0.f, 0.f, 0.f, inf);
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    double norm2 = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) norm2 += A[i][j] * A[i][j];
    if (!(std::fabs(det) > 1e-12 * std::pow(norm2, 1.5))) return make_float4(0.f, 0.f, 0.f, inf);
    double inv[3][3];
    inv[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
    inv[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    inv[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    inv[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
    inv[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    inv[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    inv[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
    inv[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    inv[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    double c[3], fro2 = 0;
    for (int i = 0; i < 3; ++i) {
        c[i] = -(inv[i][0] * b[0] + inv[i][1] * b[1] + inv[i][2] * b[2]);
        for (int j = 0; j < 3; ++j) fro2 += inv[i][j] * inv[i][j];
    }
    // sigma_max(A^-1)^2 = largest eigenvalue of S = A^-1 A^-T (closed form for a symmetric 3x3; double precision,
    // then padded by 1e-6 relative and never allowed above the Frobenius bound or below a third of it)
    double S[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i][j] = inv[i][0] * inv[j][0] + inv[i][1] * inv[j][1] + inv[i][2] * inv[j][2];
    double lam_max = fro2;
    {
        const double q = (S[0][0] + S[1][1] + S[2][2]) / 3.0;
        const double p1 = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
        const double p2 = (S[0][0] - q) * (S[0][0] - q) + (S[1][1] - q) * (S[1][1] - q) + (S[2][2] - q) * (S[2][2] - q) + 2.0 * p1;
        const double pp = std::sqrt(p2 / 6.0);
        if (pp > 0 && std::isfinite(pp)) {
            double Bm[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Bm[i][j] = (S[i][j] - (i == j ? q : 0.0)) / pp;
            double r = (Bm[0][0] * (Bm[1][1] * Bm[2][2] - Bm[1][2] * Bm[2][1]) - Bm[0][1] * (Bm[1][0] * Bm[2][2] - Bm[1][2] * Bm[2][0]) +
                        Bm[0][2] * (Bm[1][0] * Bm[2][1] - Bm[1][1] * Bm[2][0])) / 2.0;
            r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
            const double lam = q + 2.0 * pp * std::cos(std::acos(r) / 3.0);
            if (std::isfinite(lam) && lam > 0) lam_max = lam * (1.0 + 1e-6);
        } else if (pp == 0) {
            lam_max = q * (1.0 + 1e-6);  // S is a multiple of the identity
        }
        if (lam_max > fro2) lam_max = fro2;
        if (lam_max < fro2 / 3.0) lam_max = fro2 / 3.0;  // lambda_max >= trace / 3 always holds
    }
    const double r0 = (o.type == 0u) ? 1.0 : std::sqrt(0.75);
    const double R = r0 * std::sqrt(lam_max);
    // lambda_min >= det(S) / lambda_max^2 (the other two eigenvalues are <= lambda_max), det(S) = 1 / det(A)^2
    const double kappa2 = lam_max * lam_max * lam_max * det * det * (1.0 + 1e-6);
    if (!std::isfinite(R) || !std::isfinite(kappa2) || !(kappa2 >= 0.999) || !std::isfinite(c[0] + c[1] + c[2]))
        return make_float4(0.f, 0.f, 0.f, inf);
    Bound bd{c[0], c[1], c[2], R, kappa2 < 1.0 ? 1.0 : kappa2};
    return bd;
#undef make_float4
}

// the small-scene screen culling keeps its original, generous margins: 2^-9 of the radius and of the distance
Sphere bounding_sphere(const rt_object_data& o) {
    const Bound b = object_bound(o);
    if (!std::isfinite(b.r)) return Sphere{0.0, 0.0, 0.0, b.r};
    const double cl = std::sqrt(b.x * b.x + b.y * b.y + b.z * b.z);
    const double Reff = b.r * (1.0 + 1.0 / 512.0) + cl / 512.0;
    if (!std::isfinite(Reff)) return Sphere{0.0, 0.0, 0.0, std::numeric_limits<double>::infinity()};
    return Sphere{b.x, b.y, b.z, Reff};
}

// size proxy for ordering the shadow stream: r0 * |A^-1|_F (an upper bound of the bounding radius)
double size_proxy(const rt_object_data& o) {
    if (o.type > 1u) return -1.0;
    const float* m = o.mvInverse;
    const double A[3][3] = {{m[0], m[4], m[8]}, {m[1], m[5], m[9]}, {m[2], m[6], m[10]}};
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return 1e300;  // degenerate: test it first
    double cof2 = 0;  // |adj(A)|_F^2 ; A^-1 = adj / det
    const int nx[3] = {1, 2, 0}, pv[3] = {2, 0, 1};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double cf = A[nx[i]][nx[j]] * A[pv[i]][pv[j]] - A[nx[i]][pv[j]] * A[pv[i]][nx[j]];
            cof2 += cf * cf;
        }
    const double r = std::sqrt(cof2) / std::fabs(det) * (o.type == 0u ? 1.0 : 0.8660254037844386);
    return std::isfinite(r) ? r : 1e300;
}

static void build_walk_records(rt_context* c, const int dim[3], const std::vector<uint2>& ranges, const std::vector<float4>& es,
                        const std::vector<uint32_t>& entries) {
    c->h_walk.clear();
    c->grid.walk_rec = nullptr;
    c->grid.walk_cells = 0;
    if (std::getenv("RT_NO_WALK2")) return;  // measurement knob: the round-2 walk
    const uint64_t wnx = (uint64_t)dim[0] + 2 * kWalkBorder, wny = (uint64_t)dim[1] + 2 * kWalkBorder, wnz = (uint64_t)dim[2] + 2 * kWalkBorder;
    const uint64_t cells = wnx * wny * wnz;
    uint64_t overflow = 0;
    for (const uint2& r : ranges) overflow += r.y > 1u ? r.y - 1u : 0u;
    if ((cells + overflow) * 32ull >= 0xf0000000ull) return;
    const float ninf = -std::numeric_limits<float>::infinity();
    const uint32_t none = c->n_objs;
    std::vector<float4>& rec = c->h_walk;
    rec.assign(2 * (size_t)(cells + overflow), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t k = 0; k < (size_t)cells; ++k) {
        rec[2 * k] = make_float4(0.f, 0.f, 0.f, ninf);
        rec[2 * k + 1] = walk_link(none, 0u, ninf);
    }
    uint64_t next_free = cells;
    for (int z = 0; z < dim[2]; ++z)
        for (int y = 0; y < dim[1]; ++y)
            for (int x = 0; x < dim[0]; ++x) {
                const uint2 r = ranges[((size_t)z * dim[1] + y) * dim[0] + x];
                if (r.y == 0u) continue;
                const size_t head = (size_t)(((uint64_t)(z + kWalkBorder) * wny + (y + kWalkBorder)) * wnx + (x + kWalkBorder));
                rec[2 * head] = walk_sphere(es[r.x]);
                rec[2 * head + 1] = walk_link(entries[r.x], r.y > 1u ? (uint32_t)next_free : 0u, ninf);
                for (uint32_t j = 1; j < r.y; ++j) {
                    const size_t at = (size_t)next_free++;
                    rec[2 * at] = walk_sphere(es[r.x + j]);
                    rec[2 * at + 1] = walk_link(entries[r.x + j], j + 1u < r.y ? (uint32_t)next_free : 0u, ninf);
                }
            }
    c->grid.walk_cells = (uint32_t)cells;
    c->grid.walk_nx = (uint32_t)wnx;
    c->grid.walk_nxy = (uint32_t)(wnx * wny);
    c->grid.walk_none = none;
}

int upload_walk_records(rt_context* c) {
    if (c->h_walk.empty() || (uint64_t)c->h_walk.size() * 16ull >= 0xfffffff0ull) {
        std::vector<float4>().swap(c->h_walk);
        c->grid.walk_rec = nullptr;
        c->grid.walk_cells = 0;
        c->light_tiles.walk_base = 0;
        return RT_OK;
    }
    RT_HIP(c, hipMalloc((void**)&c->d_walk_rec, sizeof(float4) * c->h_walk.size()));
    RT_HIP(c, hipMemcpy(c->d_walk_rec, c->h_walk.data(), sizeof(float4) * c->h_walk.size(), hipMemcpyHostToDevice));
    c->grid.walk_rec = c->d_walk_rec;
    std::vector<float4>().swap(c->h_walk);
    return RT_OK;
}

// The closest-hit walk's coarse grid of 32-byte blocks (rt_grid.h: BlockGrid). Same box and same objects as the fine grid;
// an object sits in every block-cell its registration sphere reaches (the fine grid's radius with the walk-arithmetic slack
// re-sized to this grid's cell). Every entry's sphere is rounded OUTWARDS onto its block's lattice - see the struct's comment;
// the derivation of the radius: with the centre off by delta (quantisation error, known exactly, + the rounding of the
// ray's transform into lattice coordinates), "the line passes c within sqrt(w^2 + a |oc|^2)" (a = 6e-6 K^2, the pre-test's
// distance term) implies "it passes c' within sqrt(w'^2 + a |oc'|^2)" for
//     w'^2 = (w + delta)^2 + 2 delta sqrt(a) D + a (2 delta D + delta^2),     D = the largest possible |oc|,
// and a sphere that contains the original can only be "entirely behind the origin" if the original is.
static int build_walk_blocks(rt_context* c, uint32_t n, const std::vector<Bound>& sph, const std::vector<double>& rg, double cell_fine,
                      const double glo[3], const double ghi[3], double K2) {
    c->blocks = rt::BlockGrid{};
    for (int a = 0; a < 3; ++a) { c->block_occ[a] = 0; c->block_occ[3 + a] = -1; }
    SetupTrace lap("block grid");
    if (std::getenv("RT_NO_WALK3") || c->h_grid_pre.size() != n) return RT_OK;  // (measurement knob: the record walk)
    double factor = 1.67;
    if (const char* env = std::getenv("RT_WALK_BLOCK_FACTOR")) {  // tuning knob (results do not depend on it)
        const double v = std::atof(env);
        if (v >= 0.25 && v <= 16.0) factor = v;
    }
    const double cell = cell_fine * factor;
    const float cellf = (float)cell;
    const float lof[3] = {(float)glo[0], (float)glo[1], (float)glo[2]};
    const int B = (int)rt::kBlockBorder;
    int dim[3];
    uint64_t wn[3];
    for (int a = 0; a < 3; ++a) {
        dim[a] = (int)std::ceil((ghi[a] - (double)lof[a]) / (double)cellf) + 1;
        if (dim[a] < 1) dim[a] = 1;
        if (dim[a] > 1040) return RT_OK;
        wn[a] = (uint64_t)dim[a] + 2 * B;
    }
    const uint64_t n_cells = wn[0] * wn[1] * wn[2];
    if (n_cells >= (1ull << 24)) return RT_OK;  // block indices are 24 bits in a header
    if (n_cells > 64ull * n + (1ull << 18)) return RT_OK;  // a few objects in a huge box: 64 bytes per (mostly empty) cell would be all table
    float c0[3];
    for (int a = 0; a < 3; ++a) c0[a] = (float)((double)lof[a] + (0.5 - B) * (double)cellf);
    const volatile float inv_step_v = 128.0f / cellf;
    const float inv_step = inv_step_v;
    // D: no ray of a frame starts outside the grid box - build_grid's box holds every uploaded primary origin (origin_lo / hi;
    // the pinhole camera's (0,0,0) is their initial value) and secondary rays start on object surfaces - so |oc| never exceeds
    // the box's diagonal (+ the two border cells the walks may look at). The walks' `t_enter <= 4096 dmin` admission is therefore
    // always met (t_enter = 0); what their `tame` test really screens is |d|^2 (the bound and the admission rule agree)
    double Dmax = 0;
    for (int a = 0; a < 3; ++a) Dmax += (ghi[a] - glo[a] + 2 * cell) * (ghi[a] - glo[a] + 2 * cell);
    Dmax = std::sqrt(Dmax);
    const double alpha0 = 6e-6 * K2, sq_alpha0 = std::sqrt(alpha0);
    // registration (as build_grid: the cells the registration SPHERE reaches)
    std::vector<uint32_t> start(n_cells + 1, 0), entries, fill;
    auto cell_index = [&](int x, int y, int z) { return (size_t)((((uint64_t)(z + B)) * wn[1] + (uint64_t)(y + B)) * wn[0] + (uint64_t)(x + B)); };
    uint64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            for (size_t k = 0; k < (size_t)n_cells; ++k) start[k + 1] += start[k];
            total = start[n_cells];
            if (total > 0x7fffffffull) return RT_OK;
            entries.assign((size_t)total, 0);
            fill.assign(start.begin(), start.end() - 1);
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (!(rg[i] >= 0) || !std::isfinite(rg[i])) continue;
            const double rb = rg[i] - 0.01 * cell_fine + 0.01 * cell;
            const double cc[3] = {sph[i].x, sph[i].y, sph[i].z};
            int lo_i[3], hi_i[3];
            for (int a = 0; a < 3; ++a) {
                lo_i[a] = std::max((int)std::floor((cc[a] - rb - (double)lof[a]) / (double)cellf), 0);
                hi_i[a] = std::min((int)std::floor((cc[a] + rb - (double)lof[a]) / (double)cellf), dim[a] - 1);
            }
            const double r2 = rb * rb;
            auto gap2 = [&](int a, int k) {
                const double w0 = (double)lof[a] + (double)cellf * k, w1 = w0 + (double)cellf;
                const double d = cc[a] < w0 ? w0 - cc[a] : (cc[a] > w1 ? cc[a] - w1 : 0.0);
                return d * d;
            };
            for (int z = lo_i[2]; z <= hi_i[2]; ++z) {
                const double dz2 = gap2(2, z);
                for (int y = lo_i[1]; y <= hi_i[1]; ++y) {
                    const double dyz2 = dz2 + gap2(1, y);
                    if (dyz2 > r2) continue;
                    for (int x = lo_i[0]; x <= hi_i[0]; ++x) {
                        if (dyz2 + gap2(0, x) > r2) continue;
                        const size_t k = cell_index(x, y, z);
                        if (pass == 0) { start[k + 1] += 1; if (++total > 64ull * n + 1024ull) return RT_OK; }
                        else entries[fill[k]++] = i;
                    }
                }
            }
        }
    }
    lap("registration");
    // The axis-aligned range of occupied cells, per axis of the grid proper (rt_walk_box.h: a walk ends where its ray leaves it).
    // Nothing on a live context rebuilds these tables - rt_set_transforms puts a moved object on the always-list, rt_set_visibility
    // only patches record types - so the range found here holds for the context's life. No occupied cell, or RT_BLOCK_BOX_STOP=0
    // (measurement knob: the same kernels with the grid-box rule): the whole grid.
    int occ_lo[3] = {dim[0], dim[1], dim[2]}, occ_hi[3] = {-1, -1, -1};
    for (int z = 0; z < dim[2]; ++z)
        for (int y = 0; y < dim[1]; ++y) {
            const size_t row = cell_index(0, y, z);
            int x0 = 0, x1 = dim[0] - 1;
            while (x0 <= x1 && start[row + x0 + 1] == start[row + x0]) ++x0;
            if (x0 > x1) continue;
            while (start[row + x1 + 1] == start[row + x1]) --x1;
            occ_lo[0] = std::min(occ_lo[0], x0); occ_hi[0] = std::max(occ_hi[0], x1);
            occ_lo[1] = std::min(occ_lo[1], y); occ_hi[1] = std::max(occ_hi[1], y);
            occ_lo[2] = std::min(occ_lo[2], z); occ_hi[2] = std::max(occ_hi[2], z);
        }
    bool box_stop = occ_hi[0] >= 0;
    if (const char* env = std::getenv("RT_BLOCK_BOX_STOP")) box_stop = box_stop && env[0] != '0';
    if (!box_stop)
        for (int a = 0; a < 3; ++a) { occ_lo[a] = 0; occ_hi[a] = dim[a] - 1; }
    // blocks
    struct Enc { uint32_t word; uint32_t id; int s; };
    // Two sweeps over the cells, each on several threads: (1) every entry of a cell encoded on the finest of the four lattices that
    // holds it, the cell's entries ordered by lattice (stable), the blocks its chain needs counted; (2) - after a prefix sum that
    // gives every chain the indices it would get if the cells were laid out one after the other - the blocks written. The table is
    // the serial builder's, byte for byte.
    std::vector<Enc> encs((size_t)total);
    std::vector<uint32_t> chain_at((size_t)n_cells + 1, 0u);  // blocks behind the head, per cell; then their prefix sum
    std::atomic<uint64_t> hist_sum[5];
    for (auto& h : hist_sum) h.store(0);
    parallel_for((size_t)n_cells, 4096, [&](size_t k0, size_t k1) {
        uint64_t hist_local[5] = {0, 0, 0, 0, 0};
        for (size_t k = k0; k < k1; ++k) {
            const uint32_t cnt = start[k + 1] - start[k];
            if (cnt == 0) continue;
            const uint64_t wx = (uint64_t)k % wn[0], wy = ((uint64_t)k / wn[0]) % wn[1], wz = (uint64_t)k / (wn[0] * wn[1]);
            const float Cdev[3] = {std::fmaf((float)wx, cellf, c0[0]), std::fmaf((float)wy, cellf, c0[1]), std::fmaf((float)wz, cellf, c0[2])};
            Enc* enc = encs.data() + start[k];
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t i = entries[start[k] + j];
                const double w = std::fabs((double)c->h_grid_pre[i]);
                const double cc[3] = {sph[i].x, sph[i].y, sph[i].z};
                Enc e{(255u << 24) | (128u << 16) | (128u << 8) | 128u, i, 3};  // the whole cell and then some: 255 steps of cell / 16 around its centre
                bool found = false;
                for (int sc = 0; sc < 4 && !found; ++sc) {
                    const double inv = (double)inv_step * std::ldexp(1.0, -sc), step = 1.0 / inv;
                    double d2 = 0;
                    int q[3];
                    bool ok = true;
                    for (int a = 0; a < 3; ++a) {
                        const double u = (cc[a] - (double)Cdev[a]) * inv + 128.0;
                        q[a] = (int)std::floor(u + 0.5);
                        if (q[a] < 0 || q[a] > 255) ok = false;
                        d2 += (u - q[a]) * (u - q[a]);
                    }
                    if (!ok) continue;
                    // centre error in view-space units + the rounding of the device's transform of the ray origin
                    const double delta = std::sqrt(d2) * step + 1.5 * 5.97e-8 * (2.0 * Dmax + 128.0 * step);
                    const double w2 = (w + delta) * (w + delta) + 2.0 * delta * sq_alpha0 * Dmax + alpha0 * (2.0 * delta * Dmax + delta * delta);
                    const double r_lat = std::sqrt(w2) * (1.0 + 1e-6) * inv + 1e-3;
                    const int r = (int)std::ceil(r_lat);
                    if (r > 255) continue;
                    e = Enc{((uint32_t)r << 24) | ((uint32_t)q[2] << 16) | ((uint32_t)q[1] << 8) | (uint32_t)q[0], i, sc};
                    found = true;
                }
                hist_local[found ? e.s : 4] += 1;
                enc[j] = e;
            }
            std::stable_sort(enc, enc + cnt, [](const Enc& a, const Enc& b) { return a.s < b.s; });
            uint32_t n_blocks = 0;
            for (uint32_t pos = 0; pos < cnt; ++n_blocks) {
                const int sc = enc[pos].s;
                uint32_t m = 0;
                while (m < rt::kBlockEntries && pos < cnt && enc[pos].s == sc) { ++m; ++pos; }
            }
            chain_at[k + 1] = n_blocks - 1u;
        }
        for (int h = 0; h < 5; ++h) hist_sum[h].fetch_add(hist_local[h], std::memory_order_relaxed);
    });
    uint64_t hist[5], chain_blocks = 0;
    for (int h = 0; h < 5; ++h) hist[h] = hist_sum[h].load();
    for (size_t k = 0; k < (size_t)n_cells; ++k) { chain_blocks += chain_at[k + 1]; chain_at[k + 1] = (uint32_t)chain_blocks; }  // (< total <= 2^31)
    if (chain_blocks != 0 && n_cells + chain_blocks > (1ull << 24)) return RT_OK;  // block indices are 24 bits in a header
    const size_t n_blocks_all = (size_t)(n_cells + chain_blocks);
    std::vector<uint32_t> blocks(n_blocks_all * 8, 0u), ids(n_blocks_all * 8, c->n_objs);
    parallel_for((size_t)n_cells, 4096, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k) {
            const uint32_t cnt = start[k + 1] - start[k];
            if (cnt == 0) continue;
            const Enc* enc = encs.data() + start[k];
            size_t at = k, next_free = (size_t)n_cells + chain_at[k];
            uint32_t pos = 0;
            while (pos < cnt) {
                const int sc = enc[pos].s;
                uint32_t m = 0;
                while (m < rt::kBlockEntries && pos < cnt && enc[pos].s == sc) {
                    blocks[at * 8 + 1 + m] = enc[pos].word;
                    ids[at * 8 + m] = enc[pos].id;
                    ++m; ++pos;
                }
                const uint32_t next = pos < cnt ? (uint32_t)next_free++ : 0u;
                blocks[at * 8] = next | ((uint32_t)sc << 27);
                at = next;
            }
        }
    });
    if ((uint64_t)blocks.size() * 4ull >= 0xf0000000ull) return RT_OK;
    lap("encoding");
    {   // Empty cells say how many FURTHER steps of a walk are sure to stay in empty cells: the Chebyshev distance to the nearest
        // occupied cell minus one (a walk moves by one face per step), two-pass chamfer over the 26-neighbourhood of the padded
        // array, capped at 63 - in the six header bits the chain pointer and the scale leave free (24-26 and 29-31). The walk takes
        // those steps without fetching their blocks (a mesh leaves most of its grid empty: cfg5 walks 107 cells per ray).
        const int nx = (int)wn[0], ny = (int)wn[1], nz = (int)wn[2];
        std::vector<uint8_t> dist((size_t)n_cells);
        for (size_t k = 0; k < (size_t)n_cells; ++k) dist[k] = (start[k + 1] - start[k]) ? 0 : 64;
        auto at = [&](int x, int y, int z) -> uint8_t& { return dist[((size_t)z * ny + y) * nx + x]; };
        for (int pass = 0; pass < 2; ++pass) {
            const int dz = pass ? -1 : 1;
            for (int z = pass ? nz - 1 : 0; z != (pass ? -1 : nz); z += dz)
                for (int y = pass ? ny - 1 : 0; y != (pass ? -1 : ny); y += dz)
                    for (int x = pass ? nx - 1 : 0; x != (pass ? -1 : nx); x += dz) {
                        uint8_t& d = at(x, y, z);
                        if (d == 0) continue;
                        int best = d;
                        for (int oz = -1; oz <= 0; ++oz)  // the 13 neighbours already visited in this scan direction
                            for (int oy = -1; oy <= (oz ? 1 : 0); ++oy)
                                for (int ox = -1; ox <= ((oz || oy) ? 1 : -1); ++ox) {
                                    const int X = x + ox * dz, Y = y + oy * dz, Z = z + oz * dz;
                                    if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz) continue;
                                    best = std::min(best, (int)at(X, Y, Z) + 1);
                                }
                        d = (uint8_t)best;
                    }
        }
        c->blocks.take_skips = 1u;  // (cfg4 - a quarter of the cells empty, by ones and twos - still gains 0.25 ms: 15.0 -> 12.4 trips per ray)
        for (size_t k = 0; k < (size_t)n_cells; ++k) {
            if (dist[k] < 2) continue;
            const uint32_t skip = std::min<uint32_t>(63u, (uint32_t)dist[k] - 1u);
            blocks[8 * k] |= ((skip & 7u) << 24) | ((skip >> 3) << 29);
        }
    }
    lap("empty-space distances");
    RT_HIP(c, hipMalloc((void**)&c->d_walk_blocks, sizeof(uint32_t) * blocks.size()));
    RT_HIP(c, hipMalloc((void**)&c->d_walk_ids, sizeof(uint32_t) * ids.size()));
    RT_HIP(c, hipMemcpy(c->d_walk_blocks, blocks.data(), sizeof(uint32_t) * blocks.size(), hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(c->d_walk_ids, ids.data(), sizeof(uint32_t) * ids.size(), hipMemcpyHostToDevice));
    lap("uploads");
    rt::BlockGrid& b = c->blocks;
    if (const char* env = std::getenv("RT_BLOCK_SKIPS")) b.take_skips = env[0] != '0' ? 1u : 0u;  // measurement knob
    b.lox = lof[0]; b.loy = lof[1]; b.loz = lof[2];
    b.cell = cellf;
    b.inv_cell = 1.0f / cellf;
    b.nx = dim[0]; b.ny = dim[1]; b.nz = dim[2];
    b.c0x = c0[0]; b.c0y = c0[1]; b.c0z = c0[2];
    b.inv_step = inv_step;
    b.wnx = (uint32_t)wn[0]; b.wny = (uint32_t)wn[1];
    b.n_cells = (uint32_t)n_cells;
    b.blocks = c->d_walk_blocks;
    b.ids = c->d_walk_ids;
    b.none = c->n_objs;
    b.enabled = 1u;
    // (the faces as the device computes a cell wall, lo + cell * i: the whole grid gives walk_begin's own box, bit for bit)
    b.occ.lox = walk_box_face(lof[0], cellf, occ_lo[0]); b.occ.hix = walk_box_face(lof[0], cellf, occ_hi[0] + 1);
    b.occ.loy = walk_box_face(lof[1], cellf, occ_lo[1]); b.occ.hiy = walk_box_face(lof[1], cellf, occ_hi[1] + 1);
    b.occ.loz = walk_box_face(lof[2], cellf, occ_lo[2]); b.occ.hiz = walk_box_face(lof[2], cellf, occ_hi[2] + 1);
    for (int a = 0; a < 3; ++a) { c->block_occ[a] = occ_lo[a]; c->block_occ[3 + a] = occ_hi[a]; }
    if (std::getenv("RT_WALK_STATS"))
        std::fprintf(stderr, "[blocks] %d x %d x %d cells, edge %g, %llu entries, %zu blocks (%llu chained), scale 0/1/2/3/whole-cell: %llu %llu %llu %llu %llu\n",
                     dim[0], dim[1], dim[2], (double)cellf, (unsigned long long)total, blocks.size() / 8, (unsigned long long)chain_blocks,
                     (unsigned long long)hist[0], (unsigned long long)hist[1], (unsigned long long)hist[2], (unsigned long long)hist[3], (unsigned long long)hist[4]);
    if (std::getenv("RT_WALK_STATS"))
        std::fprintf(stderr, "[blocks] occupied cells %d..%d x %d..%d x %d..%d%s\n", occ_lo[0], occ_hi[0], occ_lo[1], occ_hi[1], occ_lo[2], occ_hi[2],
                     box_stop ? "" : " (the whole grid)");
    return RT_OK;
}

// Radii (rt_grid.h derives the bound): with u = 2^-24, a ray that starts `dist` from the centre c of an object
// with bounding radius R and condition number kappa can only be accepted by the reference's fp32 test if its
// line passes c within
//     sqrt(R^2 (1 + 8u) + 14 u kappa^2 dist^2) + 10.4 u kappa (|start| + |c|) + 9 u kappa^2 dist.
// Everything below uses u_eff = 2e-7 (3.3 u):  a = R sqrt(1 + 2e-6),  L = 2.2e-6 kappa (S + |c|) + 2e-6 kappa^2 D,
//   registration radius  sqrt(a^2 + 3e-6 kappa^2 D^2) + L   (D = farthest possible ray origin, S = largest |origin|)
//   pre-test radius      a + 2L + 1e-6 |c|, used with the ACTUAL distance: r^2 = w^2 + alpha dist^2, alpha = 6e-6 K^2
// (K^2 = largest kappa^2 among the objects that use the distance-dependent form, at most 4; more anisotropic
// objects carry their full registration radius instead, flagged by a negative w).
ObjectRadii grid_radii(const GridRadii& g, const Bound& b, uint32_t type, double K2_limit) {
    const double inf = std::numeric_limits<double>::infinity();
    ObjectRadii out{0.0, 0.0, false, false};
    if (b.r == -inf) { out.rg = -1.0; return out; }
    if (!std::isfinite(b.r)) { out.rg = inf; out.always = true; return out; }
    // (the expressions themselves: rt_grid_radii.h, shared with the per-pose spheres of rt_tiles.hip)
    const double cc[3] = {b.x, b.y, b.z};
    const double k2 = b.kappa2;
    const rt::RadiusTerms rt_ = rt::registration_terms(cc, b.r, k2, type, rt::farthest_corner2(cc, g.lo, g.hi), g.S_max, g.cell);
    const double cl = rt_.cl, a2 = rt_.a2, L = rt_.L, reg = rt_.reg;
    out.rg = rt_.rg;
    if (type == 2u) out.rpre = -(reg * (1.0 + 1e-6) + 1e-6 * cl);  // no distance term: its guard has none to speak of
    else if (k2 <= kKappa2Tight && k2 <= K2_limit) { out.rpre = std::sqrt(a2) + 2.0 * L + 1e-6 * cl; out.tight = true; }
    else out.rpre = -(reg * (1.0 + 1e-6) + 1e-6 * cl);
    if (!std::isfinite(out.rg) || out.rg > 0.25 * g.diag) { out.rg = inf; out.always = true; }  // as big as the scene: test it for every ray
    return out;
}

float pretest_as_stored(double rpre) {
    return rpre >= 0 ? std::nextafter((float)rpre, std::numeric_limits<float>::infinity())
                     : std::nextafter((float)rpre, -std::numeric_limits<float>::infinity());
}

// Conservative uniform grid for the large-scene trace kernels (rt_grid.h explains the margins).
int build_grid(rt_context* c, const rt_object_data* objs, uint32_t n) {
    SetupTrace lap("grid");
    c->grid = rt::GridDesc{};
    // The grid reasons about ONE line in view space per ray. That needs w = 1 starts, affine instances (checked at
    // upload) and direction.w = 0: with a non-zero direction.w the reference adds every object's own translation
    // column to the object-space direction, i.e. each object sees a different line (found by the differential fuzz).
    if (n == 0 || (c->flags & RT_FLAG_NO_GRID) || !c->affine_w || !c->primary_w_one || !(c->pinhole || c->dir_w_zero)) return RT_OK;
    std::vector<Bound> sph(n);
    double lo[3] = {c->origin_lo[0], c->origin_lo[1], c->origin_lo[2]};
    double hi[3] = {c->origin_hi[0], c->origin_hi[1], c->origin_hi[2]};
    const double inf = std::numeric_limits<double>::infinity();
    parallel_for(n, 8192, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; ++i) sph[i] = object_bound(objs[i]); });
    for (uint32_t i = 0; i < n; ++i) {
        if (!std::isfinite(sph[i].r)) continue;  // +inf: always-list, -inf: can never be hit
        const double cc[3] = {sph[i].x, sph[i].y, sph[i].z};
        const double pad = sph[i].r * 1.01;
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], cc[a] - pad);
            hi[a] = std::max(hi[a], cc[a] + pad);
        }
    }
    const double ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double diag = std::sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
    if (!(diag > 0) || !std::isfinite(diag)) return RT_OK;
    // cell edge: about two cells per object in volume, at most 256 cells per axis
    double cells_per_object = 3.0;  // (2: 22.3 ms per cfg4 frame, 3: 22.0, 4: 22.0 - since the shadow rays of the last light left the grid for the light tiles)
    if (const char* env = std::getenv("RT_GRID_CELLS_PER_OBJECT")) {  // tuning knob (results do not depend on it)
        const double v = std::atof(env);
        if (v > 0.01 && v < 1000.0) cells_per_object = v;
    }
    double cell = std::cbrt(std::max(ext[0], 1e-6) * std::max(ext[1], 1e-6) * std::max(ext[2], 1e-6) / (cells_per_object * n));
    cell = std::max(cell, std::max(ext[0], std::max(ext[1], ext[2])) / 256.0);
    if (!(cell > 0) || !std::isfinite(cell)) return RT_OK;
    // Objects that crowd on surfaces (tessellated meshes) leave most of such a grid empty and pile up in the rest:
    // refine while an occupied cell holds more than four object centres on average (random clouds: ~1.3, no change)
    {
        const double max_ext = std::max(ext[0], std::max(ext[1], ext[2]));
        std::vector<uint64_t> keys;
        const double vol = std::max(ext[0], 1e-6) * std::max(ext[1], 1e-6) * std::max(ext[2], 1e-6);
        double max_dim = c->has_triangles ? 560.0 : 280.0;  // meshes (cfg5, 1 M triangles): 280: 76.5 ms per frame, 400: 70.6, 560: 66.4, 800: 75.5
        if (const char* env = std::getenv("RT_GRID_MAX_DIM")) max_dim = std::min(1000.0, std::max(16.0, std::atof(env)));
        for (int attempt = 0; attempt < 10 && max_ext / (cell * 0.7) < max_dim && vol / std::pow(cell * 0.7, 3) < 128.0 * n; ++attempt) {
            keys.clear();
            keys.reserve(n);
            for (uint32_t i = 0; i < n; ++i) {
                if (!std::isfinite(sph[i].r)) continue;
                const uint64_t kx = (uint64_t)std::max(0.0, std::floor((sph[i].x - lo[0]) / cell));
                const uint64_t ky = (uint64_t)std::max(0.0, std::floor((sph[i].y - lo[1]) / cell));
                const uint64_t kz = (uint64_t)std::max(0.0, std::floor((sph[i].z - lo[2]) / cell));
                keys.push_back((kz << 42) | (ky << 21) | kx);
            }
            std::sort(keys.begin(), keys.end());
            const size_t distinct = (size_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
            if (distinct == 0 || (double)keys.size() / (double)distinct <= 4.0) break;
            cell *= 0.7;
        }
    }
    lap("bounds + cell size");
    // Radii: grid_radii, above, per object
    GridRadii gr;
    for (int a = 0; a < 3; ++a) { gr.lo[a] = lo[a]; gr.hi[a] = hi[a]; }
    gr.cell = cell;
    gr.diag = diag;
    gr.S_max = 0;
    for (int k = 0; k < 8; ++k) {
        const double px = (k & 1) ? hi[0] : lo[0], py = (k & 2) ? hi[1] : lo[1], pz = (k & 4) ? hi[2] : lo[2];
        gr.S_max = std::max(gr.S_max, std::sqrt(px * px + py * py + pz * pz));
    }
    const double S_max = gr.S_max;
    double K2 = 1.0;
    std::vector<double> rg(n), rpre(n);
    std::vector<uint32_t> always;
    for (uint32_t i = 0; i < n; ++i) {
        const ObjectRadii r = grid_radii(gr, sph[i], objs[i].type, inf);
        rg[i] = r.rg;
        rpre[i] = r.rpre;
        if (r.tight) K2 = std::max(K2, sph[i].kappa2);
        if (r.always) always.push_back(i);
    }
    // many scene-sized objects: a grid would not pay, stay with the brute-force stream - unless the scene holds
    // triangles, which only this path can trace (then every ray simply tests the whole always-list)
    if (always.size() > 64 && !c->has_triangles) return RT_OK;
    // the grid box: everything registered plus the ray origins, padded by one cell
    double glo[3], ghi[3];
    for (int a = 0; a < 3; ++a) { glo[a] = lo[a] - cell; ghi[a] = hi[a] + cell; }
    for (uint32_t i = 0; i < n; ++i) {
        if (!(rg[i] >= 0) || !std::isfinite(rg[i])) continue;
        const double cc[3] = {sph[i].x, sph[i].y, sph[i].z};
        for (int a = 0; a < 3; ++a) { glo[a] = std::min(glo[a], cc[a] - rg[i] - cell); ghi[a] = std::max(ghi[a], cc[a] + rg[i] + cell); }
    }
    int dim[3];
    for (int a = 0; a < 3; ++a) {
        dim[a] = (int)std::ceil((ghi[a] - glo[a]) / cell);
        if (dim[a] < 1) dim[a] = 1;
        if (dim[a] > 1040) return RT_OK;
    }
    // the box D and S_max above were taken over: a later ray buffer (rt_set_rays_device) whose origins lie inside it is covered
    // by the radii as built
    for (int a = 0; a < 3; ++a) { c->grid_box_lo[a] = lo[a]; c->grid_box_hi[a] = hi[a]; }
    c->grid_cell = cell;
    c->grid_diag = diag;
    c->grid_s_max = S_max;
    c->grid_k2 = K2;
    c->h_always = always;
    c->n_unbounded = (uint32_t)always.size();
    const float cellf = (float)cell;
    const float lof[3] = {(float)glo[0], (float)glo[1], (float)glo[2]};
    // cell range of a sphere's box, computed with the SAME float origin / cell edge the kernels use (rg already
    // contains 0.01 cell of slack for the kernels' fp32 cell arithmetic)
    auto range = [&](uint32_t i, int a, int& i0, int& i1) {
        const double cc = (a == 0 ? sph[i].x : a == 1 ? sph[i].y : sph[i].z);
        i0 = (int)std::floor((cc - rg[i] - (double)lof[a]) / (double)cellf);
        i1 = (int)std::floor((cc + rg[i] - (double)lof[a]) / (double)cellf);
        i0 = std::max(i0, 0);
        i1 = std::min(i1, dim[a] - 1);
    };
    const size_t n_cells = (size_t)dim[0] * dim[1] * dim[2];
    std::vector<uint32_t> start(n_cells + 1, 0);
    size_t total = 0;
    lap("radii + box");
    // (object, cell) pairs: counted in 64 bits against the budget as the first pass goes, and an object's BOX of cells
    // is checked before its cells are visited - many large overlapping objects must neither wrap the 32-bit prefix
    // sums nor cost billions of iterations before the grid is given up
    const uint64_t entry_budget = std::min<uint64_t>((c->has_triangles ? 1024ull : 64ull) * n + 1024ull, 0x7fffffffull);
    uint64_t counted = 0;
    std::vector<uint32_t> entries, fill;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            fill.assign(start.begin(), start.end() - 1);
            entries.assign(total, 0);
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (!(rg[i] >= 0) || !std::isfinite(rg[i])) continue;
            int x0, x1, y0, y1, z0, z1;
            range(i, 0, x0, x1); range(i, 1, y0, y1); range(i, 2, z0, z1);
            if (pass == 0) {
                if (x1 < x0 || y1 < y0 || z1 < z0) continue;
                const uint64_t box_cells = (uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1) * (uint64_t)(z1 - z0 + 1);
                if (box_cells > 8ull * entry_budget) return RT_OK;  // the sphere fills >= ~half of its box: far over budget on its own
            }
            // of the cells its box touches, only those the registration SPHERE reaches (distance from the centre to
            // the cell's box <= radius, cell walls taken from the kernels' float origin / edge, radius already
            // holding 0.01 cell of slack): a quarter fewer entries for spheres that are small against a cell
            const double cc[3] = {sph[i].x, sph[i].y, sph[i].z};
            const double r2 = rg[i] * rg[i];
            auto gap2 = [&](int a, int k) {  // squared distance from the centre to slab k of axis a
                const double w0 = (double)lof[a] + (double)cellf * k, w1 = w0 + (double)cellf;
                const double d = cc[a] < w0 ? w0 - cc[a] : (cc[a] > w1 ? cc[a] - w1 : 0.0);
                return d * d;
            };
            for (int z = z0; z <= z1; ++z) {
                const double dz2 = gap2(2, z);
                for (int y = y0; y <= y1; ++y) {
                    const double dyz2 = dz2 + gap2(1, y);
                    if (dyz2 > r2) continue;
                    for (int x = x0; x <= x1; ++x) {
                        if (dyz2 + gap2(0, x) > r2) continue;
                        const size_t cidx = ((size_t)z * dim[1] + y) * dim[0] + x;
                        if (pass == 0) { start[cidx + 1] += 1; ++counted; }
                        else entries[fill[cidx]++] = i;
                    }
                }
            }
            if (pass == 0 && counted > entry_budget) return RT_OK;  // objects too large for this cell size: not worth it
        }
        if (pass == 0) {
            lap("cell lists: count");
            for (size_t k = 0; k < n_cells; ++k) start[k + 1] += start[k];
            total = start[n_cells];
            // the kernels address these tables with 32-bit byte offsets (table_at)
            if ((uint64_t)total * 16ull >= 0xffffffffull || (uint64_t)n_cells * 32ull >= 0xffffffffull) return RT_OK;
        } else {
            lap("cell lists: fill");
            RT_HIP(c, hipMalloc((void**)&c->d_grid_entries, sizeof(uint32_t) * (total + 1)));
            // (room for the dynamic objects of rt_set_transforms behind the create-time entries; a mesh may bring more of its own)
            RT_HIP(c, hipMalloc((void**)&c->d_grid_always, sizeof(uint32_t) * (std::max<size_t>(always.size(), kMaxAlways) + 1)));
            {   // per entry: the sphere the object was registered with (rounded outwards), for the kernels' pre-test
                // pre-test radius per object, rounded away from zero; negative = "already holds the worst-case distance term"
                c->h_grid_pre.resize(n);
                for (uint32_t i = 0; i < n; ++i) c->h_grid_pre[i] = pretest_as_stored(rpre[i]);
                std::vector<float4> es(total);
                parallel_for(total, 1u << 16, [&](size_t k0, size_t k1) {
                    for (size_t k = k0; k < k1; ++k) {
                        const uint32_t i = entries[k];
                        es[k] = make_float4((float)sph[i].x, (float)sph[i].y, (float)sph[i].z, c->h_grid_pre[i]);
                    }
                });
                RT_HIP(c, hipMalloc((void**)&c->d_grid_entry_sphere, sizeof(float4) * (total + 1)));
                if (total) RT_HIP(c, hipMemcpy(c->d_grid_entry_sphere, es.data(), sizeof(float4) * total, hipMemcpyHostToDevice));
                std::vector<uint2> ranges(n_cells);
                parallel_for(n_cells, 1u << 18, [&](size_t k0, size_t k1) {
                    for (size_t k = k0; k < k1; ++k) ranges[k] = make_uint2(start[k], start[k + 1] - start[k]);
                });
                // Empty cells carry, in the unused offset word, how many FURTHER steps of a walk are sure to land in
                // empty cells too: the Chebyshev distance to the nearest occupied cell minus one (a walk moves by one
                // face per step), from a two-pass chamfer over the 26-neighbourhood, capped at 255. The grid walk
                // takes those steps without fetching their records (meshes leave most of a grid empty).
                if (n_cells <= (64ull << 20)) {
                    std::vector<uint8_t> dist(n_cells);
                    for (size_t k = 0; k < n_cells; ++k) dist[k] = ranges[k].y ? 0 : 255;
                    const int nx = dim[0], ny = dim[1], nz = dim[2];
                    auto at = [&](int x, int y, int z) -> uint8_t& { return dist[((size_t)z * ny + y) * nx + x]; };
                    for (int pass = 0; pass < 2; ++pass) {
                        const int z0 = pass ? nz - 1 : 0, z1 = pass ? -1 : nz, dz = pass ? -1 : 1;
                        for (int z = z0; z != z1; z += dz)
                            for (int y = pass ? ny - 1 : 0; y != (pass ? -1 : ny); y += dz)
                                for (int x = pass ? nx - 1 : 0; x != (pass ? -1 : nx); x += dz) {
                                    uint8_t& d = at(x, y, z);
                                    if (d == 0) continue;
                                    int best = d;
                                    // the 13 neighbours already visited in this scan direction
                                    for (int oz = -1; oz <= 0; ++oz)
                                        for (int oy = -1; oy <= (oz ? 1 : 0); ++oy)
                                            for (int ox = -1; ox <= ((oz || oy) ? 1 : -1); ++ox) {
                                                const int X = x + ox * dz, Y = y + oy * dz, Z = z + oz * dz;
                                                if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz) continue;
                                                best = std::min(best, (int)at(X, Y, Z) + 1);
                                            }
                                    d = (uint8_t)best;
                                }
                    }
                    for (size_t k = 0; k < n_cells; ++k)
                        if (ranges[k].y == 0) ranges[k].x = dist[k] > 1 ? (uint32_t)dist[k] - 1u : 0u;
                } else {
                    parallel_for(n_cells, 1u << 18, [&](size_t k0, size_t k1) {
                        for (size_t k = k0; k < k1; ++k)
                            if (ranges[k].y == 0) ranges[k].x = 0u;
                    });
                }
                RT_HIP(c, hipMalloc((void**)&c->d_grid_cell_range, sizeof(uint2) * n_cells));
                RT_HIP(c, hipMemcpy(c->d_grid_cell_range, ranges.data(), sizeof(uint2) * n_cells, hipMemcpyHostToDevice));
                // the same ranges with the first entry inline (the persistent walk's 32-byte cell records; the kernel variants
                // for scenes without triangles read these, the mesh variants the 8-byte ranges: a mesh leaves its grid mostly
                // empty, and an empty cell has nothing to inline)
                if (!c->has_triangles) {
                    std::vector<float4> rec(2 * n_cells);
                    for (size_t k = 0; k < n_cells; ++k) {
                        const bool any = ranges[k].y != 0u;
                        rec[2 * k] = any ? es[ranges[k].x] : make_float4(0.f, 0.f, 0.f, 0.f);
                        uint32_t w[4] = {ranges[k].x, ranges[k].y, any ? entries[ranges[k].x] : 0u, 0u};
                        std::memcpy(&rec[2 * k + 1], w, sizeof(w));
                    }
                    RT_HIP(c, hipMalloc((void**)&c->d_grid_cell_rec, sizeof(float4) * 2 * n_cells));
                    RT_HIP(c, hipMemcpy(c->d_grid_cell_rec, rec.data(), sizeof(float4) * 2 * n_cells, hipMemcpyHostToDevice));
                    build_walk_records(c, dim, ranges, es, entries);
                }
            }
            if (total) RT_HIP(c, hipMemcpy(c->d_grid_entries, entries.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice));
            if (!always.empty())
                RT_HIP(c, hipMemcpy(c->d_grid_always, always.data(), sizeof(uint32_t) * always.size(), hipMemcpyHostToDevice));
        }
    }
    rt::GridDesc& g = c->grid;
    g.lox = lof[0]; g.loy = lof[1]; g.loz = lof[2];
    g.cell = cellf;
    g.inv_cell = 1.0f / cellf;
    g.nx = dim[0]; g.ny = dim[1]; g.nz = dim[2];
    g.cell_range = c->d_grid_cell_range;
    g.cell_rec = c->d_grid_cell_rec;
    g.entries = c->d_grid_entries;
    g.entry_sphere = c->d_grid_entry_sphere;
    g.always = c->d_grid_always;
    g.n_always = (uint32_t)always.size();
    g.has_triangles = c->has_triangles ? 1u : 0u;
    lap("cell lists + uploads");
    {   // first-cell rule (rt_grid.h: entered_inside; RT_WALK_FIRST_CELL): the ball it uses must stay inside every object's
        // registration radius by 1e-3 cell (DDA) + the rule's own fp32 rounding (~1e-6 of the largest coordinate)
        double worst = 0.0;  // max over objects of |pre-test radius| - registration radius (normally about -0.01 cell)
        bool any = false;
        for (uint32_t i = 0; i < n; ++i) {
            if (!(rg[i] >= 0) || !std::isfinite(rg[i])) continue;
            const double d = std::fabs((double)c->h_grid_pre[i]) - rg[i];
            worst = any ? std::max(worst, d) : d;
            any = true;
        }
        const double shrink = std::max(0.0, worst + 1e-3 * cell + 2e-6 * (S_max + diag));
        g.own_shrink = std::nextafter((float)shrink, std::numeric_limits<float>::infinity());
    }
    g.pretest_alpha = std::nextafter((float)(6e-6 * K2 + 8e-6), std::numeric_limits<float>::infinity());
    g.enabled = 1u;
    if (!c->has_triangles || !std::getenv("RT_NO_TRI_BLOCKS")) {  // (meshes too since round 3: cfg5 56 -> 40 ms; the knob restores round 2's walk for them)
        StopWatch sw;
        const int rc = build_walk_blocks(c, n, sph, rg, cell, glo, ghi, K2);
        if (rc != RT_OK) return rc;
        c->setup.blocks_ms = sw.lap_ms();
    }
    c->h_grid_spheres.resize(4 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        c->h_grid_spheres[4 * i] = sph[i].x; c->h_grid_spheres[4 * i + 1] = sph[i].y; c->h_grid_spheres[4 * i + 2] = sph[i].z;
        c->h_grid_spheres[4 * i + 3] = rg[i];
    }
    // the bounds themselves, for the spheres of a pose outside the box (rt_tiles.hip: pose_spheres; such poses are refused for meshes)
    if (!c->has_triangles) {
        c->h_obj_bound6.resize(rt::kBoundDoubles * (size_t)n);
        for (uint32_t i = 0; i < n; ++i) {
            double* b = &c->h_obj_bound6[rt::kBoundDoubles * (size_t)i];
            b[0] = sph[i].x; b[1] = sph[i].y; b[2] = sph[i].z; b[3] = sph[i].r; b[4] = sph[i].kappa2; b[5] = (double)objs[i].type;
        }
    }
    return RT_OK;
}

}  // namespace rt::host
