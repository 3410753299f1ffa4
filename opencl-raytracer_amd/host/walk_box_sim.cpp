// The block walk's stop parameter on the host (tests/test_walk_box_cpu.py): no library, no GPU.
// ../csrc/rt_walk_box.h - the parameter at which a ray leaves the range of occupied block cells - computed in fp32 exactly as
// block_segment's prepare and closest_hit_blocks (../csrc/rt_wavefront.hip) compute it, and held against the exact line: a DDA
// in double lists the cells of the occupied range that the line o + t d, t >= 0, crosses, and each of them must be entered at
// a parameter <= the fp32 t_stop, or the walk would end before it looked at a cell that can hold a hit. The second property:
// t_stop never exceeds the value of the grid-box rule it replaces.
//
// Seeded cases: a range of 1..40 cells per axis inside a grid with 0..12 empty layers on each side; rays from inside the
// range, from the void and from outside the grid; axis-parallel rays, rays with zero components, rays in a face plane, rays
// through edges and corners, and rays that miss the range by one ulp either way. A ray is judged only if the walk would
// take it (walk_begin's clip finds the grid box, and the `tame` admission holds): any other ray tests every object.
// The device's reciprocal is good to 1 ulp, so every ray is judged three times: with the correctly rounded reciprocals and
// with all three moved one ulp up and one ulp down.
//
//   walk_box_sim <seed> <cases> <rays per kind> [shrink]
// shrink = 1 computes t_stop from a range one cell SMALLER on every high side: the check must then fail (the test's own test).
// Prints "judged <n> crossing <n> missing <n> cells <n> kinds <k0> ... <k7>"; exit status 1 (and the first violations) on failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/rt_walk_box.h"

namespace {

constexpr int kKinds = 8;
constexpr float kBig = 3.0e38f;

struct Grid {
    float lo[3], cell;
    int n[3], occ_lo[3], occ_hi[3];
    std::vector<double> face[3];  // face[a][i] = the fp32 face i of axis a, as a double
};

struct Ray { float o[3], d[3]; };

// walk_begin's clip against the grid box (../csrc/rt_grid.h), fp32: alive, t_enter, t_exit
bool grid_clip(const Grid& g, const Ray& r, const float inv[3], float& t0, float& t1) {
    t0 = 0.f; t1 = kBig;
    for (int a = 0; a < 3; ++a) {
        const float lo = g.lo[a], hi = walk_box_face(g.lo[a], g.cell, g.n[a]);
        float p = (lo - r.o[a]) * inv[a], q = (hi - r.o[a]) * inv[a];
        if (r.d[a] == 0.f) { const bool outside = r.o[a] < lo || r.o[a] > hi; p = outside ? kBig : -kBig; q = outside ? -kBig : kBig; }
        t0 = std::fmax(t0, std::fmin(p, q));
        t1 = std::fmin(t1, std::fmax(p, q));
    }
    return t0 <= t1;
}

struct Verdict { bool judged = false, crossing = false; uint64_t cells = 0; int bad = 0; };

Verdict judge(const Grid& g, const Ray& r, int ulp, bool shrink, bool verbose) {
    Verdict v;
    float inv[3];
    for (int a = 0; a < 3; ++a) {
        inv[a] = 1.0f / r.d[a];  // (d == 0: +-inf, never used - as on the device)
        if (ulp != 0 && std::isfinite(inv[a])) inv[a] = std::nextafter(inv[a], ulp > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity());
    }
    float t_enter, t_exit;
    if (!grid_clip(g, r, inv, t_enter, t_exit)) return v;
    float dmin = kBig;
    for (int a = 0; a < 3; ++a) dmin = std::fmin(dmin, r.d[a] != 0.f ? g.cell * std::fabs(inv[a]) : kBig);
    const float dd = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    if (!(dd > 1.0e-30f && dd < 1.0e30f && t_enter <= 4096.f * dmin)) return v;  // not `tame`: no walk
    v.judged = true;
    WalkBox b;
    const int s = shrink ? 0 : 1;
    b.lox = walk_box_face(g.lo[0], g.cell, g.occ_lo[0]); b.hix = walk_box_face(g.lo[0], g.cell, g.occ_hi[0] + s);
    b.loy = walk_box_face(g.lo[1], g.cell, g.occ_lo[1]); b.hiy = walk_box_face(g.lo[1], g.cell, g.occ_hi[1] + s);
    b.loz = walk_box_face(g.lo[2], g.cell, g.occ_lo[2]); b.hiz = walk_box_face(g.lo[2], g.cell, g.occ_hi[2] + s);
    const float t_box = walk_box_exit(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], inv[0], inv[1], inv[2], b);
    const float t_stop = walk_box_stop(t_exit, t_box, dmin);
    const float t_grid_rule = std::fmin(t_exit + 0.25f * dmin, kBig);
    if (!(t_stop <= t_grid_rule) || !(t_box >= 0.f)) {
        ++v.bad;
        if (verbose) std::printf("t_stop %.9g above the grid-box rule's %.9g (t_box %.9g)\n", (double)t_stop, (double)t_grid_rule, (double)t_box);
    }
    // the exact line against the exact range: slab clip in double, then a DDA over the range's cells
    const double o[3] = {r.o[0], r.o[1], r.o[2]}, d[3] = {r.d[0], r.d[1], r.d[2]};
    double t0 = 0.0, t1 = std::numeric_limits<double>::infinity();
    for (int a = 0; a < 3; ++a) {
        const double lo = g.face[a][g.occ_lo[a]], hi = g.face[a][g.occ_hi[a] + 1];
        if (d[a] == 0.0) {
            if (o[a] < lo || o[a] > hi) return v;  // the line misses the range
            continue;
        }
        const double p = (lo - o[a]) / d[a], q = (hi - o[a]) / d[a];
        t0 = std::fmax(t0, std::fmin(p, q));
        t1 = std::fmin(t1, std::fmax(p, q));
    }
    if (!(t0 <= t1)) return v;
    v.crossing = true;
    int idx[3];
    for (int a = 0; a < 3; ++a) {
        const double p = o[a] + t0 * d[a];
        int i = g.occ_lo[a];
        // on a face: the cell the ray is about to be in (d > 0: the upper one, d < 0: the lower one, d == 0: the lower one)
        while (i < g.occ_hi[a] && (d[a] > 0.0 ? p >= g.face[a][i + 1] : p > g.face[a][i + 1])) ++i;
        idx[a] = i;
    }
    double t = t0;
    for (int guard = 0; guard < 200; ++guard) {
        ++v.cells;
        if (!(t <= (double)t_stop)) {
            ++v.bad;
            if (verbose)
                std::printf("cell (%d %d %d) entered at %.17g > t_stop %.9g  [o %.9g %.9g %.9g d %.9g %.9g %.9g ulp %d]\n", idx[0], idx[1], idx[2], t, (double)t_stop,
                            o[0], o[1], o[2], d[0], d[1], d[2], ulp);
            return v;
        }
        int ax = -1;
        double tout = std::numeric_limits<double>::infinity();
        for (int a = 0; a < 3; ++a) {
            if (d[a] == 0.0) continue;
            const double ta = (g.face[a][idx[a] + (d[a] > 0.0 ? 1 : 0)] - o[a]) / d[a];
            if (ta < tout) { tout = ta; ax = a; }
        }
        if (ax < 0) break;
        idx[ax] += d[ax] > 0.0 ? 1 : -1;
        if (idx[ax] < g.occ_lo[ax] || idx[ax] > g.occ_hi[ax]) break;
        t = std::fmax(t, tout);
    }
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: walk_box_sim <seed> <cases> <rays per kind> [shrink]\n"); return 2; }
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    const int n_cases = std::atoi(argv[2]), per_kind = std::atoi(argv[3]);
    const bool shrink = argc > 4 && std::atoi(argv[4]) != 0;
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    auto pick = [&](int a, int b) { return a + (int)(rng() % (uint64_t)(b - a + 1)); };
    const float inf = std::numeric_limits<float>::infinity();
    uint64_t judged = 0, crossing = 0, missing = 0, cells = 0, kinds[kKinds] = {};
    int bad = 0;
    for (int c = 0; c < n_cases; ++c) {
        Grid g;
        g.cell = (float)std::exp(uni(std::log(0.05), std::log(8.0)));
        for (int a = 0; a < 3; ++a) {
            const int before = pick(0, 12), after = pick(0, 12), box = (c % 7 == 0) ? 1 : pick(1, 40);
            g.lo[a] = (float)uni(-200.0, 200.0);
            g.n[a] = before + box + after;
            g.occ_lo[a] = before;
            g.occ_hi[a] = before + box - 1;
            g.face[a].resize((size_t)g.n[a] + 1);
            for (int i = 0; i <= g.n[a]; ++i) g.face[a][(size_t)i] = (double)walk_box_face(g.lo[a], g.cell, i);
        }
        auto face_f = [&](int a, int i) { return walk_box_face(g.lo[a], g.cell, i); };
        auto inside_range = [&](int a) { return (float)uni(g.face[a][g.occ_lo[a]], g.face[a][g.occ_hi[a] + 1]); };
        auto inside_grid = [&](int a) { return (float)uni(g.face[a][0], g.face[a][g.n[a]]); };
        auto around_grid = [&](int a) { return (float)uni(g.face[a][0] - 20.0 * g.cell, g.face[a][g.n[a]] + 20.0 * g.cell); };
        auto any_dir = [&](Ray& r) { const double s = std::exp(uni(std::log(1e-3), std::log(1e3))); for (int a = 0; a < 3; ++a) r.d[a] = (float)(s * uni(-1.0, 1.0)); };
        for (int kind = 0; kind < kKinds; ++kind)
            for (int k = 0; k < per_kind; ++k) {
                Ray r;
                switch (kind) {
                case 0:  // from inside the range, any direction
                    for (int a = 0; a < 3; ++a) r.o[a] = inside_range(a);
                    any_dir(r);
                    break;
                case 1:  // from the void (or the range) inside the grid: any direction, or aimed at a point of the range
                    for (int a = 0; a < 3; ++a) r.o[a] = inside_grid(a);
                    any_dir(r);
                    if (k & 1) for (int a = 0; a < 3; ++a) r.d[a] = inside_range(a) - r.o[a];
                    break;
                case 2:  // from outside the grid, aimed at the range or anywhere
                    for (int a = 0; a < 3; ++a) r.o[a] = around_grid(a);
                    for (int a = 0; a < 3; ++a) r.d[a] = inside_range(a) - r.o[a];
                    if (k % 3 == 0) any_dir(r);
                    break;
                case 3: {  // axis-parallel
                    for (int a = 0; a < 3; ++a) { r.o[a] = (k & 1) ? inside_range(a) : inside_grid(a); r.d[a] = 0.f; }
                    r.d[pick(0, 2)] = (float)((rng() & 1) ? uni(1e-3, 1e3) : -uni(1e-3, 1e3));
                    break;
                }
                case 4: {  // one zero component (also -0)
                    for (int a = 0; a < 3; ++a) r.o[a] = (k & 1) ? inside_range(a) : inside_grid(a);
                    any_dir(r);
                    r.d[pick(0, 2)] = (k & 2) ? -0.f : 0.f;
                    break;
                }
                case 5: {  // in a face plane: of the range, of a cell inside it, of the grid
                    for (int a = 0; a < 3; ++a) r.o[a] = (k & 1) ? inside_range(a) : inside_grid(a);
                    any_dir(r);
                    const int a = pick(0, 2), which = pick(0, 3);
                    r.o[a] = face_f(a, which == 0 ? g.occ_lo[a] : which == 1 ? g.occ_hi[a] + 1 : which == 2 ? pick(g.occ_lo[a], g.occ_hi[a] + 1) : pick(0, g.n[a]));
                    r.d[a] = 0.f;
                    if (k % 5 == 0) { const int a2 = (a + 1) % 3; r.o[a2] = face_f(a2, (k & 2) ? g.occ_lo[a2] : g.occ_hi[a2] + 1); r.d[a2] = 0.f; }  // along an edge
                    break;
                }
                case 6: {  // through an edge or a corner of the range (or of a cell inside it), from anywhere
                    for (int a = 0; a < 3; ++a) r.o[a] = (k & 1) ? inside_grid(a) : around_grid(a);
                    float target[3];
                    const int free_axis = (k % 3 == 0) ? pick(0, 2) : -1;  // an edge: one coordinate anywhere along it
                    for (int a = 0; a < 3; ++a) {
                        const int which = pick(0, 2);
                        target[a] = a == free_axis ? inside_range(a) : face_f(a, which == 0 ? g.occ_lo[a] : which == 1 ? g.occ_hi[a] + 1 : pick(g.occ_lo[a], g.occ_hi[a] + 1));
                    }
                    for (int a = 0; a < 3; ++a) r.d[a] = target[a] - r.o[a];
                    if (k & 4) for (int a = 0; a < 3; ++a) r.d[a] *= 0.37f;  // (another rounding of the direction)
                    break;
                }
                default: {  // misses (or meets) the range by one ulp: a coordinate one float beside an outer face, the ray (almost) parallel to it
                    for (int a = 0; a < 3; ++a) r.o[a] = (k & 1) ? inside_range(a) : inside_grid(a);
                    any_dir(r);
                    const int a = pick(0, 2);
                    const float f = face_f(a, (k & 2) ? g.occ_lo[a] : g.occ_hi[a] + 1);
                    r.o[a] = std::nextafter(f, (k & 4) ? inf : -inf);
                    const int m = k % 3;
                    r.d[a] = m == 0 ? 0.f : (float)(((k & 8) ? 1.0 : -1.0) * std::fabs((double)r.d[(a + 1) % 3]) * (m == 1 ? 1e-7 : 1e-12));
                    break;
                }
                }
                bool ok = true;
                for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(r.o[a]) && std::isfinite(r.d[a]);
                if (!ok) continue;
                for (int ulp = -1; ulp <= 1; ++ulp) {
                    const Verdict v = judge(g, r, ulp, shrink, bad < 5);
                    if (!v.judged) continue;
                    ++judged;
                    ++kinds[kind];
                    if (v.crossing) ++crossing; else ++missing;
                    cells += v.cells;
                    bad += v.bad;
                }
            }
    }
    std::printf("judged %llu crossing %llu missing %llu cells %llu kinds", (unsigned long long)judged, (unsigned long long)crossing, (unsigned long long)missing,
                (unsigned long long)cells);
    for (int k = 0; k < kKinds; ++k) std::printf(" %llu", (unsigned long long)kinds[k]);
    std::printf("\n");
    if (bad) std::printf("violations %d\n", bad);
    return bad ? 1 : 0;
}
