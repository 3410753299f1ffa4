// rt_grid_radii.h - the registration radius of one object as ONE set of expressions for the host (rt_scene.cpp: grid_radii, per object
// at rt_create and per moved object) and the device (rt_tiles.hip: pose_spheres, per object and pose). rt_scene.cpp has the bound's
// derivation at grid_radii; tiles.py (grid_registration_spheres, pose_registration_spheres) is the executable definition.
// Double, nothing contracted (the library is built with -ffp-contract=off), + - * / sqrt only - correctly rounded on both sides - and
// every sum in the order written here, so that an origin inside the grid's box reproduces the context's spheres bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {

// D^2: the squared distance from the centre to the farthest corner of the box lo .. hi
__host__ __device__ inline double farthest_corner2(const double c[3], const double lo[3], const double hi[3]) {
    double D2 = 0;
    for (int a = 0; a < 3; ++a) {
        const double d0 = __builtin_fabs(c[a] - lo[a]), d1 = __builtin_fabs(hi[a] - c[a]);
        const double d = d0 < d1 ? d1 : d0;  // (std::max(d0, d1))
        D2 += d * d;
    }
    return D2;
}

// What grid_radii forms for a finite bound (centre c, radius r, kappa^2 k2) whose rays start at most sqrt(D2) from c and S from the
// world's origin: a^2, |c|, L, the registration radius before the walk's slack (`reg`) and with it (`rg`, `cell` the fine grid's edge).
struct RadiusTerms { double a2, cl, L, reg, rg; };
__host__ __device__ inline RadiusTerms registration_terms(const double c[3], double r, double k2, uint32_t type, double D2, double S, double cell) {
    RadiusTerms t;
    const double kap = __builtin_sqrt(k2);
    t.cl = __builtin_sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    t.a2 = r * r * (1.0 + 2e-6);
    t.L = 2.2e-6 * kap * (S + t.cl) + 2e-6 * k2 * __builtin_sqrt(D2);
    t.reg = __builtin_sqrt(t.a2 + 3e-6 * k2 * D2) + t.L;
    if (type == 2u) {
        // triangle: the guard |(c - start) x d|^2 <= R^2 |d|^2 is computed with an error of ~10 u R |c - start| |d|^2
        // (cross-product form), i.e. it can pass lines up to R + ~5 u D away; + the rounding of c - start itself
        t.reg = r * (1.0 + 1e-6) + 2e-6 * __builtin_sqrt(D2) + 1e-6 * (S + t.cl);
    }
    t.rg = t.reg * (1.0 + 1e-6) + 0.01 * cell;  // + slack for the kernels' fp32 cell arithmetic
    return t;
}

// A pose whose origin o lies outside the box: the same expressions with D^2 replaced by max(D^2, |o - c|^2) and S by max(S, |o|)
// (DESIGN.md 4.1). Inside the box both maxima are the box's own values.
__host__ __device__ inline double pose_far2(const double c[3], const double o[3], double D2) {
    const double d0 = o[0] - c[0], d1 = o[1] - c[1], d2 = o[2] - c[2];
    const double oc2 = (d0 * d0 + d1 * d1) + d2 * d2;
    return D2 < oc2 ? oc2 : D2;
}
__host__ __device__ inline double pose_reach(const double o[3], double S) {
    const double ol = __builtin_sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
    return S < ol ? ol : S;
}

}  // namespace rt
