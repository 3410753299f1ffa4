// The block walk's stop: the parameter at which a ray leaves the axis-aligned range of OCCUPIED block cells
// (rt_wavefront.hip: block_segment, closest_hit_blocks; rt_scene.cpp: build_walk_blocks stores the range).
//
// A walk used to end where its ray leaves the grid box. That box also holds the ray origins known when the context was
// made - a pinhole camera far in front of the objects, say - so a reflection ray that hits nothing crossed all the empty
// layers between the objects and the box's faces, a few cells per trip. No cell outside the occupied range has an entry,
// and a hit at T has its point inside the object's registration sphere, i.e. in a cell that lists the object (rt_grid.h,
// the invariant above kWalkSlackCells) - a cell of the occupied range, which the ray therefore has not left at T. So the
// walk may stop where the ray leaves that range: the grid-box rule with a smaller box whose faces are cell faces.
//
// This is walk_begin's slab clip (rt_grid.h), same arithmetic and same d == 0 convention, reduced to the exit parameter
// and clipped to [0, inf). A ray that misses the range gets a small value - its walk ends at the first step - and needs
// no case of its own. With the whole grid as the range the value IS walk_begin's t_exit, bit for bit.
// Compiled for the kernels and for the host (host/walk_box_sim.cpp, tests/test_walk_box_cpu.py).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_BOX_HD __host__ __device__ __forceinline__
#else
#define RT_BOX_HD inline
#endif

// face i of an axis whose cells start at `lo`: what walk_begin computes for a cell wall (a product, then a sum: two
// roundings - every user is compiled without contraction, and the volatile keeps a host compiler from fusing them)
RT_BOX_HD float walk_box_face(float lo, float cell, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return lo + cell * (float)i;
#else
    const volatile float m = cell * (float)i;
    return lo + m;
#endif
}

struct WalkBox {
    float lox, loy, loz, hix, hiy, hiz;  // faces of the occupied range: walk_box_face(lo, cell, first cell), (.., last cell + 1)
};

// one axis of the clip: the parameter at which the ray leaves the slab [lo, hi] (`inv` = the reciprocal walk_begin made)
RT_BOX_HD float walk_box_axis_exit(float o, float d, float inv, float lo, float hi) {
    const float big = 3.0e38f;
    float a = (lo - o) * inv, b = (hi - o) * inv;
    if (d == 0.f) { const bool outside = o < lo || o > hi; a = outside ? big : -big; b = outside ? -big : big; }
    return __builtin_fmaxf(a, b);
}

RT_BOX_HD float walk_box_exit(float ox, float oy, float oz, float dx, float dy, float dz, float invx, float invy, float invz, const WalkBox& b) {
    float t1 = 3.0e38f;
    t1 = __builtin_fminf(t1, walk_box_axis_exit(ox, dx, invx, b.lox, b.hix));
    t1 = __builtin_fminf(t1, walk_box_axis_exit(oy, dy, invy, b.loy, b.hiy));
    t1 = __builtin_fminf(t1, walk_box_axis_exit(oz, dz, invz, b.loz, b.hiz));
    return __builtin_fmaxf(t1, 0.f);
}

// the walk's stop parameter: the earlier of the two exits plus a quarter of the shortest cell crossing (`t_exit_grid`:
// walk_begin's t_exit; `dmin`: the smallest of its dtx / dty / dtz)
RT_BOX_HD float walk_box_stop(float t_exit_grid, float t_exit_box, float dmin) {
    return __builtin_fminf(__builtin_fminf(t_exit_grid, t_exit_box) + 0.25f * dmin, 3.0e38f);
}
