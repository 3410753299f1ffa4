// rt_query.h - launch interface of the ray queries (rt_query.hip): closest hit and occlusion for rays that are NOT the frame's, on a
// live context's object records and grid (hip_raytracer.h, "ray queries").
#pragma once

#include "rt_device.h"
#include "rt_grid.h"

namespace rt {

// The box a query ray's origin must lie in to be served by the grid: rt_context::grid_box_lo / hi rounded INWARDS to fp32 on the
// host (lo up, hi down), so that the kernel's fp32 comparison never admits an origin the double box excludes. grid = 0: the context
// has no grid, or is literal by RT_FLAG_LITERAL or for a degenerate instance (rt_query_host.cpp: grid_serves_queries): every ray
// takes the ordered loop.
struct QueryBox {
    float lox, loy, loz;
    float hix, hiy, hiz;
    uint32_t grid;
};

// What a query adds up, once per wave (vector atomics): rays, rays per route, exact ray-object tests (2 per pair for a brute-force ray,
// as Counters::tests counts them). Zeroed on the query's stream before the kernel.
struct QueryCounters {
    unsigned long long n_rays, n_grid, n_brute, tests;
};

// Where rt_query_primary's rays come from: the context's pinhole camera (rt_kernels.h: RenderParams' fields of the same names) or its
// ray buffer.
struct QueryCamera {
    const float4* __restrict__ rays;  // null in pinhole mode
    uint32_t pinhole;
    uint32_t width;
    float half_w, half_h, height_f, z;
};

// One thread per ray, 256 per workgroup; any n (a workgroup loops when n exceeds the launch). `arith`: kUnfused / kFused / kDeviceCL.
// d_rays: n x {start, direction}, 16-byte aligned. d_t / d_index: either may be null. n == 0 launches nothing.
hipError_t launch_query_closest(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays,
                                uint64_t n, float* d_t, int32_t* d_index, QueryCounters* d_counters, hipStream_t stream);
hipError_t launch_query_occluded(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays,
                                 uint64_t n, uint8_t* d_occluded, QueryCounters* d_counters, hipStream_t stream);
// ... of the primary rays of the work-items d_items[0 .. n) (each below the camera's / the buffer's ray count: the caller checks)
hipError_t launch_query_primary(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const QueryCamera& camera,
                                const uint64_t* d_items, uint64_t n, float* d_t, int32_t* d_index, QueryCounters* d_counters,
                                hipStream_t stream);

// Hit-record queries (hip_raytracer.h: rt_hits_t with device pointers). Every member may be null, not all of them; point / normal /
// reflected 16-byte aligned (reflected: two float4 per ray, start then direction), t / index 4-byte aligned.
struct QueryHits {
    float* t;
    int32_t* index;
    float4* point;
    float4* normal;
    float4* reflected;
};
// (t, index) as launch_query_closest's, and for the winner what materialise() and reflection_ray() give in mode `arith`; all-zero
// records where index == -1. d_mask: null, or n int32 - a ray whose entry is negative is not traced (nor counted) and reads as a
// miss. out.reflected may be d_rays and out.index may be d_mask: a lane reads element i of both before it writes element i.
hipError_t launch_query_hits(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const float4* d_rays, uint64_t n,
                             const int32_t* d_mask, const QueryHits& out, QueryCounters* d_counters, hipStream_t stream);
hipError_t launch_query_primary_hits(const Scene& scene, const GridDesc& grid, const QueryBox& box, int arith, const QueryCamera& camera,
                                     const uint64_t* d_items, uint64_t n, const QueryHits& out, QueryCounters* d_counters, hipStream_t stream);

// Shaded queries (hip_raytracer.h: rt_shade_t with device pointers; rt_query_shade.hip). Every member may be null, not all of them;
// rgba 16-byte aligned, t / index 4-byte aligned.
struct QueryShade {
    float4* rgba;
    float* t;
    int32_t* index;
};
// What a shaded query adds up, once per wave: QueryCounters for the PRIMARY rays (their route; `tests` counts every ray of the paths),
// the primary rays whose path ran the literal loops, and what Counters holds for a counted frame - primary hits as the context's
// kernel takes them, rays issued, rays the reference semantics trace.
struct QueryShadeCounters {
    QueryCounters q;
    unsigned long long n_literal, hits, traced, reference;
};
// One thread per ray runs the reference's per-pixel program (kernel 1: shade, 2: shade_and_reflect with scene-independent
// `max_bounces`) with a tracer that routes every ray of the path by itself. scene.literal: the context is literal (every path is);
// scene.fast_phong as the frames fill it. Rays: d_rays, or - d_items non-null - the camera's primary rays of those work-items.
// d_mask: null, or n int32 - a negative entry is not traced, not counted and reads as a miss (background, MAX_FLOAT, -1).
hipError_t launch_query_shade(const Scene& scene, const GridDesc& grid, const QueryBox& box, int kernel, int arith, uint32_t max_bounces,
                              const float4* d_rays, const QueryCamera& camera, const uint64_t* d_items, uint64_t n, const int32_t* d_mask,
                              const QueryShade& out, QueryShadeCounters* d_counters, hipStream_t stream);

}  // namespace rt
