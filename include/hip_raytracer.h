/*
 * hip_raytracer.h - C ABI of the MI355X (gfx950) backend for the reference's IRaytracer hot path.
 *
 * This is the drop-in boundary: a `HIPRaytracer : IRaytracer` (C++: opencl-raytracer_amd/host/HIPRaytracer.hpp,
 * Python: opencl-raytracer_amd/hip_raytracer.py) replaces the reference's `OpenCLRaytracer` and calls only
 * these entry points. Plain pointers and sizes; no C++/torch/HIP types in any signature.
 *
 * Reference interfaces replaced (citations into the reference tree):
 *   rt_create          <- OpenCLRaytracer::OpenCLRaytracer(objects, lights, rays, MAX_BOUNCES)
 *                         OpenCLRaytracer.cpp:13-74 (AoS conversion :16-33, buffers :47-50, program build :53-59,
 *                         kernel args :62-68, uploads :70-73)
 *   rt_render          <- OpenCLRaytracer::Render()  OpenCLRaytracer.cpp:80-105 (enqueue_1d_range_kernel :89-91,
 *                         blocking enqueue_read_buffer :94, returns the object-owned host buffer :104);
 *                         declared by IRaytracer::Render()  IRaytracer.hpp:13
 *   rt_render_device   <- the same launch without the read-back (device-resident framebuffer; used for
 *                         multi-GPU gathers and for timing with inputs/outputs resident in HBM)
 *   rt_destroy         <- OpenCLRaytracer::~OpenCLRaytracer()  OpenCLRaytracer.cpp:76-78
 *   rt_set_camera      <- main()'s primary-ray loop  OpenCL-Raytracer.cpp:18-26,68-72 (rays regenerated in-kernel)
 *   kernel selector    <- `__kernel hittest`  hittest_kernel.cl:54, `__kernel shade`  shade_kernel.cl:180,
 *                         `__kernel shade_and_reflect`  shade_and_reflect_kernel.cl:244
 *
 * Record layouts are the reference's device structs, byte for byte (shade_and_reflect_kernel.cl:1-29,
 * OpenCLRaytracer.hpp:25-58): ObjectData 320 B, Light 64 B, Ray 32 B, pixel float4 16 B. See rt_records.h.
 *
 * Error behaviour: the reference has no error codes (Boost.Compute throws). Every function here returns
 * RT_OK (0) or a negative rt_status and records a message retrievable with rt_last_error(); nothing throws
 * across the boundary. There is no CPU fallback: without a usable HIP device rt_create fails with
 * RT_ERR_NO_DEVICE.
 *
 * Threading: like the reference (single in-order queue, OpenCLRaytracer.cpp:44) a context is not
 * re-entrant; use one context per thread / per GPU.
 */
#ifndef HIP_RAYTRACER_H
#define HIP_RAYTRACER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version history:
 *   1  round 1-2.
 *   2  rt_render_device(ctx, out, NULL) means the LEGACY DEFAULT stream (it was the context's private stream in early
 *      builds of version 1); rt_get_setup_times; the multi-device entry points rt_create_multi / rt_render_multi /
 *      rt_render_multi_device / rt_multi_context / rt_destroy_multi. A caller built against version 1 keeps working:
 *      no existing signature or struct changed.
 *   3  rt_get_stats_multi / rt_count_rays_multi (the counters of every shard, summed); rt_render_multi places every device's
 *      tiles straight in the pinned host frame (no hop through devices[0]); rt_create / rt_set_camera switch a frame whose
 *      primary directions leave the default path's domain (|d|^2 == 0, < 1e-30, > 1e30) to RT_FLAG_LITERAL by themselves.
 *      Additions only: a caller built against version 2 keeps working.
 *      Later addition, same version: RT_FLAG_DEVICE_OPENCL (0x80). A library without it refuses the bit with "unknown flag bits",
 *      which is how a caller detects support.
 *      Later addition, same version: 8-bit frames - rt_pixel_format, rt_packed_pixel_bytes, rt_pack_device,
 *      rt_render_device_packed, rt_render_packed, rt_render_multi_packed. Additions only; a caller detects support by the
 *      symbol (dlsym of rt_packed_pixel_bytes).
 *      Later addition, same version: supersampled frames - rt_set_supersampling, rt_supersampling, rt_local_pixels,
 *      rt_resolve_device, rt_set_supersampling_multi, rt_multi_frame_pixels. Additions only; a caller detects support by the
 *      symbol (dlsym of rt_set_supersampling).
 *      Later addition, same version: replaceable rays - rt_set_rays_device, rt_set_rays, rt_get_rays_info. Additions only; a caller
 *      detects support by the symbol (dlsym of rt_set_rays_device).
 *      Later addition, same version: posed cameras - rt_set_pose, rt_generate_rays_device, rt_set_pose_multi; rt_rays_info_t::source
 *      may read 3. Additions only; a caller detects support by the symbol (dlsym of rt_set_pose).
 *      Later addition, same version: replaceable lights - rt_set_lights, rt_set_lights_multi, rt_get_light_tiles_info,
 *      rt_read_light_tiles, rt_read_grid_pretest. Additions only; a caller detects support by the symbol (dlsym of rt_set_lights).
 *      Later addition, same version: replaceable materials - rt_set_materials, rt_set_materials_device, rt_set_materials_multi,
 *      rt_read_materials. Additions only; a caller detects support by the symbol (dlsym of rt_set_materials).
 *      Later addition, same version: replaceable transforms - rt_set_transforms, rt_set_transforms_multi, rt_read_transforms,
 *      rt_get_geometry_info. Additions only; detect by dlsym of rt_set_transforms.
 *      Later addition, same version: poses outside the grid's box keep the grid - RT_TILES_REFUSED_FAR, rt_tiles_info_t::source may
 *      read 3, rt_rays_info_t::reserved became primary_outside_box, rt_read_pose_spheres, rt_read_object_bounds,
 *      rt_get_grid_constants. Additions only; detect by dlsym of rt_read_pose_spheres.
 *      Later addition, same version: replaceable visibility - rt_set_visibility, rt_set_visibility_device, rt_read_visibility,
 *      rt_set_visibility_multi; RT_TYPE_HIDDEN in rt_records.h. Additions only; detect by dlsym of rt_set_visibility.
 *      Later addition, same version: ray queries - rt_query_closest_device, rt_query_occluded_device, rt_query_closest,
 *      rt_query_occluded, rt_query_primary, rt_get_query_info. Additions only; detect by dlsym of rt_query_closest_device.
 *      Later addition, same version: hit-record queries - rt_hits_t, rt_query_hits_device, rt_query_hits, rt_query_primary_hits.
 *      Additions only; detect by dlsym of rt_query_hits_device.
 *      Later addition, same version: compact records - rt_compact_info_t, rt_get_compact_info. Additions only; detect by dlsym of
 *      rt_get_compact_info.
 *      Later addition, same version: G-buffer frames - rt_gbuffer_t, rt_gbuffer_info_t, rt_render_gbuffer_device, rt_render_gbuffer,
 *      rt_get_gbuffer_info. Additions only; detect by dlsym of rt_render_gbuffer_device.
 *      Later addition, same version: the block walk's occupied range - rt_block_range_t, rt_get_block_range. Additions only; detect
 *      by dlsym of rt_get_block_range.
 *      Later addition, same version: ambient-occlusion frames - rt_ao_params_t, rt_ao_t, rt_ao_info_t, rt_ao_device, rt_ao,
 *      rt_render_ao_device, rt_render_ao, rt_get_ao_info. Additions only; detect by dlsym of rt_render_ao_device.
 *      Later addition, same version: filtered ambient occlusion - rt_ao_filter_params_t, rt_ao_filtered_t, rt_ao_filter_info_t,
 *      rt_ao_filter_device, rt_ao_filter, rt_render_ao_filtered_device, rt_render_ao_filtered, rt_get_ao_filter_info. Additions only;
 *      detect by dlsym of rt_ao_filter_device. */
#define RT_ABI_VERSION 3

typedef struct rt_context rt_context;

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_NO_DEVICE = -2,
    RT_ERR_OUT_OF_MEMORY = -3,
    RT_ERR_HIP = -4,
    RT_ERR_STATE = -5
} rt_status;

typedef enum rt_kernel {
    RT_KERNEL_HITTEST = 0,           /* nearest t per ray          (hittest_kernel.cl:54)            */
    RT_KERNEL_SHADE = 1,             /* direct lighting, summed    (shade_kernel.cl:180)             */
    RT_KERNEL_SHADE_AND_REFLECT = 2  /* + iterative reflection     (shade_and_reflect_kernel.cl:244) */
} rt_kernel;

/* rt_create flags */
#define RT_FLAG_UNFUSED   0x1u /* arithmetic of an OpenCL device WITHOUT fma contraction (x86 baseline); default
                                  is the contraction the OpenCL front-end marks (llvm.fmuladd -> fma)          */
#define RT_FLAG_LITERAL   0x2u /* trace every ray the reference traces (no exact eliminations: any-hit shadow
                                  early-out, backward light scan, dead reflection ray). Results are identical.
                                  rt_create sets it by itself for a scene with a DEGENERATE instance (non-finite or
                                  singular mvInverse): its NaN hit times make the reference's result depend on the
                                  order of the object loop, which only the literal loops reproduce - and for a frame
                                  whose PRIMARY rays leave the domain of the exact eliminations: any direction with
                                  |d|^2 == 0, < 1e-30 or > 1e30 (or not finite) in the uploaded buffer, or a pinhole
                                  camera (rt_set_camera) that produces one. The reference's tests give such a ray a
                                  NaN time on EVERY object (shade_and_reflect_kernel.cl:85-108). Domain of the default
                                  (grid) path therefore: finite rays with start.w = 1, direction.w = 0,
                                  1e-30 < |d|^2 < 1e30, affine instances; everything else is rendered by the
                                  brute-force or literal loops, never approximated                               */
#define RT_FLAG_NO_RAYGEN 0x4u /* never replace an uploaded pinhole ray grid by in-kernel generation            */
#define RT_FLAG_WAVEFRONT  0x8u  /* force the large-scene path (separate traversal / shading kernels)          */
#define RT_FLAG_NO_GRID    0x20u /* large-scene path: test every object for every ray (no conservative grid culling);
                                    results are identical, this is the brute-force baseline                  */
#define RT_FLAG_MONOLITHIC 0x10u /* force the small-scene path (one fused kernel per frame); default: chosen by
                                    object count. Both paths produce identical bits.                          */

#define RT_FLAG_FAST_PHONG 0x40u /* opt-in: values that feed COLOUR only (the shading normal, the view vector, the reflected
                                    light vector, the specular power) on the hardware's fast reciprocal-square-root / log2 /
                                    exp2 paths instead of IEEE sqrt + divisions and the library powf. Every ray - hit index, t,
                                    shadow and reflection rays, the reference-equivalent ray count - stays bit-exact; colours
                                    stay within the 1e-5 the reference comparison allows (north_star), not bit-identical to
                                    the default arithmetic.                                                              */

#define RT_FLAG_DEVICE_OPENCL 0x80u /* opt-in: the arithmetic of the reference's kernels as AMD's OpenCL toolchain builds them for gfx950,
                                    instead of the x86 oracle's: `/` as v_frexp + v_rcp_f32 + v_ldexp (2.5 ulp), sqrt as a scaled
                                    v_sqrt_f32, normalize as the OpenCL library's scaled v_rsq_f32 (a zero vector stays zero), dot as an
                                    fma chain, contraction as the default. Someone who renders with the reference's OpenCLRaytracer on
                                    an AMD GPU gets that picture. Refused (RT_ERR_INVALID_ARGUMENT) together with RT_FLAG_UNFUSED or
                                    RT_FLAG_FAST_PHONG, and for scenes with triangles (type 2). A scene with a light inside an object's bounding
                                    sphere, or a directional light of direction 0 or of |d|^2 outside (1e-30, 1e30), is rendered with
                                    RT_FLAG_LITERAL set by rt_create. */

typedef struct rt_stats_t {
    uint64_t rays_traced;     /* rays this backend actually issued in the last counted render (R_act)          */
    uint64_t rays_reference;  /* rays the reference semantics trace for the same frame (R_ref)                 */
    uint64_t hit_pixels;      /* work-items whose primary ray hit something                                    */
    float    last_kernel_ms;  /* device time of the last render's kernel(s), HIP events on the render stream   */
    uint32_t pinhole;         /* 1 if primary rays are generated in-kernel                                     */
    uint32_t width, height;   /* pinhole grid (0 when rays come from the uploaded buffer)                      */
    uint64_t local_rays;      /* work-items this context renders (after rt_set_shard)                          */
    uint32_t wavefront;       /* 1 if the last render used the large-scene (wavefront) path                    */
    uint32_t rounds;          /* trace/resume rounds of the last wavefront render                              */
    uint64_t object_tests;    /* ray-object tests executed by the traversal kernels in the last counted render
                                 (large-scene path only; 0 otherwise)                                           */
} rt_stats_t;

/* Build a raytracer for one GPU.
 *   objs   : n_objs  x 320-byte ObjectData records (may be NULL when n_objs == 0)
 *   lights : n_lights x 64-byte Light records      (may be NULL when n_lights == 0)
 *   rays   : n_rays  x 32-byte Ray records in work-item order, or NULL when rt_set_camera() will
 *            describe an n_rays = width*height pinhole grid
 *   max_bounces : MAX_BOUNCES of shade_and_reflect (ignored by the other kernels, as in the reference)
 *   device : HIP device ordinal
 * Host buffers are copied; the caller may free them after the call returns. */
int rt_create(rt_context** ctx, const void* objs, uint32_t n_objs, const void* lights, uint32_t n_lights,
              const void* rays, uint64_t n_rays, uint32_t max_bounces, int kernel, int device, uint32_t flags);

/* Primary rays = the reference's pinhole grid, generated in-kernel (bit-exact):
 * start (0,0,0,1), direction (i - W/2, (H - j) - H/2, z, 0) for work-item j*W + i. width*height must equal n_rays.
 * Callable any number of times between renders, also on a context that has rendered: the NEXT render uses the new camera, and
 * the frame is the one a context created directly with that camera renders, bit for bit - whatever was rendered before
 * (tests/test_context_lifecycle_gpu.py). A camera replaces the ray buffer in use until the next rt_set_rays_device / rt_set_rays
 * ("replaceable rays", below) puts a buffer in its place: the buffer uploaded at rt_create is not kept behind a camera's back.
 * The ray-domain guard (RT_FLAG_LITERAL, above) follows the camera: one whose grid holds a direction of |d|^2 outside
 * (1e-30, 1e30) - z = 0 with an even width and height, say - renders with the literal loops, and the next camera inside the
 * domain takes the context back to the default path. A scene with triangles REFUSES such a camera
 * (RT_ERR_INVALID_ARGUMENT: the literal loops do not know triangle records) and keeps rendering the previous one. The shard
 * setting (rt_set_shard) survives a camera change unchanged. */
int rt_set_camera(rt_context* ctx, uint32_t width, uint32_t height, float z);

/* Multi-GPU partition: work-items are cut into tiles of `tile_rays` consecutive rays (a row-tile is
 * tile_rows*width rays); tile j belongs to rank j % world. After this call the context renders only its
 * own tiles, packed back to back in its output buffer (rt_local_rays() work-items); the ragged last tile of the frame is
 * padded to a whole tile with background pixels (misses). world == 1 is the whole frame again.
 * Callable any number of times between renders, also after renders with another shard (rt_local_rays() may grow or shrink; the
 * context's buffers grow as needed and never shrink): the next render is the one a fresh context with that shard renders.
 * The partition is expressed in RAYS, not rows: a later rt_set_camera with another width keeps tile_rays, so the tiles need
 * not be whole rows any more (any tile_rays is valid; whole rows in multiples of 8 only render faster). */
int rt_set_shard(rt_context* ctx, uint64_t tile_rays, uint32_t rank, uint32_t world);
uint64_t rt_local_rays(const rt_context* ctx);

/* Synchronous render into a context-owned host buffer, like IRaytracer::Render():
 *   kernels 1,2: rt_local_rays() x float4; RGB in [0..2]; misses are (0,0,0,1) (the reference's upload-time
 *                background, OpenCLRaytracer.cpp:32), hit pixels have w = 1
 *   kernel 0   : rt_local_rays() x float; misses are 3.402823466e+38f
 * The buffer is overwritten by the next call and freed by rt_destroy.
 * A large frame of the large-scene path (>= 4 M rays, not sharded by the caller) is rendered in two passes over interleaved
 * 16-row tiles - three tiles of every four, then the fourth - the first pass's read-back running while the second renders: same
 * pixels, three quarters of the blocking copy (OpenCLRaytracer.cpp:94) hidden. RT_RENDER_PASSES=1 in the environment keeps it
 * to one pass, RT_RENDER_SPLIT="a,b[,c[,d]]" chooses another split (tiles per pass out of every a + b + ..). */
int rt_render(rt_context* ctx, const float** out);

/* Render into caller-provided DEVICE memory (same element layout) on a caller-provided HIP stream (hipStream_t passed
 * as void*). NULL is the LEGACY DEFAULT stream - what a host framework's "current stream" handle is when it is on its
 * default stream (torch: cuda_stream == 0) - so the frame is always ordered with the caller's own work on that stream;
 * it is never a private stream of the context. The small-scene path does not synchronise the host. The large-scene
 * path keeps its round loop on the device (queue lengths never travel to the host inside a round) and synchronises
 * the stream once per batch of rounds - once per frame in the normal case. The calling thread's current device is
 * left as it was. */
int rt_render_device(rt_context* ctx, void* d_out, void* hip_stream);

/* Optional per-work-item primary-hit record of the NEXT render: t (float) and winning object index
 * (int32, -1 on a miss) into caller-provided DEVICE buffers of rt_local_rays() elements (either may be NULL).
 * A miss is what the KERNEL takes for one, as rt_stats_t::hit_pixels counts it: a primary ray whose time is NaN (a direction of
 * 0: the reference's loop ends with the last sphere / box and a NaN time) is a miss for RT_KERNEL_HITTEST and RT_KERNEL_SHADE
 * (index -1; `t < MAX_FLOAT` fails, shade_kernel.cl:167) and a hit of that object for RT_KERNEL_SHADE_AND_REFLECT (`t ==
 * MAX_FLOAT` fails, shade_and_reflect_kernel.cl:173). t is the loop's value in both cases (NaN). */
int rt_set_aux_device(rt_context* ctx, void* d_hit_t, void* d_hit_index);
/* Host-side convenience: render once and copy t / index to host arrays (either may be NULL). */
int rt_render_aux(rt_context* ctx, float* hit_t, int32_t* hit_index);

/* Counted render (untimed instrumentation pass): fills rays_traced / rays_reference / hit_pixels. */
int rt_count_rays(rt_context* ctx);
int rt_get_stats(rt_context* ctx, rt_stats_t* stats);

/* Device-time bookkeeping: every render records a HIP event pair around its kernel(s) on the stream it was
 * launched on (up to 256 launches are kept). rt_timing_summary waits for them and returns the summed device
 * time and the number of launches since rt_timing_reset. */
int rt_timing_reset(rt_context* ctx);
int rt_timing_summary(rt_context* ctx, double* sum_ms, uint32_t* launches);

/* One-time host-side work that sits OUTSIDE every render timer (the reference's equivalent is its constructor,
 * OpenCLRaytracer.cpp:13-74): milliseconds of wall clock spent in rt_create and, for the per-camera screen tiles and the
 * large-scene path's state buffers, in the first render. */
typedef struct rt_setup_times_t {
    double create_ms;        /* rt_create as a whole (incl. the HIP runtime's start-up when rt_create is the process's
                                first HIP call: ~140 ms that belong to no phase below)                          */
    double upload_ms;        /* record re-pack + uploads (objects, lights, rays)                               */
    double grid_ms;          /* conservative grid + the record table of the unified walk (0 for small scenes)  */
    double blocks_ms;        /* the closest-hit walk's coarse grid of 32-byte blocks                           */
    double light_tiles_ms;   /* light tiles of the last positional light                                       */
    double screen_tiles_ms;  /* per-camera screen tiles (first render after rt_create / rt_set_camera)         */
    double buffers_ms;       /* large-scene path: pixel state + queues allocation (first render)               */
} rt_setup_times_t;
int rt_get_setup_times(rt_context* ctx, rt_setup_times_t* times);

/* ---- 8-bit frames ----------------------------------------------------------------------------------------------------------
 * What a picture's consumers take - the reference's PPMExporter::ExportP3 (PPMExporter.cpp:7-30), a window, an encoder - is 8
 * bits per channel. These entry points quantise ON THE DEVICE (one streaming pass over the float4 frame, csrc/rt_pack.hip) and
 * move a quarter (RGBA8) or 3/16 (RGB8) of the float frame's bytes. The float entry points are untouched.
 *
 * The byte a channel value v (fp32) becomes:  p = v * 255.0f (ONE fp32 multiplication), f = floorf(p), then
 *     f is NaN, or f < 0 (-inf included; -0.0f gives 0 anyway)  ->  0
 *     f >= 255 (+inf included)                                  ->  255
 *     otherwise                                                 ->  (uint8_t)f
 * This is the reference's min(255, (int)floorf(v * 255.f)) wherever that expression yields 0..255, i.e. wherever the P3 file
 * it writes is a valid PPM. Outside that range the reference's (int) conversion is undefined behaviour in C (x86 gives
 * INT_MIN for NaN and +inf, a negative number for v < 0): a byte cannot carry that, and the table above is what it gets
 * instead. The fourth byte of an RGBA8 pixel is the same function of w (1 -> 255 for every pixel the kernels write).
 * Pixels are in work-item order, RGB8 tightly packed (3 bytes per pixel, no row padding). */
typedef enum rt_pixel_format { RT_PIXEL_RGBA8 = 1, RT_PIXEL_RGB8 = 2 } rt_pixel_format;
size_t rt_packed_pixel_bytes(int format); /* 4, 3; 0 for an unknown format. Needs no device. */

/* Convert n_pixels float4 pixels that already are in DEVICE memory (any colour frame of this library; d_rgba_f32 16-byte
 * aligned) into n_pixels * rt_packed_pixel_bytes(format) bytes at d_out, asynchronously on hip_stream (NULL = legacy default
 * stream), on any context whatever its kernel. d_out must be 4-BYTE ALIGNED (RT_ERR_INVALID_ARGUMENT otherwise); beyond that
 * any offset is fine and not one byte behind the last pixel is written. Unknown format or a NULL pointer with n_pixels > 0:
 * RT_ERR_INVALID_ARGUMENT. n_pixels == 0: RT_OK, nothing launched. */
int rt_pack_device(rt_context* ctx, const void* d_rgba_f32, uint64_t n_pixels, int format, void* d_out, void* hip_stream);

/* rt_render_device, then the pass, on the same stream: d_out is rt_local_rays() * rt_packed_pixel_bytes(format) bytes of
 * caller DEVICE memory, 4-byte aligned. The float frame lives in a context-owned scratch buffer (allocated by the first
 * call, freed by rt_destroy); calls that share a context must be ordered by the caller, as for every other entry point.
 * Same stream semantics as rt_render_device (NULL = legacy default stream). Shards (rt_set_shard) work unchanged: packed
 * tiles back to back. RT_KERNEL_HITTEST contexts are refused (RT_ERR_STATE: one float per ray is not a colour).
 * Timing: rt_get_stats' last_kernel_ms and rt_timing_summary keep meaning the RENDER's kernels - the pass is launched behind
 * the event pair, not inside it. */
int rt_render_device_packed(rt_context* ctx, int format, void* d_out, void* hip_stream);

/* rt_render's synchronous twin: rt_local_rays() pixels of bytes in a context-owned PINNED host buffer, overwritten by the next
 * packed call and freed by rt_destroy (rt_render's float buffer is a different one and keeps its contents). A large frame goes
 * through rt_render's passes under rt_render's conditions - per pass: render, pack that pass's pixels, strided copy of bytes -
 * with RT_RENDER_PASSES / RT_RENDER_SPLIT read alike; the default split of a byte frame is "7,1" (its copy is a quarter as long,
 * so a smaller last pass leaves less of it behind the kernels). */
int rt_render_packed(rt_context* ctx, int format, const uint8_t** out);

/* ---- supersampled frames -----------------------------------------------------------------------------------------------------
 * Anti-aliasing by a box filter ON THE DEVICE (csrc/rt_resolve.hip): the context renders its SAMPLE grid exactly as without it and
 * delivers one PIXEL per s x s block of samples, so s^2 times fewer bytes cross the bus.
 *
 * Primary directions are not normalised - (i - W/2, (H - j) - H/2, z) - so the pinhole grid (s W, s H, s z) is a regular s x s
 * lattice of sub-pixel rays inside every pixel of the (W, H, z) grid: sample (s i + a, s j + b) has direction
 * s * (i - W/2 + a/s, (H - j) - H/2 - b/s, z). A supersampled W x H frame IS what the reference renders at s W x s H with s z,
 * box-filtered s x s; every sample is a ray every existing path of this library already agrees on with the reference.
 *
 * Definition. A context whose camera is the pinhole grid (w, h, z) and whose factor is s (1, 2, 3 or 4; 1 = off) renders w x h
 * samples and delivers (w/s) x (h/s) pixels. Pixel (i, j) (row-major, j outer), each of the four channels by itself, in fp32
 * with every addition rounded, nothing contracted, ONE multiplication at the end:
 *     acc = sample[(s j + 0) w + s i + 0]
 *     for b in 0..s-1: for a in 0..s-1 (b outer, a inner, the first one skipped):  acc = acc + sample[(s j + b) w + s i + a]
 *     pixel = acc * fl(1.0f / (float)(s s))
 * NaN and infinities propagate as IEEE says. The ORDER is part of the definition (another one changes the bits of some pixels).
 * w is filtered like a colour channel and comes out as exactly 1 for s = 2, 3, 4. The bytes of a supersampled frame are the
 * table of "8-bit frames" applied to that float pixel (filter first, then quantise).
 *
 * The camera keeps describing the SAMPLE grid (width * height == n_rays stays rt_set_camera's rule): work-items, shards,
 * rt_local_rays(), rt_stats_t, rt_count_rays and rt_timing_* keep counting samples, and the filter is launched behind the
 * render's event pair (last_kernel_ms keeps meaning the render's kernels). With s > 1 rt_render, rt_render_device,
 * rt_render_packed, rt_render_device_packed and the rt_render_multi* calls deliver rt_local_pixels() (rt_multi_frame_pixels())
 * elements; the sample frame lives in context-owned device memory (allocated by the first such call, grown never shrunk, freed
 * by rt_destroy; a context that never supersamples allocates nothing for it). Stream semantics are the entry point's.
 *
 * rt_set_supersampling is callable any number of times between renders, like rt_set_camera and rt_set_shard: the next frame
 * depends on the current (camera, shard, factor) only. The three setters validate against each other, and a refused call leaves
 * the context as it was. Refused with RT_ERR_INVALID_ARGUMENT: s outside 1..4; s > 1 without a pinhole camera; width % s or
 * height % s != 0 (also a later rt_set_camera while s > 1); s > 1 with world > 1 and tile_rays % (s width) != 0 - a tile must
 * hold whole pixel rows, then a shard's pixels are tile_rays / s^2 per tile, packed back to back, and the padding of a ragged
 * last tile filters to the background (0,0,0,1) exactly - checked by whichever of the three setters comes last. Refused with
 * RT_ERR_STATE: s > 1 on an RT_KERNEL_HITTEST context (a time is not a colour); s > 1 while aux buffers are set, and
 * rt_set_aux_device (with a buffer) / rt_render_aux while s > 1 (aux is per work-item).
 * A large frame goes through rt_render's passes (render -> filter (-> pack) -> strided copy of PIXELS per pass) over tiles of
 * 16 sample rows (48 for s = 3), RT_RENDER_PASSES / RT_RENDER_SPLIT read as ever; the frame is the one-pass frame bit for bit. */
int      rt_set_supersampling(rt_context* ctx, uint32_t s);
uint32_t rt_supersampling(const rt_context* ctx);   /* 0 for NULL */
uint64_t rt_local_pixels(const rt_context* ctx);    /* rt_local_rays() / s^2: what every render call delivers; 0 for NULL */
/* The pass alone, like rt_pack_device: sample_rows rows of sample_width float4 samples in DEVICE memory (16-byte aligned) ->
 * (sample_width / s) x (sample_rows / s) pixels at d_out, asynchronously on hip_stream (NULL = legacy default stream), on any
 * context. format 0 = float4 pixels (d_out 16-byte aligned), RT_PIXEL_RGBA8 / RT_PIXEL_RGB8 = bytes (d_out 4-byte aligned), filter
 * and quantisation fused. s = 1..4 (1: a copy, or rt_pack_device); sample_width and sample_rows multiples of s; nothing is written
 * behind the last pixel; zero pixels: RT_OK, nothing launched. Anything else: RT_ERR_INVALID_ARGUMENT. */
int      rt_resolve_device(rt_context* ctx, const void* d_samples, uint32_t sample_width, uint32_t sample_rows, uint32_t s,
                           int format, void* d_out, void* hip_stream);

/* ---- replaceable rays ----------------------------------------------------------------------------------------------------------
 * The fourth piece of a live context's state next to camera, shard and factor: its primary rays, replaced from DEVICE memory (rays
 * another kernel or a host framework computed on the GPU: a panned, rolled or moved pinhole, a fisheye) or from host memory. The next
 * frame is the one a context created with those rays and RT_FLAG_NO_RAYGEN renders, bit for bit, whatever was rendered before.
 *
 * rt_set_rays_device: d_rays is n_rays records of 32 bytes (start, direction) in work-item order, 16-byte aligned, on the context's
 * device; n_rays must equal the context's ray count (rt_set_camera's width * height == n_rays: the state buffers are sized by it).
 * The call enqueues a read-only scan of the rays (csrc/rt_rays.hip) on hip_stream (NULL = legacy default stream) - behind the
 * caller's own kernels that produce them - waits for its verdict, and, if the context can render these rays, copies them
 * device-to-device into a buffer of its own (allocated by the first call, also for a context created with rays = NULL) and waits
 * for the copy. It is synchronous like rt_create: when it returns the caller may overwrite or free d_rays, and the next render on
 * any stream sees the new rays. Renders of this context still in flight on ANOTHER stream must be ordered by the caller, as for
 * every other entry point. A refused call leaves the context exactly as it was (the scan runs before the copy).
 * Refused with RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, another n_rays, a supersampling factor > 1 (it needs a pinhole
 * grid; rt_set_supersampling(s > 1) after this call is refused by its own rule), and - for a scene with triangles, which only the
 * grid path traces - rays that would need the literal loops or brute force (below); the context keeps rendering what it rendered.
 * rt_set_rays is the host twin: it stages the array in device memory and takes the same route.
 *
 * The scan computes what rt_create's loops over an uploaded array compute, in fp32, nothing contracted, left to right:
 *   dir_w_zero            every direction.w == 0.0f
 *   directions_in_domain  every dd = (dx*dx + dy*dy) + dz*dz has dd > 1e-30f && dd < 1e30f (a NaN fails)
 *   starts_ok             every start.w == 1.0f and (sx + sy) + sz finite (finite components whose fp32 sum overflows fail)
 *   origin_lo / origin_hi the numeric minimum / maximum of start.x, .y, .z (meaningful only when starts_ok)
 * and the verdict follows the rays in use, frame by frame:
 *   - not directions_in_domain: the literal loops (RT_FLAG_LITERAL, above), until the next rays or camera inside the domain;
 *   - the conservative grid built at rt_create (fine grid, block grid, light tiles) serves the frame only if dir_w_zero, starts_ok
 *     and the origin box lies inside the box the grid's radii were derived for (box_lo / box_hi: the create-time origins united with
 *     the padded object bounds). Otherwise the frame is rendered as RT_FLAG_NO_GRID renders it - same pixels,
 *     every object tested - and the next rays inside the box, or the next camera, bring the grid back. No grid is rebuilt.
 * No pinhole grid is recognised in replaced rays (as with RT_FLAG_NO_RAYGEN): rt_stats_t::pinhole is 0, width and height are 0. A
 * later rt_set_camera takes the context back to in-kernel rays, a later rt_set_rays* back to a buffer. Shards, rt_render's passes,
 * aux buffers, 8-bit frames and rt_count_rays work as for rays uploaded at rt_create. */
typedef struct rt_rays_info_t {
    uint32_t source;                /* 0 none yet (rays = NULL and no camera), 1 in-kernel pinhole grid, 2 the ray buffer,
                                       3 ray buffer generated from a pose (rt_set_pose; every other field reads as for 2)     */
    uint32_t dir_w_zero;            /* the three predicates of the rays in use (a pinhole grid: 1, domain by its camera, 1)   */
    uint32_t directions_in_domain;
    uint32_t starts_ok;
    float    origin_lo[3];          /* box of the origins; (0,0,0) for a pinhole grid and when !starts_ok. For rays uploaded at */
    float    origin_hi[3];          /* rt_create: united with (0,0,0), as the grid's box took them                             */
    double   box_lo[3];             /* the box the grid's radii were derived for (0 when grid_built == 0)                      */
    double   box_hi[3];
    uint32_t grid_built;            /* rt_create built a conservative grid                                                     */
    uint32_t grid_in_use;           /* ... and the next frame's rays are served by it (0 also while `literal`)                 */
    uint32_t literal;               /* the next frame renders with the literal loops                                           */
    uint32_t primary_outside_box;   /* the next frame's primary rays start OUTSIDE box_lo .. box_hi (a pose's) and are served by its screen
                                       tiles while the grid serves every later ray; grid_in_use then reads 1 ("posed cameras")  */
} rt_rays_info_t;
int rt_set_rays_device(rt_context* ctx, const void* d_rays, uint64_t n_rays, void* hip_stream);
int rt_set_rays(rt_context* ctx, const void* rays, uint64_t n_rays);
int rt_get_rays_info(const rt_context* ctx, rt_rays_info_t* info);   /* valid for every context, also one that never called the setters.
                                                                         After a pose outside the grid's box it builds that pose's screen tiles
                                                                         first, as rt_get_tiles_info does: kernels on the context's stream, a
                                                                         wait, possibly RT_ERR_HIP ("posed cameras", outside the box)          */

/* ---- posed cameras -------------------------------------------------------------------------------------------------------------
 * A pinhole that turns or moves: the grid (width, height, z) of rt_set_camera seen through an fp32 3 x 3 matrix M (row-major,
 * m[3 r + c]; any matrix, a rotation is the usual one) from a common origin. The rays are generated ON THE DEVICE (one streaming
 * pass, csrc/rt_raygen.hip: 32 bytes written per ray, nothing read) straight into the context's ray buffer; behind that the
 * context is in the state rt_set_rays_device leaves for the same rays, and renders them as "replaceable rays" says.
 *
 * Definition (opencl-raytracer_amd/rays.py: posed_rays is the executable one). For work-item j * width + i, in fp32, every product
 * and sum rounded, nothing fused, left to right:
 *     x = fl(i) - fl(width / 2);  y = (fl(height) - fl(j)) - fl(height / 2)
 *     direction[r] = (M[r][0] * x + M[r][1] * y) + M[r][2] * z   (r = 0, 1, 2),  direction.w = 0,  start = (origin, 1)
 * With the identity and a zero origin these are rt_set_camera's rays, bit for bit, and the frame is that camera's.
 *
 * rt_set_pose: width * height must equal the context's ray count, width and height are at most 2^24 (rt_set_camera's rules). The
 * call enqueues on hip_stream (NULL = legacy default stream) a verdict pass that stores no ray, waits for it, refuses what the
 * context cannot render, and only then generates into the context's own ray buffer (allocated by the first call, also for a
 * context created with rays = NULL) and waits. No staging buffer, no copy. It is synchronous like rt_set_rays_device, and a refused
 * call leaves the context exactly as it was. The verdict is the one the ray scan gives the same rays: dir_w_zero holds;
 * directions_in_domain is reduced over every direction's dd; starts_ok is isfinite((ox + oy) + oz); the origin box is the point.
 * A non-finite or degenerate M is no error: its directions leave the domain and the frame renders with the literal loops. An
 * origin outside box_lo .. box_hi keeps the grid when the pose's screen tiles are accepted (below: "outside the box"); otherwise it
 * renders by brute force, as for any ray buffer. No grid is rebuilt either way.
 * Refused with RT_ERR_INVALID_ARGUMENT: a NULL m or origin; width * height != n_rays; for a scene with triangles a pose that needs
 * the literal loops or brute force; and, while the supersampling factor is > 1, what rt_set_camera is refused for (below).
 * rt_get_rays_info reports source 3; rt_stats_t::pinhole, width and height stay 0 as for any buffer. The RAYS of a posed frame are
 * read from the buffer, but its primary round is the fixed camera's: the context keeps the pose, and the first large-scene frame
 * after it builds the pose's depth-ordered screen tiles ON THE DEVICE from the objects' registration spheres ("screen tiles"
 * below; csrc/rt_tiles.hip) - 64 x 8 tiles, since a posed frame's work-items are in linear order - and traces the primary rays
 * through them instead of the grid walk. Same pixels, bit for bit. A pose whose table is refused (rt_tiles_info_t::refused) is
 * traced through the grid walk as before; RT_POSE_TILES=0 in the environment keeps every pose there (a measurement knob). A later
 * rt_set_camera or rt_set_rays* replaces the pose, and the other way round. Shards, rt_render's passes, aux buffers, 8-bit frames and rt_count_rays work as for a buffer; a
 * sharded context generates the whole frame's rays.
 *
 * Outside the box. A camera that orbits the scene or pulls back from it leaves box_lo .. box_hi at once. Only its PRIMARY rays start
 * out there - every later ray starts on a surface, inside the box - and the tile lists need no grid: so such a pose gets registration
 * spheres made for its own origin, on the device (csrc/rt_tiles.hip: pose_spheres; tiles.py: pose_registration_spheres - the grid's
 * own expressions with the farthest origin and the largest |origin| taken over the box and the pose's origin), its table is built
 * from them (rt_tiles_info_t::source 3), the primary round walks the lists and never the grid, and the grid, the block grid and the
 * light tiles serve the rest as built. Accepted when the table is not refused and 3e-6 (|o| + far) <= 0.01 cell (far: the largest
 * distance from the origin o to a corner of the box; cell: the fine grid's edge; else RT_TILES_REFUSED_FAR; DESIGN.md section 4.1 has
 * the argument). rt_get_rays_info then reads grid_in_use = 1 and primary_outside_box = 1; both, like rt_get_tiles_info, build the
 * table if the pose is new. (Both may therefore launch kernels on the context's stream, wait for them and return RT_ERR_HIP.) A frame
 * of fewer than 16 tiles (128 x 64 pixels) of a scene of fewer than 512 objects is not served this way (RT_TILES_REFUSED_SMALL): it
 * keeps the route it had before - the small-scene kernel - for callers and tests that rely on it; RT_POSE_OUTSIDE_MIN_TILES=0 in the
 * environment serves such frames too (it is the faster route there as well: DESIGN.md section 6). A refused table of any kind - RT_POSE_TILES=0,
 * width % 64 != 0, GLOBAL, FAR, SMALL, ... - reads RT_TILES_REFUSED_NO_GRID beside its own bit and leaves the frame where it was
 * before this addition: the whole frame as RT_FLAG_NO_GRID renders it. Same pixels, bit for bit, on every route. rt_set_rays*
 * buffers outside the box stay brute force (no common origin, no table), and scenes with triangles keep refusing such poses.
 *
 * Supersampling. The sample grid of a posed camera is defined, so a factor > 1 is open to it: the pose's (width, height, z) is the
 * SAMPLE grid, as rt_set_camera's is (camera.supersampled gives it for a picture's (W, H, z)); the context remembers the pose's
 * width and height, and rt_set_supersampling, rt_set_shard and rt_set_pose validate against each other like the three setters of
 * "supersampled frames" - rt_set_pose counting as the camera setter: width % s, height % s, whole pixel rows per tile.
 * rt_set_rays* keeps refusing a factor > 1. rt_render's passes cut a posed frame into tiles of 16 sample rows (48 for s = 3).
 *
 * rt_generate_rays_device is the pass alone, like rt_pack_device: width * height rays to d_rays (DEVICE memory, 16-byte aligned),
 * asynchronously on hip_stream, on any context, touching no context state. A zero-sized grid: RT_OK, nothing launched. A NULL or
 * misaligned pointer, a NULL m or origin, a width or height above 2^24: RT_ERR_INVALID_ARGUMENT. */
int rt_set_pose(rt_context* ctx, uint32_t width, uint32_t height, float z, const float m[9], const float origin[3], void* hip_stream);
int rt_generate_rays_device(rt_context* ctx, uint32_t width, uint32_t height, float z, const float m[9], const float origin[3],
                            void* d_rays, void* hip_stream);

/* ---- screen tiles ---------------------------------------------------------------------------------------------------------------
 * The first trace round of a large-scene frame walks, per screen tile, a depth-ordered list of the objects a primary ray of that
 * tile can meet (csrc/rt_grid.h: ScreenTiles). The fixed camera's table is built on the host (per rt_set_camera), a posed camera's
 * on the device (per rt_set_pose; opencl-raytracer_amd/tiles.py: pose_screen_tiles is the executable definition). Both are an
 * acceleration only: a frame is the same with and without them.
 * rt_get_tiles_info is valid for every context and reports the table the NEXT large-scene frame would use; it builds the table
 * if the rays changed since the last build (on the context's own stream, synchronously), so a caller need not render first.
 * rt_read_tiles copies that table to host arrays: tile_start[tiles_x * tiles_y + 1] offsets and `entries` as pairs of 32-bit words
 * {object index, depth key (float bits)} - n_entries + n_global of them, a tile's ascending by (key, index), the whole-screen
 * objects behind the last tile's. n_start and n_entries are the arrays' capacities in elements / pairs; too small, or no table:
 * RT_ERR_INVALID_ARGUMENT / RT_ERR_STATE. rt_read_grid_spheres copies the registration spheres the tables are built from: 4
 * doubles per object (centre, radius; inf: tested by every ray, negative: never hit), n = the object count; RT_ERR_STATE for a
 * context without a grid. All three are accessors for tests and tools, as rt_get_rays_info is. */
#define RT_TILES_REFUSED_NO_GRID 0x1u   /* the grid does not serve the rays in use (no grid, literal loops, small-scene path, a buffer's
                                           origins outside its box) or the rays are neither a camera's nor a pose's               */
#define RT_TILES_REFUSED_Z       0x2u   /* z is not < 0                                                                          */
#define RT_TILES_REFUSED_MATRIX  0x4u   /* the pose's matrix or origin is not finite, or the matrix is singular                  */
#define RT_TILES_REFUSED_EPS     0x8u   /* eps >= |z| / 2 or pad > 1: the pose is too ill-conditioned for the table's margins    */
#define RT_TILES_REFUSED_WIDTH   0x10u  /* width is not a multiple of the tile's                                                 */
#define RT_TILES_REFUSED_GLOBAL  0x20u  /* more than 64 objects cover the whole screen                                           */
#define RT_TILES_REFUSED_BUDGET  0x40u  /* more (object, tile) pairs than 256 n_objs + 4096                                      */
#define RT_TILES_REFUSED_LIST    0x80u  /* a tile's list is longer than 1024 entries                                             */
#define RT_TILES_REFUSED_TILES   0x100u /* more than 2^20 tiles                                                                  */
#define RT_TILES_REFUSED_KNOB    0x200u /* RT_POSE_TILES=0                                                                       */
#define RT_TILES_REFUSED_FAR     0x400u /* a pose outside the grid's box whose origin is too far: 3e-6 (|o| + far) > 0.01 cell         */
#define RT_TILES_REFUSED_SMALL   0x800u /* a pose outside the grid's box, fewer than 512 objects and fewer than 16 tiles (128 x 64 pixels) */
typedef struct rt_tiles_info_t {
    uint32_t enabled;               /* the next large-scene frame's primary round walks tile lists                             */
    uint32_t source;                /* 0 none, 1 the fixed camera's (host), 2 the pose's (device), 3 a pose's outside the grid's box
                                       (device, from spheres made for its origin: rt_read_pose_spheres)                        */
    uint32_t tiles_x, tiles_y;      /* tiles are 8 rows tall ...                                                               */
    uint32_t col_shift;             /* ... and 1 << col_shift pixels wide (3 or 6; a pose's: 6)                                */
    uint32_t n_global;              /* whole-screen objects, tested by every wave                                              */
    uint32_t max_list;              /* longest tile list                                                                       */
    uint32_t refused;               /* RT_TILES_REFUSED_* of the last build (0 when enabled; a camera's table reports NO_GRID,
                                       Z, WIDTH, or BUDGET for its pair and whole-screen limits together)                       */
    uint64_t n_entries;             /* (object, tile) pairs of the table (also of a pose's refused for GLOBAL or LIST)         */
    double   build_device_ms;       /* device time of the last build's passes (a pose's; 0 for the host's)                     */
    double   eps, pad;              /* a pose's: the bound on |v' - v| and the rectangle's pad in direction units (rt_grid.h)  */
} rt_tiles_info_t;
int rt_get_tiles_info(const rt_context* ctx, rt_tiles_info_t* info);
int rt_read_tiles(rt_context* ctx, uint32_t* tile_start, uint64_t n_start, uint32_t* entries, uint64_t n_entries);
int rt_read_grid_spheres(const rt_context* ctx, double* spheres, uint64_t n);
/* Accessors for tests and tools, next to rt_read_grid_spheres. rt_read_pose_spheres copies the per-pose registration spheres the
 * current table was built from (4 doubles per object, as above; a sphere above a quarter of the box's diagonal is a whole-screen
 * entry); RT_ERR_STATE when the current table was not built from such spheres (source != 3). rt_read_object_bounds copies what they
 * are made from: 6 doubles per object - centre, radius, kappa^2 (squared condition number), type - kept from rt_create and replaced by
 * rt_set_transforms; RT_ERR_STATE for a context without a grid or with triangles. rt_get_grid_constants: the fine grid's cell edge,
 * the diagonal of box_lo .. box_hi, the largest |origin| that box allows, and the pre-test's K^2; RT_ERR_STATE without a grid. */
int rt_read_pose_spheres(rt_context* ctx, double* spheres, uint64_t n);
int rt_read_object_bounds(const rt_context* ctx, double* bounds, uint64_t n);
int rt_get_grid_constants(const rt_context* ctx, double constants[4]);

/* ---- replaceable lights --------------------------------------------------------------------------------------------------------
 * The last input of a frame that was frozen at rt_create: the lights. rt_set_lights replaces them on a live context - a viewer that
 * drags a light, an animation that changes one per frame - without rt_destroy + rt_create.
 *
 * rt_set_lights: `lights` are n_lights HOST records in the layout rt_create takes. The count may differ from the creation's; 0 is
 * allowed. Refused with RT_ERR_INVALID_ARGUMENT: n_lights >= 1 << 22 (rt_create's limit), n_lights != 0 with lights == NULL. A
 * refused call leaves the context exactly as it was: lights, tables and flags. The call is synchronous like rt_set_pose: on return
 * the array may be reused and the next render on any stream sees the new lights. Renders of this context still in flight on ANOTHER
 * stream must be ordered by the caller (wait for them first), as for rt_set_pose and every other entry point: the call rewrites
 * the light array and the light tiles those frames read.
 *
 * Contract. The next render is the frame a FRESH context renders that is created with the same objects and flags, the current rays /
 * camera / pose / shard / supersampling factor, and these lights - bit for bit, with the same rays_reference and hit_pixels - for
 * every kernel (hittest, shade, shade_and_reflect) and every path (small-scene kernel, round machine, literal loops, brute force,
 * RT_FLAG_NO_GRID). What was set or rendered before does not matter.
 *
 * RT_FLAG_DEVICE_OPENCL: rt_create's predicate on the lights - a positional light on (within the padded bound of) an object, or a
 * directional light whose direction is outside the walks' domain - is evaluated again for the new lights against the objects' bounds
 * kept from creation; the frame goes literal, or stops being literal, as a fresh context's would. rt_get_rays_info().literal
 * reports the result. (A literal frame forced by a degenerate instance, by RT_FLAG_LITERAL or by the rays in use is independent.)
 *
 * Light tiles. The shadow rays towards the LAST light are served by per-direction candidate lists (csrc/rt_grid.h: LightTiles).
 * rt_create builds them on the host; rt_set_lights rebuilds them ON THE DEVICE from the objects' registration spheres
 * (csrc/rt_light_tiles.hip; opencl-raytracer_amd/light_tiles.py is the executable definition), in the block form only. They are a
 * culling structure - every candidate still goes through the pre-test and the exact test - so pixels do not depend on which side
 * built them, or on whether they were built at all: a refused table (bits below) leaves the last light's shadow rays to the grid
 * walk, same bits. RT_LIGHT_TILES_DEVICE=0 in the environment makes rt_set_lights build nothing (a measurement knob, as
 * RT_POSE_TILES=0 is for poses); RT_NO_LIGHT_TILES and RT_NO_LT_BLOCKS keep their meaning. A context that never calls
 * rt_set_lights renders through exactly the tables rt_create built (source 1).
 *
 * rt_get_light_tiles_info reports the table the next frame's shadow rays will use (valid for every context). rt_read_light_tiles
 * copies the block table and its ids back and walks the chains on the host - what is read out is what the kernels read:
 * tile_start[tiles_u * tiles_v + 1] offsets and, per entry in list order, three 32-bit words {object index, block word lo, block
 * word hi} (lo = x16 | y16 << 16, hi = z16 | r8 << 16 | k8 << 24). n_start and n_entries are the arrays' capacities in elements /
 * triples; too small: RT_ERR_INVALID_ARGUMENT. RT_ERR_STATE when no table, or only the record form (RT_NO_LT_BLOCKS), is in use. */
#define RT_LTILES_REFUSED_NO_GRID 0x1u   /* no grid built, literal loops, kernel not shade_and_reflect, no lights, or an object
                                            without a finite registration radius (it is in no list)                               */
#define RT_LTILES_REFUSED_LIGHT   0x2u   /* the last light is directional or not finite                                           */
#define RT_LTILES_REFUSED_PLANE   0x4u   /* no axis-aligned plane through the light with every object 0.05 in front of it         */
#define RT_LTILES_REFUSED_TANGENT 0x8u   /* an object without a usable tangent (beyond 1.5533 rad of the axis)                     */
#define RT_LTILES_REFUSED_BOUNDS  0x10u  /* the rectangles' bounds are empty or not finite                                        */
#define RT_LTILES_REFUSED_BUDGET  0x20u  /* more than 64 n_objs + 4096 (object, tile) pairs, or 32-bit byte offsets exceeded       */
#define RT_LTILES_REFUSED_LIST    0x40u  /* a tile's list is longer than 1024 entries (device builder)                            */
#define RT_LTILES_REFUSED_BLOCKS  0x80u  /* block form impossible: lattice or steps not finite, 2^24 blocks, RT_NO_LT_BLOCKS       */
#define RT_LTILES_REFUSED_KNOB    0x100u /* RT_NO_LIGHT_TILES, or RT_LIGHT_TILES_DEVICE=0 for a device build                       */
typedef struct rt_light_tiles_info_t {
    uint32_t enabled;               /* the next large-scene frame's shadow rays to `light` look up tile lists                  */
    uint32_t source;                /* 0 none, 1 built by rt_create on the host, 2 built by rt_set_lights on the device        */
    uint32_t light;                 /* index of the light the table serves (the last one)                                      */
    uint32_t axis;                  /* projection axis 0 / 1 / 2: every object lies on the `sign` side of the light along it   */
    int32_t  sign;                  /* +1 or -1                                                                                */
    uint32_t tiles_u, tiles_v;
    uint32_t n_blocks;              /* 32-byte blocks of the table: a head per tile + the chains (0: record form)              */
    uint32_t max_list;              /* longest tile list                                                                       */
    uint32_t refused;               /* RT_LTILES_REFUSED_* of the last build (0 when enabled)                                  */
    uint64_t n_entries;             /* (object, tile) pairs                                                                    */
    double   build_device_ms;       /* device time of the last build's passes (events; 0 for the host's)                       */
    double   k_pad;                 /* the pad kPad every registration sphere gets                                             */
    double   cut_pad;               /* absolute slack of the kernels' distance cut                                             */
    double   box_diagonal;          /* the grid box's diagonal D used for the radius rounding                                  */
    float    u0, v0, inv_du, inv_dv;/* tile (iu, iv) covers u0 + iu / inv_du ...                                               */
    float    lat_lo[3], lat_step;   /* the 16-bit lattice of the centres: lat_lo + q lat_step                                  */
    float    rstep, kstep;          /* the 8-bit steps of the radius (rounded up) and the key (rounded down)                   */
    float    pretest_alpha;         /* the grid's pre-test distance term, part of the radius rounding                          */
    uint32_t reserved;
} rt_light_tiles_info_t;
int rt_set_lights(rt_context* ctx, const void* lights, uint32_t n_lights);
int rt_get_light_tiles_info(const rt_context* ctx, rt_light_tiles_info_t* info);
int rt_read_light_tiles(rt_context* ctx, uint32_t* tile_start, uint64_t n_start, uint32_t* entries, uint64_t n_entries);
/* The pre-test radii the block form's radii are rounded from, one float per object as the grid's entry spheres carry them (the
 * sign is a flag of the kernels' pre-test; the radius is the magnitude): an accessor for tests, next to rt_read_grid_spheres. */
int rt_read_grid_pretest(const rt_context* ctx, float* pre, uint64_t n);

/* ---- replaceable materials -----------------------------------------------------------------------------------------------------
 * The colours of a live context's objects: a viewer that highlights the object under the mouse (rt_render_aux names it), a
 * simulation that colours its particles by a scalar every step - without rt_destroy + rt_create. (The two matrices have a setter of
 * their own, "replaceable transforms" below, and an object can be hidden, "replaceable visibility"; sphere <-> box and the object
 * count are NOT replaceable.)
 *
 * `materials` are `count` records of 64 bytes in rt_material's layout (rt_records.h), assigned to objects first .. first + count - 1.
 *
 * Contract. The next render is the frame a FRESH context renders that is created with the same object array except that those
 * objects carry these materials (mv, mvInverse and type untouched), the same flags, and the current rays / camera / pose / shard /
 * supersampling factor / lights - bit for bit, with the same rays_reference and hit_pixels - for every kernel (on an
 * RT_KERNEL_HITTEST context the call is accepted and changes nothing visible), every path (small-scene kernel, round machine, literal
 * loops, brute force, RT_FLAG_NO_GRID, triangles) and every arithmetic mode (default, RT_FLAG_UNFUSED, RT_FLAG_FAST_PHONG,
 * RT_FLAG_DEVICE_OPENCL). What was set or rendered before does not matter. No table is rebuilt and no predicate re-evaluated -
 * none depends on a material: rt_get_rays_info, rt_get_tiles_info and rt_get_light_tiles_info read exactly as before the call.
 * Of a material the kernels read eleven floats (ambient, diffuse and specular rgb, absorption, shininess); reflection,
 * transparency and the three pad words are accepted and ignored. NaN and infinite values are no error: they propagate exactly as
 * in a fresh context.
 *
 * rt_set_materials: a HOST array of any alignment. It is staged in a context-owned device buffer (grow-only, allocated by the first
 * call, freed by rt_destroy) and patched into the object records by the same kernel as the device form (csrc/rt_materials.hip).
 * rt_set_materials_device: `d_materials` is device memory on the context's device, 16-byte aligned; the patch kernel is enqueued
 * on `hip_stream` (NULL: the legacy default stream), behind the caller's kernels that produced the array.
 * Both are synchronous like rt_set_lights: on return the array is the caller's again and the next render on any stream sees the
 * materials. Renders of this context still in flight on ANOTHER stream must be ordered by the caller, as for every setter.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT: first + count > n_objs (computed in 64 bits), a NULL array with count != 0, a misaligned
 * device pointer. A refused call has touched nothing. count == 0 returns RT_OK and launches nothing.
 *
 * rt_read_materials: an accessor for tests and tools, next to rt_read_light_tiles. Copies the device records of objects first ..
 * first + count - 1 back and reassembles rt_material records from what the kernels read: the eleven live floats, the five other
 * words 0. The absorption is kept twice on the device (the shading records and the round machine's object records): the shading
 * records' is returned, and RT_ERR_STATE with a message if the other copy holds other bits. Same refusals as above. */
int rt_set_materials(rt_context* ctx, const void* materials, uint32_t first, uint32_t count);
int rt_set_materials_device(rt_context* ctx, const void* d_materials, uint32_t first, uint32_t count, void* hip_stream);
int rt_read_materials(rt_context* ctx, void* materials, uint32_t first, uint32_t count);

/* ---- replaceable transforms ----------------------------------------------------------------------------------------------------
 * Where a live context's objects are: a viewer that drags the object under the mouse (rt_render_aux names it), an animation that
 * moves a few bodies per frame - without rt_destroy + rt_create, which costs several frames' time for a large scene.
 *
 * `transforms` are `count` HOST records of 128 bytes in rt_transform's layout (rt_records.h: mv, then mvInverse, column-major like
 * rt_object_data's), of any alignment, assigned to objects first .. first + count - 1. The caller supplies both matrices, as it
 * does to rt_create; mvInverseTranspose is read by no kernel and is no part of the record.
 *
 * Contract. The next render is the frame a FRESH context renders that is created with the same object array except that those
 * objects carry these two matrices (materials and type untouched), the same flags, and the current rays / camera / pose / shard /
 * supersampling factor / lights / materials - bit for bit, with the same rays_reference and hit_pixels - for every kernel, every
 * path (small-scene kernel, round machine, literal loops, brute force, RT_FLAG_NO_GRID) and every arithmetic mode. What was set or
 * rendered before does not matter. The call is synchronous like rt_set_lights: on return the array is the caller's again and the
 * next render on any stream sees the objects where they now are; renders of this context still in flight on ANOTHER stream must be
 * ordered by the caller. count == 0 returns RT_OK and launches nothing.
 *
 * The records. One pass on the device (csrc/rt_transforms.hip) rewrites every copy of the two matrices the kernels read - the
 * walks' records, the shading records, the round machine's records and the object's half of its pair in both pair streams - from
 * the array, staged in a context-owned device buffer (grow-only, freed by rt_destroy). Values are moved, not computed with.
 *
 * Contexts with a grid (rt_get_rays_info().grid_built): the DYNAMIC set. The grid, the block grid and the current screen tiles list
 * an object by where it was at rt_create, and rebuilding them on the device is not part of this call. Instead every object an
 * accepted call names becomes dynamic and stays so until rt_destroy: it is appended to the list of "objects every ray must test"
 * that the kernels loop over before they look at any table (the list rt_create uses for objects without a usable bound), and its old
 * registrations stay where they are. That is sound because a table entry is only ever a CANDIDATE: a stale one can do no more than
 * trigger one more exact test of an object the always-loop tests anyway, taking the closer of two hits is order-free and idempotent,
 * and an any-hit answer does not depend on who asks - so pixels are those of a fresh context. The screen tiles' depth-order exit
 * stays valid too: a stale entry keeps its place in the order, which still bounds every entry behind it. The list holds 64 entries,
 * create-time ones included (rt_get_geometry_info: dynamic_capacity). A dynamic object gets registration spheres from the formula
 * the grid was built with, evaluated for the box, cell and scene constant of THAT grid; they are what later screen tiles (a camera
 * or pose change) and light tiles are built from, so those list the object where it is. The light tiles are the one table whose
 * lists are all a ray consults: they ARE rebuilt by the call, on the device, as rt_set_lights does it
 * (rt_get_light_tiles_info: source 2). The price is the always-loop: every ray tests every dynamic object (rt_get_stats:
 * object_tests), and the rays of a frame's tail walk the fine grid instead of the block grid while the list is not empty.
 * Contexts without a grid (at most 95 objects, RT_FLAG_NO_GRID, non-affine instances, literal contexts): no cap, no dynamic set;
 * the records are patched and the small-scene kernel's culling rectangles follow.
 * RT_FLAG_DEVICE_OPENCL: the predicate on the lights ("replaceable lights") is evaluated again with the objects' new bounds; the
 * frame goes literal or stops being literal as a fresh context's would.
 *
 * Refusals are decided on the host, over the WHOLE range, before anything is touched; a refused call leaves the context exactly as
 * it was. RT_ERR_INVALID_ARGUMENT: a NULL array with count != 0; first + count > n_objs (in 64 bits); an object in the range whose
 * type is not 0 or 1 (a triangle's mv holds vertices); on a context whose instances are all affine, a matrix whose bottom row is
 * not (0,0,0,1) exactly; on a context that is not already literal for a degenerate instance, a transform without a finite bound
 * (singular or non-finite mvInverse); on a grid context, a new bound whose centre +- 1.01 R leaves box_lo .. box_hi of
 * rt_get_rays_info on any axis (the grid's margins are derived for ray origins inside that box, and secondary rays start on object
 * surfaces). RT_ERR_STATE: the dynamic set would exceed its capacity. A fresh context would render each of these by the literal
 * loops, by brute force or with a bigger grid; this call never switches paths behind the caller's back.
 *
 * NOT part of this call (each would be its own addition): a device-memory form (the bounds and refusals are evaluated on the host);
 * changing an object between sphere and box, or the object count; triangles; folding dynamic objects back into the grid, hence moving more than 64
 * objects of a grid context - that is the device rebuild of the fine grid and the block grid; poses outside the grid box.
 *
 * rt_read_transforms: an accessor for tests and tools, next to rt_read_materials. Reassembles rt_transform records of objects
 * first .. first + count - 1 from the device records; RT_ERR_STATE with a message if two copies of a word disagree (HotObject /
 * ObjectRecord / either pair stream for rows x, y, z of mvInverse; ColdObject / ObjectRecord for rows x, y, z of mv).
 * rt_get_geometry_info: the dynamic set and what the last accepted rt_set_transforms did. */
typedef struct rt_geometry_info_t {
    uint32_t grid_built;            /* as rt_rays_info_t::grid_built: the context has a grid, moved objects become dynamic         */
    uint32_t n_unbounded;           /* entries rt_create put on the always-list (objects without a usable bound)                  */
    uint32_t n_dynamic;             /* objects rt_set_transforms has put there since                                              */
    uint32_t dynamic_capacity;      /* how many it may put there in all: 64 - n_unbounded (0 without a grid: no dynamic set)      */
    uint32_t dynamic_ids[64];       /* the first n_dynamic: object indices in the order they became dynamic                       */
    uint32_t light_tiles_rebuilt;   /* the last accepted call ran the light tiles' device builder (rt_get_light_tiles_info)       */
    uint32_t reserved;
    double   patch_device_ms;       /* device time of the last accepted call's upload + patch pass (events)                       */
} rt_geometry_info_t;
int rt_set_transforms(rt_context* ctx, const void* transforms, uint32_t first, uint32_t count);
int rt_read_transforms(rt_context* ctx, void* transforms, uint32_t first, uint32_t count);
int rt_get_geometry_info(const rt_context* ctx, rt_geometry_info_t* info);

/* ---- compact records ---------------------------------------------------------------------------------------------------------------
 * A scene whose spheres and boxes are all scale-and-translate instances - the upper 3x3 of mv and of mvInverse hold +0.0f, the bit
 * pattern, in every off-diagonal place; bottom rows (0,0,0,1); no triangles - is `diagonal`. A context without triangles keeps a
 * 64-byte record per object with the diagonals, the translations, the type and the absorption, and the round machine's shading
 * kernels (wf_resume, wf_finish) read it instead of the full records while the scene is diagonal: the same arithmetic on rows rebuilt
 * with literal zeros, so the same frame, bit for bit, from fewer scattered loads. rt_set_transforms may switch the predicate either
 * way; rt_set_materials and rt_set_visibility keep the record's copies true. The walks, literal frames, the small-scene kernel, brute
 * force and the queries read the full records. The environment variable RT_COMPACT_RECORDS=0, read by rt_create: no frame of the
 * context reads the compact records (tests, A/B runs). */
typedef struct rt_compact_info_t {
    uint32_t table_built;      /* the context keeps compact records (it has no triangles)                                        */
    uint32_t n_not_diagonal;   /* spheres / boxes whose matrices are not diagonal (rt_create, then every rt_set_transforms)       */
    uint32_t allowed;          /* RT_COMPACT_RECORDS was not "0" at rt_create                                                     */
    uint32_t in_use;           /* the NEXT frame through the round machine reads them: the scene is diagonal and affine, the      */
                               /* frame is not a literal one                                                                      */
} rt_compact_info_t;
int rt_get_compact_info(const rt_context* ctx, rt_compact_info_t* info);

/* ---- the block walk's occupied range -------------------------------------------------------------------------------------------
 * Closest-hit rays of a grid-able context walk a coarse grid of blocks over the grid's box - the objects' box united with the ray
 * origins known to rt_create. A walk ends where its ray leaves the axis-aligned range of cells that hold an object, not where it
 * leaves the box: no cell beyond that range can hold a hit. The range is taken at rt_create and holds for the context's life
 * (moved objects are tested by every ray, hidden ones keep their cells). The environment variable RT_BLOCK_BOX_STOP=0, read by
 * rt_create: the whole grid is the range - the same kernels, walks that end at the box (tests, A/B runs). */
typedef struct rt_block_range_t {
    uint32_t built;        /* the context has a block grid (else every other field is 0)                                          */
    uint32_t whole_grid;   /* the range is the whole grid: RT_BLOCK_BOX_STOP=0, no occupied cell, or objects out to every face    */
    int32_t cells[3];      /* cells of the grid proper along x, y, z                                                              */
    int32_t lo[3], hi[3];  /* lowest and highest occupied cell along x, y, z (0 <= lo <= hi < cells)                              */
    float cell;            /* cell edge                                                                                           */
    float face_lo[3], face_hi[3];  /* the range's faces in view space, as the walks compute a cell wall: origin + cell * index    */
} rt_block_range_t;
int rt_get_block_range(const rt_context* ctx, rt_block_range_t* range);

/* ---- replaceable visibility ----------------------------------------------------------------------------------------------------
 * Which of a live context's objects are in the picture: a viewer that deletes the object under the mouse, switches a layer off or
 * looks behind a wall, a simulation whose particles die and are born - without rt_destroy + rt_create.
 *
 * The hidden word. The reference's `raycast` switch has no default: an object whose type is none of 0, 1 (and 2, this backend's
 * triangle) is never hit. RT_TYPE_HIDDEN (rt_records.h) is one such word, and not the pair streams' pad 0xffffffff. A hidden object
 * is an object whose type word is RT_TYPE_HIDDEN in every record copy the kernels read.
 *
 * `visible` are `count` bytes for objects first .. first + count - 1: 0 hides the object, anything else gives it the type word
 * rt_create was given. An object created with a type other than 0, 1, 2 can never be hit anyway: it is left alone and reads back
 * as visible.
 *
 * Contract. The next render is the frame a FRESH context renders that is created with the same object array except that the hidden
 * objects carry type = RT_TYPE_HIDDEN (records.with_visibility is the executable definition), the same flags, and the current rays /
 * camera / pose / shard / supersampling factor / lights / materials / transforms - bit for bit, with the same rays_reference and
 * hit_pixels - for every kernel (RT_KERNEL_HITTEST included: its times change), every path (small-scene kernel, round machine,
 * literal loops, brute force, RT_FLAG_NO_GRID, triangles) and every arithmetic mode. What was set or rendered before does not
 * matter: hide, then show, is the untouched context again. Object indices are stable: rt_render_aux keeps naming the same objects
 * and never names a hidden one.
 * rays_traced and object_tests are NOT part of the contract: no table is rebuilt, so a hidden object keeps its registrations in the
 * grid, the block grid, the screen tiles and the light tiles (and its place on the always-list if it is dynamic), and each can still
 * cost an exact test - which a never-hit type fails - but never a pixel: a table entry is only a candidate ("replaceable
 * transforms"). rt_get_tiles_info, rt_get_light_tiles_info and rt_get_geometry_info read exactly as before the call. A frame that
 * hides much of a scene is therefore slower than the fresh context's (README has the measured ratio).
 *
 * What follows the types, on the host, from a mirror of the mask: the NaN-ray winner (rt_set_aux_device: "the last sphere / box")
 * is the last VISIBLE sphere or box; under RT_FLAG_DEVICE_OPENCL the predicate on the lights ("replaceable lights") skips hidden
 * objects - a fresh context gives them no bound - here and in every later rt_set_lights / rt_set_transforms, so
 * rt_get_rays_info().literal goes 0 or 1 as a fresh context's would. One exception, pixels unaffected: a context that rt_create made
 * literal for a degenerate instance (singular or non-finite mvInverse) STAYS literal when that instance is hidden; `literal` reads 1
 * where the fresh context's reads 0.
 * rt_set_materials and rt_set_transforms go by the create-time type and keep working on hidden objects exactly as on visible ones
 * (a moved hidden object becomes dynamic like any other); what they set is what shows when the object is shown again.
 *
 * rt_set_visibility: a HOST mask. It is staged in a context-owned device buffer (grow-only, freed by rt_destroy) and patched into
 * the records by the same kernel as the device form (csrc/rt_visibility.hip: one pass, five 4-byte stores per object).
 * rt_set_visibility_device: `d_visible` is device memory on the context's device, at ANY alignment (a torch bool or uint8 tensor
 * qualifies); the kernel is enqueued on `hip_stream` (NULL: the legacy default stream) behind the caller's kernels that produced
 * the mask, and the range is then copied back into the host mirror for the predicates above.
 * Both are synchronous like rt_set_materials: on return the mask is the caller's again and the next render on any stream sees it.
 * Renders of this context still in flight on ANOTHER stream must be ordered by the caller, as for every setter.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT, before anything is touched: first + count > n_objs (computed in 64 bits), a NULL mask with
 * count != 0. count == 0 returns RT_OK and launches nothing.
 *
 * NOT part of this call (each would be its own addition): sphere <-> box (the bounds change: that is the dynamic set's business);
 * changing the object count; dropping hidden objects from the tables (the device rebuild of the grids); un-literalising a context
 * whose degenerate instance is hidden; a scene_tool option.
 *
 * rt_read_visibility: an accessor for tests and tools, next to rt_read_transforms. Reads the type word of objects first .. first +
 * count - 1 from EVERY device copy (walk records, round-machine records, shading records, both pair streams) and writes 1 or 0 per
 * object; RT_ERR_STATE with a message if two copies disagree or a word is neither the create-time type nor RT_TYPE_HIDDEN. */
int rt_set_visibility(rt_context* ctx, const uint8_t* visible, uint32_t first, uint32_t count);
int rt_set_visibility_device(rt_context* ctx, const void* d_visible, uint32_t first, uint32_t count, void* hip_stream);
int rt_read_visibility(rt_context* ctx, uint8_t* visible, uint32_t first, uint32_t count);

/* ---- ray queries ----------------------------------------------------------------------------------------------------------------
 * Closest hit and occlusion for a few rays of the caller's own, on a live context: the object under the mouse, line of sight between
 * particles, collision and depth probes - without a frame (rt_render_aux traces every ray of the frame for one answer) and without a
 * second RT_KERNEL_HITTEST context (a second grid, a second copy of the records, which sees none of this context's rt_set_transforms /
 * rt_set_visibility). "intersect" / "occluded" of every library of this kind.
 *
 * `rays` are n 32-byte rt_ray records; n is ANY count, independent of the context's ray count. A query reads the context's object
 * records and grid as the setters have left them and writes only the caller's outputs and a context-owned counter block. The frame's
 * rays, camera, pose, shard, supersampling factor, aux buffers and state buffers are untouched: a render before and after a query is
 * the same frame. It works on a context of any rt_kernel; max_bounces, lights and materials do not enter.
 *
 * Closest hit. (t[i], index[i]) is what rt_render_aux returns for work-item i of a FRESH RT_KERNEL_HITTEST context created with the
 * context's current objects (the create-time array through records.with_transforms / with_visibility as set so far), the same
 * arithmetic flags (RT_FLAG_UNFUSED, RT_FLAG_DEVICE_OPENCL), these rays and RT_FLAG_NO_RAYGEN - bit for bit. t is the loop's value:
 * 3.402823466e+38f on a miss, NaN where the loop ends with NaN; index follows the hittest rule of rt_set_aux_device: the winner where
 * t < MAX_FLOAT, else -1. Either output may be NULL, not both.
 * Occlusion. occluded[i] = !(T >= 1.f || T < 0) ? 1 : 0 with T that closest-hit time: the reference's shadow predicate
 * (shade_and_reflect_kernel.cl:229) - something lies on the segment start .. start + direction. A NaN T reads occluded.
 *
 * Route, decided in the kernel by each lane for its own ray (csrc/rt_query.hip; rays.query_route is the executable definition). The
 * grid serves a ray iff the context has a grid (rt_rays_info_t::grid_built) and is not literal by its objects or by the caller - it
 * was not created with RT_FLAG_LITERAL and holds no degenerate instance (a singular or non-finite mvInverse, for which rt_create
 * renders literally: NaN times for finite rays make the result depend on the order of the loop) -, every component of the ray is finite, start.w == 1.0f,
 * direction.w == 0.0f, dd = (dx*dx + dy*dy) + dz*dz lies in (1e-30, 1e30), and the origin lies inside box_lo .. box_hi of
 * rt_get_rays_info - compared in fp32 against the box rounded INWARDS (lo up, hi down), so that a ray the double box excludes is never
 * admitted. Every other ray runs the ordered brute-force loop over all objects: the reference's loop in the reference's order, NaN and
 * zero-direction rays included (no closed form is consulted). Such a ray costs n_objs tests in one lane and keeps its wave until it is
 * done (the brute-force lanes of a wave share one pass): the price of never refusing a ray and never approximating one. The
 * frame-level predicates - directions_in_domain, `literal`, a pose outside the box - play no part: a query's domain is per ray.
 *
 * rt_query_closest_device / rt_query_occluded_device: d_rays and the outputs are device memory on the context's device, d_rays
 * 16-BYTE ALIGNED, d_t / d_index 4-byte aligned. ASYNCHRONOUS on hip_stream (NULL: the legacy default stream), behind the caller's
 * kernels that made the rays: no host synchronisation, and no allocation after the first call - a one-ray pick costs a launch. The
 * rays and outputs must stay valid until the stream has passed the query. Queries, setters and renders of one context on different
 * streams are ordered by the caller, as for every entry point (the setters themselves are synchronous as ever).
 * rt_query_closest / rt_query_occluded: the host twins, synchronous; rays and results are staged in the context's grow-only patch
 * buffer ("replaceable visibility") on the context's stream.
 * rt_query_primary: the viewer's pick. Traces the context's OWN primary rays of the given frame work-items j * width + i (regardless
 * of shard; each below the context's ray count) and returns host results synchronously: with the in-kernel pinhole camera the ray is
 * generated as rt_set_camera defines it, with a pose or a ray buffer it is read from the context's ray buffer. The result is
 * rt_render_aux's for that work-item on an unsharded RT_KERNEL_HITTEST context. A primary ray of a pose OUTSIDE the box takes the
 * brute-force route like any ray whose origin is outside the box (the frame's screen tiles are not consulted). RT_ERR_STATE while the
 * context has no rays yet (rt_rays_info_t::source == 0).
 * rt_get_query_info: the LAST query's counters. The block is zeroed on the query's stream before the kernel, which adds to it once
 * per wave; the call waits for that query and reads it. n_grid + n_brute == n_rays; object_tests counts exact ray-object tests (a
 * brute-force ray: 2 per pair record); device_ms is an event pair around the kernel. RT_ERR_STATE before the first query.
 *
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: a NULL ray (work-item) array with n != 0; a misaligned device pointer; all
 * outputs NULL; a work-item >= the context's ray count. RT_ERR_STATE: a context with triangles (the ordered loop over the pair stream
 * does not know type 2, so no ray could be guaranteed a route). n == 0 returns RT_OK with nothing launched.
 *
 * There are no _multi forms: every shard of an rt_multi holds the whole scene, so rt_multi_context(m, 0) answers queries.
 *
 * NOT part of this call (each would be its own addition): contexts with triangles; a batched multi-GPU split of one query;
 * refilling a wave's idle lanes from a segment as the frame's persistent walk does. (Normals and hit points: "hit-record
 * queries" below.) */
typedef struct rt_query_info_t {
    uint64_t n_rays;        /* rays of the last query */
    uint64_t n_grid;        /* ... served by the grid */
    uint64_t n_brute;       /* ... by the ordered loop over all objects */
    uint64_t object_tests;
    double device_ms;
} rt_query_info_t;
int rt_query_closest_device(rt_context* ctx, const void* d_rays, uint64_t n, float* d_t, int32_t* d_index, void* hip_stream);
int rt_query_occluded_device(rt_context* ctx, const void* d_rays, uint64_t n, uint8_t* d_occluded, void* hip_stream);
int rt_query_closest(rt_context* ctx, const void* rays, uint64_t n, float* t, int32_t* index);
int rt_query_occluded(rt_context* ctx, const void* rays, uint64_t n, uint8_t* occluded);
int rt_query_primary(rt_context* ctx, const uint64_t* work_items, uint64_t n, float* t, int32_t* index);
int rt_get_query_info(rt_context* ctx, rt_query_info_t* info);

/* ---- hit-record queries -----------------------------------------------------------------------------------------------------------
 * WHERE a ray meets the scene and how the surface faces there: the closest-hit query with what the reference's raycast() leaves in its
 * HitRecord for the winner (shade_kernel.cl:106-112 sphere, :143-159 box) and the next ray of the reflection chain
 * (shade_and_reflect_kernel.cl:175, :260-263). For dropping an object onto the surface under the mouse, bouncing particles off the
 * scene from a device tensor, following a mirror / laser / acoustic chain, or a depth-and-normal buffer - without reading 320-byte
 * object records back and redoing the reference's arithmetic by hand. The kernels compute all of this for every frame; this call
 * hands it out.
 *
 * (t, index) are EXACTLY rt_query_closest's: the route per ray, the domain, the arithmetic flags, literal contexts, the refusal of
 * triangle contexts and the counter block are those of "ray queries" above, unchanged. Where index >= 0:
 *   point      float4: HitRecord.intersection = mv * (s' + t d') in view space, w as the reference carries it (1 for a ray with
 *              start.w == 1, direction.w == 0 on affine instances);
 *   normal     float4: HitRecord.normal = normalize((mv * (n, 0)).xyz) in xyz, w = 0; n the object-space point (sphere) or the sum of
 *              the +-1 face normals whose slab the point lies within 0.0002 of (box);
 *   reflected  rt_ray: start = intersection + 0.001 * normalize(reflection), direction = (reflection, 0), with
 *              reflection = d - 2 dot(d, normal) normal, d the ray's UN-normalised direction: the next ray of the chain, ready to be
 *              queried;
 * in the context's arithmetic mode, as the frames compute them for that winner at that time (the kernels' own functions, with the
 * scene's affine flag; a ray with an inf or a NaN among start / direction x, y, z is taken through the matrices' bottom rows like the
 * reference's, so that its w is the reference's NaN). RT_FLAG_FAST_PHONG plays no part: it never touches a vector a ray is built from.
 * Where index == -1 - a miss, a NaN time, or a masked ray - every requested record is all-zero bytes and t is as rt_query_closest
 * gives it (MAX_FLOAT for a masked ray).
 * The zero box normal follows its mode, as the frames' does: a box hit whose object-space point lies on no face within the 0.0002
 * margin (a far or tiny box, where fp32 rounding of the point exceeds the margin) has n = 0. Under the default and RT_FLAG_UNFUSED
 * arithmetic normalize(0) = 0 / 0: a NaN normal and a NaN reflected ray (direction and start). Under RT_FLAG_DEVICE_OPENCL
 * normalize(0) = 0: a zero normal and the reflection along d.
 *
 * Mask. d_mask is NULL or n int32: a ray with mask[i] < 0 is not traced and reads as a miss. This is what makes chains safe: the zero
 * record of a miss has start.w == 0 and would take the ordered brute-force loop if fed back, so the next bounce passes the previous
 * bounce's index array as its mask. rt_query_info_t::n_rays counts TRACED rays only (n_grid + n_brute == n_rays keeps holding).
 * Aliasing. A lane reads ray i and mask[i] before it writes anything of element i and touches no other element, so
 * out->reflected == d_rays (an in-place chain) and out->index == d_mask are allowed. Any other overlap is the caller's error.
 *
 * rt_query_hits_device: `d_out` points to a HOST struct, read during the call, whose members are device pointers on the context's
 * device (each may be NULL, not all). d_rays, point, normal and reflected 16-BYTE ALIGNED; t, index and d_mask 4-byte aligned.
 * ASYNCHRONOUS on hip_stream like rt_query_closest_device: no host synchronisation, no allocation after the first query.
 * rt_query_hits: the host twin, synchronous, staged through the context's grow-only patch buffer; members of `out` are host arrays.
 * rt_query_primary_hits: the pick with its record - rt_query_primary's work-items and rules (RT_ERR_STATE without rays), host results.
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: what rt_query_closest_device refuses, a NULL struct, all members NULL, a
 * misaligned device member. RT_ERR_STATE: a context with triangles. n == 0 returns RT_OK with nothing launched.
 *
 * NOT part of this call: contexts with triangles; a multi-GPU split of one query; refilling idle lanes; a whole-frame G-buffer entry
 * point (rt_generate_rays_device + rt_query_hits_device give one; a pose outside the box would send every primary ray down the
 * brute-force route - "G-buffer frames" below is that addition); materials in the record (rt_read_materials by index has them). */
typedef struct rt_hits_t {      /* every member may be NULL, not all of them */
    float*   t;          /* n floats      - as rt_query_closest                                   */
    int32_t* index;      /* n int32       - as rt_query_closest (the hittest rule)                */
    float*   point;      /* n x float4    - HitRecord.intersection, view space, w as the reference carries it */
    float*   normal;     /* n x float4    - HitRecord.normal in xyz, w = 0                        */
    void*    reflected;  /* n x 32-byte rt_ray - the next ray of the reflection chain             */
} rt_hits_t;
int rt_query_hits_device(rt_context* ctx, const void* d_rays, uint64_t n, const int32_t* d_mask, const rt_hits_t* d_out, void* hip_stream);
int rt_query_hits(rt_context* ctx, const void* rays, uint64_t n, const int32_t* mask, const rt_hits_t* out);
int rt_query_primary_hits(rt_context* ctx, const uint64_t* work_items, uint64_t n, const rt_hits_t* out);

/* ---- shaded queries ----------------------------------------------------------------------------------------------------------------
 * WHAT COLOUR comes back along a ray of the caller's own: the whole shading path - primary hit, light loop with its shadow rays,
 * reflection chain - for any number of rays, on a live context, without a frame. Light and reflection probes for a rasteriser, a mirror
 * or portal texture of a few thousand rays, extra sub-pixel rays at the edge pixels rt_render_aux's index shows, foveated or progressive
 * refinement, the colour under the mouse - without replacing the frame's rays (rt_set_rays_device wants exactly the context's ray
 * count, is synchronous, drops the camera or pose and lets one bad ray switch the frame to the literal loops) and without a second
 * context (its creation time, a second grid, and none of this context's setters). Additions only: the ABI version stays 3, and a caller
 * detects support by dlsym of rt_query_shade_device.
 *
 * Contract. Element i of rgba, t and index is, bit for bit, what a FRESH context delivers for work-item i - rt_render for rgba,
 * rt_render_aux for t and index - when it is created with the context's current objects (the create-time array through
 * records.with_transforms / with_materials / with_visibility as set so far), its current lights, the same kernel (RT_KERNEL_SHADE or
 * RT_KERNEL_SHADE_AND_REFLECT), the same max_bounces, the same arithmetic flags (RT_FLAG_UNFUSED, RT_FLAG_FAST_PHONG,
 * RT_FLAG_DEVICE_OPENCL), RT_FLAG_NO_RAYGEN and these n rays. That includes the background (0,0,0,1) of a miss and the per-kernel rule
 * of rt_set_aux_device for a NaN primary time. n is ANY count, independent of the context's ray count. A query reads the records, the
 * lights and the grid as rt_set_transforms, rt_set_visibility, rt_set_materials and rt_set_lights have left them and writes only the
 * caller's outputs and a context-owned counter block. The frame's rays, camera, pose, shard, supersampling factor, aux buffers, state
 * buffers and packed buffers are untouched: a render before and after a query is the same frame.
 *
 * Route, decided by each lane for EVERY ray of its own path (csrc/rt_query_shade.hip; rays.query_shade_route is the executable
 * definition). A ray - primary, shadow or reflection - is served by the grid walks exactly when the predicate of "ray queries" above
 * admits it (one function, shared with those kernels); shadow and reflection rays start on surfaces inside the box, as the frames' do.
 * Every other ray runs the ordered loop over all objects. A PATH is literal - the forward light loop, closest-hit shadow tests, no
 * dead-ray elimination: RT_FLAG_LITERAL - when the context is literal (by flag, for a degenerate instance, or by RT_FLAG_DEVICE_OPENCL's
 * predicate on its lights), or when its primary ray fails the DOMAIN part of the predicate: a non-finite component, start.w != 1,
 * direction.w != 0, dd outside (1e-30, 1e30). That is what a fresh context does for the whole frame when one such ray is in its buffer.
 * A primary ray that fails only the box test takes the brute-force loop for that one ray and the default path behind it. On the
 * default path a shadow ray with a NaN in it gets the closed form of the frames (the last sphere / box of the scene decides).
 * Invariant this rests on: a literal frame and a default frame agree bit for bit on every ray inside the domain (RT_FLAG_LITERAL:
 * "Results are identical"). So a batch that mixes rays of every class can be compared with ONE fresh context, which renders all of
 * it literally (tests/test_query_shade_gpu.py does).
 *
 * Mask. d_mask is NULL or n int32, as for rt_query_hits_device: a ray with a negative entry is not traced, reads as a miss - the
 * background colour, t = MAX_FLOAT, index = -1 - and enters no counter.
 *
 * rt_query_shade_device: `d_out` points to a HOST struct, read during the call, whose members are device pointers on the context's
 * device (each may be NULL, not all). d_rays and rgba 16-BYTE ALIGNED; t, index and d_mask 4-byte aligned. ASYNCHRONOUS on hip_stream
 * (NULL: the legacy default stream): no host synchronisation, no allocation after the first call. Rays and outputs must not overlap.
 * rt_query_shade: the host twin, synchronous, staged through the context's grow-only patch buffer; members of `out` are host arrays.
 * rt_query_primary_shade: the pick with its colour - rt_query_primary's work-items and rules (RT_ERR_STATE without rays), host results.
 * rt_get_query_shade_info: the LAST shaded query's counters, from a block of its own (rt_get_query_info keeps reporting the last plain
 * or hit-record query); waits for that query. RT_ERR_STATE before the first shaded query.
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: what rt_query_hits_device refuses for its arguments, a NULL struct, all members
 * NULL. RT_ERR_STATE: an RT_KERNEL_HITTEST context (a time is not a colour); a context with triangles. n == 0 returns RT_OK with
 * nothing launched.
 *
 * NOT part of this call: _multi forms (rt_multi_context(m, 0) answers); bytes out (rt_pack_device takes the float4 result); refilling
 * a wave's idle lanes (one lane keeps its ray until the path ends, so a wave lasts as long as its longest path); contexts with
 * triangles. */
typedef struct rt_shade_t {    /* every member may be NULL, not all of them */
    float*   rgba;    /* n x float4 - the pixel a frame would hold for this ray */
    float*   t;       /* n floats   - primary hit time, as rt_set_aux_device defines it for the context's kernel */
    int32_t* index;   /* n int32    - primary winner, same rule */
} rt_shade_t;
typedef struct rt_query_shade_info_t {
    uint64_t n_rays, n_grid, n_brute;   /* traced primary rays and their route (n_grid + n_brute == n_rays; masked rays not counted) */
    uint64_t n_literal;                 /* primary rays whose whole path ran the literal loops */
    uint64_t hit_rays;                  /* as rt_stats_t::hit_pixels of the fresh context */
    uint64_t rays_traced, rays_reference; /* as rt_stats_t's, summed over the batch */
    uint64_t object_tests;              /* exact ray-object tests of every ray of the paths (a brute-force ray: 2 per pair record visited) */
    double   device_ms;
} rt_query_shade_info_t;
int rt_query_shade_device(rt_context* ctx, const void* d_rays, uint64_t n, const int32_t* d_mask, const rt_shade_t* d_out, void* hip_stream);
int rt_query_shade(rt_context* ctx, const void* rays, uint64_t n, const int32_t* mask, const rt_shade_t* out);
int rt_query_primary_shade(rt_context* ctx, const uint64_t* work_items, uint64_t n, const rt_shade_t* out);
int rt_get_query_shade_info(rt_context* ctx, rt_query_shade_info_t* info);

/* ---- G-buffer frames ---------------------------------------------------------------------------------------------------------------
 * MORE THAN A COLOUR per work-item of the frame: depth, object id, hit point, surface normal and albedo of the primary hit - what a
 * denoiser, edge-directed anti-aliasing, outlines, depth compositing with a rasteriser and deferred relighting start from. The pass is
 * the frame pipeline's own primary round, run as a hittest frame (screen tiles, the grid, the literal, brute-force and no-grid routes,
 * a pose outside the grid's box served from its tiles - whatever rt_render_device takes for these rays), and one streaming kernel
 * behind it that turns (t, index) into records (csrc/rt_gbuffer.hip). It works on a context of any rt_kernel - on an RT_KERNEL_HITTEST
 * context it is rt_render_aux plus records - and on contexts WITH triangles, which the queries refuse.
 *
 * Element i of every member belongs to local work-item i of the context's current shard, in the order rt_render_device writes pixels:
 * rt_local_rays() elements, the padding of a ragged last tile included (it reads as a miss).
 *   t, index   what rt_render_aux delivers on a fresh RT_KERNEL_HITTEST context with the current objects, flags and primary rays: the
 *              loop's time (MAX_FLOAT on a miss, its NaN where it ends with NaN) and the winner where t < MAX_FLOAT, else -1. A hidden
 *              object is never named.
 *   point, normal  on a context without triangles, bit for bit what rt_query_primary_hits returns for the work-item's global index
 *              ("hit-record queries": the arithmetic flags, the affine shortcut only for a ray of finite x, y, z, the zero box normal
 *              per mode, RT_FLAG_FAST_PHONG playing no part). For a triangle winner: point = t * d + s per component (one fma in the
 *              fused modes, product then sum under RT_FLAG_UNFUSED), normal = normalize(e1 x e2), never contracted
 *              (hits.hit_records is the executable definition). All-zero bytes where index == -1.
 *   albedo     where index >= 0: (diffuse.r, diffuse.g, diffuse.b, 1) of rt_read_materials(ctx, .., index, 1), moved, not computed
 *              with (a NaN or an inf passes through); zero bytes where index == -1.
 * The pass sees the context as the setters left it - camera, pose, ray buffer, shard, materials, transforms, visibility (lights play
 * no part) - and leaves the FRAME alone: a render before and after it is the same frame, aux buffers set for the next render stay set
 * for the next render, and rt_get_stats, rt_timing_* and last_kernel_ms keep describing renders (the pass has event pairs of its own:
 * rt_get_gbuffer_info).
 * Supersampling. Records are per SAMPLE, as rt_local_rays() counts them; nothing is filtered (a mean of ids or normals means nothing).
 * Unlike aux buffers, the pass is accepted with any factor.
 *
 * rt_render_gbuffer_device: `d_out` points to a HOST struct, read during the call, whose members are device pointers on the context's
 * device (each may be NULL, not all). point, normal and albedo 16-BYTE ALIGNED; t and index 4-byte aligned. Stream semantics are
 * rt_render_device's: NULL is the legacy default stream, the large-scene path may synchronise once per batch of rounds, and the record
 * kernel is enqueued behind the trace on the same stream with no further host synchronisation. (t, index) the caller did not ask for
 * are staged in context-owned, grow-only buffers that rt_destroy frees: nothing is allocated after the first pass of a given size.
 * That staging, the pass's discard buffer for the hittest frame's own float and the frame's state buffers are the CONTEXT's: two passes,
 * or a pass and a render, of one context on different streams must be ordered by the caller, as two renders must.
 * rt_render_gbuffer: the host twin, synchronous, on the context's stream; members of `out` are host arrays, staged through
 * context-owned buffers; only the requested members are copied out.
 * rt_get_gbuffer_info: the LAST pass; waits for it. RT_ERR_STATE before the first pass.
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: a NULL struct, all members NULL, a misaligned device member. RT_ERR_STATE: no
 * primary rays yet. rt_local_rays() == 0 returns RT_OK with nothing launched.
 *
 * NOT part of this call (each would be its own addition): _multi forms (rt_multi_context(m, r) gives each shard's); byte outputs; a
 * reflected ray (rt_query_hits_device has it); the passes of rt_render's large frames (the pass is one launch over the shard); lifting
 * the queries' refusal of contexts with triangles. */
typedef struct rt_gbuffer_t {   /* every member may be NULL, not all of them; rt_local_rays() elements each */
    float*   t;        /* float   - primary hit time, the hittest rule (MAX_FLOAT on a miss, the loop's NaN where it ends with NaN) */
    int32_t* index;    /* int32   - winner where t < MAX_FLOAT, else -1 */
    float*   point;    /* float4  - HitRecord.intersection, as rt_hits_t::point */
    float*   normal;   /* float4  - HitRecord.normal in xyz, w = 0, as rt_hits_t::normal */
    float*   albedo;   /* float4  - the winner's diffuse rgb as rt_read_materials returns it, w = 1 */
} rt_gbuffer_t;
typedef struct rt_gbuffer_info_t {
    uint64_t n_items, hits;                 /* work-items of the pass (padding included), those with index >= 0 */
    double   trace_ms, records_ms;          /* event pairs around the primary round and around the record kernel */
    uint32_t wavefront, reserved;
} rt_gbuffer_info_t;
int rt_render_gbuffer_device(rt_context* ctx, const rt_gbuffer_t* d_out, void* hip_stream);
int rt_render_gbuffer(rt_context* ctx, const rt_gbuffer_t* out);          /* host arrays, synchronous */
int rt_get_gbuffer_info(rt_context* ctx, rt_gbuffer_info_t* info);        /* RT_ERR_STATE before the first pass */

/* ---- ambient-occlusion frames ------------------------------------------------------------------------------------------------------
 * The first CONSUMER of a G-buffer: K occlusion rays per work-item, started at its hit point along directions of a caller's table on
 * the normal's side, traced and counted in ONE kernel (csrc/rt_ao.hip) - instead of a G-buffer pass, n * K rays of 32 bytes built by
 * the caller, rt_query_occluded_device and a reduction. ao.py (rays, reduce) is the executable definition.
 *
 * Per item i: point[i] and normal[i] (float4, as rt_gbuffer_t / rt_hits_t deliver them) and, optionally, index[i] (int32; NULL: every
 * item may be live). The item's global work-item number g is i for rt_ao*; for rt_render_ao* it is the shard's global index (the
 * mapping of rt_set_shard), so that a sharded frame equals the unsharded one item for item.
 *   live       index[i] >= 0 (where index is given) and point.xyz, normal.xyz all finite. A dead item traces nothing, reads
 *              unoccluded = K and ao = 1.0f, and enters no counter.
 *   set        h = (uint32)g * 0x9E3779B1u (mod 2^32), set = (h >> 16) % n_sets.
 *   sample k   d = dirs[set * K + k].xyz; s = (d.x * n.x + d.y * n.y) + d.z * n.z; if s < 0 then d = -d (a NaN or zero s keeps d);
 *              start.c = p.c + (bias * n.c) for c = x, y, z; start.w = 1; direction = (d, 0). All fp32, every product and sum
 *              rounded, nothing contracted, in every arithmetic mode. The library neither normalises nor scales a direction: its
 *              LENGTH IS THE OCCLUSION RADIUS, as for every occlusion query (something on start .. start + direction).
 *   result     unoccluded[i] = K - sum over k of occluded(ray(i, k)), a uint8; occluded is exactly rt_query_occluded's answer for that
 *              ray on this context: the per-ray route ("ray queries"), the grid's any-hit walk on the grid, off it - literal
 *              contexts, a start outside the box, contexts without a grid - the ordered loop with !(T >= 1 || T < 0).
 *              ao[i] = (float)unoccluded[i] * (1.0f / K), exact for these K.
 * The normal is the reference's (mv * (n, 0), not the inverse transpose) and is NOT turned towards the viewer: a non-uniformly scaled
 * sphere can occlude some of its own samples. That is the reference's geometry.
 *
 * rt_ao_params_t: samples K is one of 1, 2, 4, 8, 16, 32, 64; n_sets 1 .. 4096; bias finite and >= 0; reserved 0; dirs n_sets * K
 * float4 (w ignored), 16-byte aligned - device memory for the _device forms, host memory for the twins, which stage it through the
 * context's grow-only patch buffer as the query twins stage their rays. rt_ao_t: each member may be NULL, not both; ao 4-byte
 * aligned, unoccluded of any alignment. Outputs must not overlap inputs.
 *
 * rt_ao_device: the pass alone on n items of the caller's, any n; point and normal 16-byte aligned, index 4-byte aligned. It touches
 * only the caller's outputs and a counter block of its own, is asynchronous (no host synchronisation; NULL is the legacy default
 * stream) and works on a context of any rt_kernel, also one without primary rays. rt_ao: its host twin, synchronous.
 * rt_render_ao_device: rt_local_rays() elements in rt_render_device's order - per SAMPLE under supersampling, per shard when sharded.
 * It runs the G-buffer pass ("G-buffer frames") into context-owned, grow-only staging (index, point, normal), then the AO kernel on
 * the same stream; stream semantics are rt_render_gbuffer_device's; nothing is allocated after the first call of a size. The frame
 * is left alone exactly as the G-buffer pass leaves it, and rt_get_gbuffer_info afterwards describes the internal pass. The staging is
 * the CONTEXT's: order two passes of one context on different streams, as two renders. rt_render_ao: the host twin, synchronous.
 * rt_get_ao_info: the LAST pass of either kind; waits for it. n_grid + n_brute == n_rays == K * n_live; gbuffer_ms is 0 for rt_ao*.
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: a NULL params or out struct, both outputs NULL, another K, n_sets outside
 * 1 .. 4096, a bias that is negative or not finite, reserved != 0, NULL dirs, NULL point or normal with n != 0, a misaligned device
 * pointer. RT_ERR_STATE: a context with triangles (the queries' reason); rt_render_ao* without primary rays; rt_get_ao_info before the
 * first pass. n == 0 or rt_local_rays() == 0 returns RT_OK with nothing launched.
 *
 * NOT part of this call: cosine weights or normalisation inside the library; turning the normal to the viewer; bent normals; a
 * filtered result under supersampling; byte or _multi forms; fusing the G-buffer's record kernel into the AO kernel; refilling idle
 * lanes; contexts with triangles. */
typedef struct rt_ao_params_t { uint32_t samples, n_sets; float bias; uint32_t reserved; const void* dirs; } rt_ao_params_t;
typedef struct rt_ao_t { uint8_t* unoccluded; float* ao; } rt_ao_t;                /* each may be NULL, not both */
typedef struct rt_ao_info_t {
    uint64_t n_items, n_live, n_rays, n_grid, n_brute, object_tests;  /* items of the pass, the live ones, rays, rays per route, exact tests */
    double   gbuffer_ms, ao_ms;                                       /* event pairs around the internal G-buffer pass and the AO kernel */
} rt_ao_info_t;
int rt_ao_device(rt_context* ctx, const float* d_point, const float* d_normal, const int32_t* d_index, uint64_t n,
                 const rt_ao_params_t* params, const rt_ao_t* d_out, void* hip_stream);   /* the pass alone, any n, asynchronous */
int rt_ao(rt_context* ctx, const float* point, const float* normal, const int32_t* index, uint64_t n, const rt_ao_params_t* params,
          const rt_ao_t* out);
int rt_render_ao_device(rt_context* ctx, const rt_ao_params_t* params, const rt_ao_t* d_out, void* hip_stream);  /* G-buffer pass + the pass */
int rt_render_ao(rt_context* ctx, const rt_ao_params_t* params, const rt_ao_t* out);
int rt_get_ao_info(rt_context* ctx, rt_ao_info_t* info);                  /* RT_ERR_STATE before the first pass */

/* ---- filtered ambient occlusion ----------------------------------------------------------------------------------------------------
 * The AO pass picks an item's direction set by a hash of its work-item number: interleaved sampling, which trades banding for noise
 * per item and expects a spatial filter to recombine the sets. This is that filter: an edge-aware box blur of the COUNTS over a
 * (2r + 1)^2 window, stopped by the G-buffer's normals and planes, in ONE kernel (csrc/rt_ao_filter.hip: a 64 x 16 tile and its halo
 * in LDS). ao.py: filter() is the executable definition; the kernel matches it bit for bit - no tolerance anywhere.
 *
 * Inputs: a row-major array of width x rows items, n = width * rows; item i sits at column i % width, row i / width. Per item
 * unoccluded[i] (a uint8, as rt_ao_t delivers it), point[i] and normal[i] (float4) and, optionally, index[i] (int32; NULL: every item
 * may be live). rt_ao_filter_params_t: radius r is 1 .. 4, normal_min any float, plane_max finite and >= 0, reserved 0; samples K is
 * one of 1, 2, 4 ... 64.
 *   live(i)         the AO pass's rule: index[i] >= 0 (where index is given) and point.xyz, normal.xyz all finite.
 *   window of p     every q with |col_q - col_p| <= r and |row_q - row_p| <= r inside the array. Nothing wraps; nothing outside the
 *                   array is read.
 *   accepted(p, q)  for a live p and q != p: live(q), and c = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z with c >= normal_min,
 *                   and d = P_q - P_p per component, e = (n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z with fabsf(e) <= plane_max. All
 *                   fp32, every product and sum rounded, nothing contracted, sums left to right, in EVERY arithmetic mode. A
 *                   comparison with a NaN is false (inf - inf makes one). A live p always accepts itself, untested.
 *   a live p        taps[p] = the accepted items, 1 .. (2r + 1)^2; sum[p] = the integer sum of their unoccluded bytes as they are
 *                   (not clamped to K); ao[p] = (float)sum[p] / (float)(taps[p] * K), ONE correctly rounded IEEE division in every
 *                   arithmetic mode.
 *   a dead p        taps = 0, ao = 1.0f.
 *   grey[p]         the byte the table of "8-bit frames" gives ao[p].
 * The weights are 0 or 1 and the sums integers: the result does not depend on the order of summation.
 *
 * rt_ao_filtered_t: each member may be NULL, not all; ao 4-byte aligned, grey and taps of any alignment. Outputs must not overlap inputs.
 * rt_ao_filter_device: the pass alone on the caller's device arrays, any width and rows, on a context of any kind - also one without
 * primary rays or with triangles (it reads nothing of the scene). point and normal 16-byte aligned, index 4-byte aligned, unoccluded
 * of any alignment. It touches only the caller's outputs and a counter block of its own, allocates nothing after the first call and
 * is asynchronous (NULL is the legacy default stream). rt_ao_filter: its host twin, synchronous, staged through the context's
 * grow-only patch buffer as rt_ao stages.
 * rt_render_ao_filtered_device: the G-buffer pass and the AO kernel exactly as rt_render_ao_device runs them - the counts go to a
 * context-owned grow-only buffer - then the filter, all on one stream; stream semantics are rt_render_gbuffer_device's, the frame is
 * left alone as rt_render_ao_device leaves it, and rt_get_ao_info and rt_get_gbuffer_info afterwards describe the internal passes.
 * The filter's width is the frame's SAMPLE-grid width - the pinhole camera's, or the pose's (the context remembers a pose's width and
 * height) - and rows = rt_local_rays() / width: under supersampling it filters samples. rt_render_ao_filtered: the host twin.
 * rt_get_ao_filter_info: the LAST pass of either kind; waits for it. accepted is the sum of taps over all items; gbuffer_ms and ao_ms
 * are 0 for rt_ao_filter*.
 * Refused, nothing touched - RT_ERR_INVALID_ARGUMENT: a NULL params or out struct, all outputs NULL, radius outside 1 .. 4, a
 * plane_max that is negative or not finite, reserved != 0, another K, width * rows overflowing, a NULL input (unoccluded, point,
 * normal) with n != 0, a misaligned device pointer, and the AO parameter errors as rt_render_ao_device reports them. RT_ERR_STATE, the
 * frame forms only: a context with triangles (the AO pass's own refusal); a sharded context (world > 1: a tile's neighbours live on
 * other shards); no primary rays; primary rays from a plain ray buffer (rt_set_rays*, RT_FLAG_NO_RAYGEN: it has no width);
 * rt_get_ao_filter_info before the first pass. n == 0 returns RT_OK with nothing launched.
 *
 * NOT part of this call: sharded and _multi forms (they need a halo exchange); Gaussian or other non-binary weights; separable or
 * a-trous passes; temporal accumulation; filtering colour frames; bent normals; fusing the filter into the AO kernel. */
typedef struct rt_ao_filter_params_t { uint32_t radius; float normal_min, plane_max; uint32_t reserved; } rt_ao_filter_params_t;
typedef struct rt_ao_filtered_t { float* ao; uint8_t* grey; uint8_t* taps; } rt_ao_filtered_t;   /* each may be NULL, not all */
typedef struct rt_ao_filter_info_t {
    uint64_t n_items, n_live, accepted;      /* items of the pass, the live ones, the sum of taps */
    double   gbuffer_ms, ao_ms, filter_ms;   /* event pairs around the internal G-buffer pass, the AO kernel and the filter kernel */
} rt_ao_filter_info_t;
int rt_ao_filter_device(rt_context* ctx, const uint8_t* d_unoccluded, const float* d_point, const float* d_normal, const int32_t* d_index,
                        uint64_t width, uint64_t rows, uint32_t samples, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* d_out,
                        void* hip_stream);                                     /* the pass alone, asynchronous */
int rt_ao_filter(rt_context* ctx, const uint8_t* unoccluded, const float* point, const float* normal, const int32_t* index, uint64_t width,
                 uint64_t rows, uint32_t samples, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out);
int rt_render_ao_filtered_device(rt_context* ctx, const rt_ao_params_t* params, const rt_ao_filter_params_t* filter,
                                 const rt_ao_filtered_t* d_out, void* hip_stream);   /* G-buffer pass + AO kernel + the filter */
int rt_render_ao_filtered(rt_context* ctx, const rt_ao_params_t* params, const rt_ao_filter_params_t* filter, const rt_ao_filtered_t* out);
int rt_get_ao_filter_info(rt_context* ctx, rt_ao_filter_info_t* info);         /* RT_ERR_STATE before the first pass */

void rt_destroy(rt_context* ctx);

/* ---- several GPUs from one process ------------------------------------------------------------------------------------
 * `new HIPRaytracer(objects, lights, rays, MAX_BOUNCES)` on a multi-GPU node (north_star: "row-tiles across the 8 GPUs of
 * one node"; the reference drives exactly one device, OpenCLRaytracer.cpp:36-44). rt_create_multi builds one context per
 * entry of `devices` (the same ordinal may appear more than once: a rehearsal on fewer GPUs), each with
 * rt_set_shard(tile_rays, r, n_devices): interleaved tiles of `tile_rays` consecutive rays (a row-tile = tile_rows * width).
 * A render runs every context on a host thread of its own, on its own device and stream; each context's packed tiles are
 * then copied device-to-device (peer access where the runtime grants it) straight to their final offsets in the frame held
 * on devices[0] - the gather of SURVEY.md 8e without a second process or a collective library.
 *   rt_render_multi         synchronous, like rt_render: the whole frame (n_rays elements) in a host buffer owned by `m`
 *   rt_render_multi_device  the whole frame into caller-provided memory ON devices[0] (n_rays elements, padded up to whole
 *                           tiles: rt_multi_frame_elems()); returns when the frame is complete. The shards write d_frame
 *                           from their own streams: the buffer must be IDLE on entry (no pending work of the caller on it -
 *                           synchronise the stream that last touched it first)
 *   rt_multi_context        the r-th context (rt_count_rays / rt_get_stats / rt_timing_* per shard)
 *   rt_count_rays_multi     the untimed counted render on every shard
 *   rt_get_stats_multi      rays_traced / rays_reference / hit_pixels / object_tests / local_rays summed over the shards,
 *                           last_kernel_ms and rounds of the slowest one (the whole frame's figures, like Render()'s frame)
 * rt_render_multi: every device copies ITS tiles from its own memory into the pinned (portable) host frame, on its own
 * stream and PCIe link (one strided device-to-host copy per shard); nothing is gathered on devices[0]. */
typedef struct rt_multi rt_multi;
int rt_create_multi(rt_multi** m, const void* objs, uint32_t n_objs, const void* lights, uint32_t n_lights,
                    const void* rays, uint64_t n_rays, uint32_t max_bounces, int kernel,
                    const int* devices, uint32_t n_devices, uint64_t tile_rays, uint32_t flags);
/* rt_set_camera on every context, any number of times between renders. An rt_multi KEEPS ITS TILE SIZE: the tile_rays given to
 * rt_create_multi (or derived there from the first pinhole width: 16 rows of it), in rays - after a camera of another width
 * the tiles are no whole rows, the frame is the same. rt_multi_frame_elems() therefore never changes. */
int rt_set_camera_multi(rt_multi* m, uint32_t width, uint32_t height, float z);
/* rt_set_pose ("posed cameras", above) on every context, all or none: every shard runs its verdict pass and its refusals, on its own
 * device, stream and host thread; only if none refuses, every shard generates the frame's rays in its own buffer. */
int rt_set_pose_multi(rt_multi* m, uint32_t width, uint32_t height, float z, const float mat[9], const float origin[3]);
/* rt_set_lights ("replaceable lights", above) on every context, all or none: the arguments are validated before any shard is touched. */
int rt_set_lights_multi(rt_multi* m, const void* lights, uint32_t n_lights);
/* rt_set_materials ("replaceable materials", above; host arrays only) on every context, all or none: the arguments are validated
 * before any shard is touched. */
int rt_set_materials_multi(rt_multi* m, const void* materials, uint32_t first, uint32_t count);
/* rt_set_transforms ("replaceable transforms", above) on every context, all or none: every refusal is evaluated on every shard
 * before any shard is touched. */
int rt_set_transforms_multi(rt_multi* m, const void* transforms, uint32_t first, uint32_t count);
/* rt_set_visibility ("replaceable visibility", above; host masks only) on every context, all or none: the arguments are validated
 * before any shard is touched. */
int rt_set_visibility_multi(rt_multi* m, const uint8_t* visible, uint32_t first, uint32_t count);
uint64_t rt_multi_frame_elems(const rt_multi* m);
int rt_render_multi(rt_multi* m, const float** out);
int rt_render_multi_device(rt_multi* m, void* d_frame);
/* rt_render_multi in bytes (8-bit frames, above): every shard packs its own tiles on its own device and stream, then ONE
 * strided device-to-host copy of bytes per shard into a pinned portable byte frame owned by `m` (n_rays pixels). */
int rt_render_multi_packed(rt_multi* m, int format, const uint8_t** out);
/* rt_set_supersampling on every context ("supersampled frames", above), all or none. The multi's fixed tile_rays must hold whole
 * pixel rows: tile_rays % (s * width) == 0 (the derived default, 16 rows, is fine for s = 2 and 4 and refused for s = 3: such a
 * caller passes tile_rays to rt_create_multi). Every shard filters its own tiles; the rt_render_multi* calls then deliver
 * rt_multi_frame_pixels() = rt_multi_frame_elems() / s^2 elements (n_rays / s^2 of them the picture). */
int      rt_set_supersampling_multi(rt_multi* m, uint32_t s);
uint64_t rt_multi_frame_pixels(const rt_multi* m);
int rt_count_rays_multi(rt_multi* m);
int rt_get_stats_multi(rt_multi* m, rt_stats_t* stats);
rt_context* rt_multi_context(rt_multi* m, uint32_t r);
const char* rt_multi_last_error(const rt_multi* m);
void rt_destroy_multi(rt_multi* m);
/* Message of the last failure on this context (ctx may be NULL for a failed rt_create). */
const char* rt_last_error(const rt_context* ctx);
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HIP_RAYTRACER_H */
