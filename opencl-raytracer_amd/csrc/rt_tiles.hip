// rt_tiles.hip - the posed camera's screen tiles, built where the objects are (tiles.py: pose_screen_tiles is the definition,
// rt_grid.h: ScreenTiles has the derivation and the layout wf_trace_primary_tiles reads).
//
// Five passes on one stream, none of which waits on another workgroup (ordering is the stream's):
//   tile_rects    one lane per object, in double: the sphere in the camera frame, its tile rectangle, its key, its class; the
//                 pair total (64 bit), the whole-screen objects and their count go to one small record
//   tile_expand   <count>: every listed (object, tile) pair bumps its tile's counter (non-returning atomics). A lane expands a
//                 small rectangle itself; a large one is expanded by the whole wave, 64 tiles per trip. Returns at once when the
//                 record says the table is over its budget - the host will refuse it - so a pose that floods the screen costs
//                 one pass over the objects, not billions of atomics
//   tile_scan_*   exclusive scan of the counters in three launches (block sums, scan of the sums, add): tile_start, the fill
//                 cursors, the total and the longest list
//   tile_expand   <fill>: the same expansion, a returning atomic on the tile's cursor places the object index in `scratch`
//   tile_sort_*   a tile's list by (key, index) ascending into `entries` as {index, key bits}: rank by comparison, one wave for
//                 up to 64 entries (registers and shuffles), one workgroup for up to 1024 (8 KB of LDS). (key, index) is a total
//                 order, so the table does not depend on where the atomics landed. The small sort also writes the global list,
//                 by index, and the zeroed entry behind it.
// Every loop is bounded by a rectangle's area or a list's length; every store is guarded by the size of its array.
#include "rt_tiles.h"
#include "rt_grid_radii.h"

namespace rt {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kScanItems = 4;                      // counters per thread of a scan block
constexpr uint32_t kScanBlock = kBlock * kScanItems;    // 1024 tiles per scan block
constexpr uint32_t kOwnArea = 8;                        // rectangles up to this many tiles are expanded by their own lane

__device__ __forceinline__ float float_below(float f) {  // nextafterf(f, -inf)
    if (!(f == f) || f == -__builtin_inff()) return f;
    if (f == 0.f) return -1.401298464e-45f;
    const uint32_t b = __float_as_uint(f);
    return __uint_as_float(f > 0.f ? b - 1u : b + 1u);
}
__device__ __forceinline__ float float_above(float f) { return -float_below(-f); }

// tangent-plane extents of the ball (cu, cz, R) at depth z along one image axis, padded and rounded outwards (screen_rect's)
__device__ __forceinline__ void extent(double cu, double cz, double R, double z, double pad, double& lo, double& hi) {
    const double inf = __builtin_inf();
    const double a = cz * cz - R * R, b = -2.0 * z * cu * cz, c = (z * z) * (cu * cu - R * R);
    const double disc = b * b - 4.0 * a * c;
    lo = -inf; hi = inf;
    if (!(a > 0) || !(disc >= 0)) return;
    const double sq = __builtin_sqrt(disc);
    const double u0 = (-b - sq) / (2.0 * a), u1 = (-b + sq) / (2.0 * a);
    double l = u0 < u1 ? u0 : u1, h = u0 < u1 ? u1 : u0;
    l = (l - (1.0 + 1e-6 * __builtin_fabs(l))) - pad;
    h = (h + (1.0 + 1e-6 * __builtin_fabs(h))) + pad;
    lo = (double)float_below((float)l);
    hi = (double)float_above((float)h);
}

// A pose outside the grid's box (in front of tile_rects): one lane per object, grid_radii's expressions with the farthest origin
// and the largest |origin| taken over the box AND the pose's origin. rg' is finite for every finite origin (squares of fp32 values
// in double); should it not be, the largest double stands for it, which tile_rects makes a whole-screen entry.
__global__ __launch_bounds__(kBlock) void pose_spheres(const PoseSphereArgs a, const double* __restrict__ bounds,
                                                       const double* __restrict__ spheres, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_objs) return;
    const double* b = bounds + (unsigned long long)kBoundDoubles * i;
    const double c[3] = {b[0], b[1], b[2]};
    double rg = spheres[4ull * i + 3];
    if (rg >= 0 && rg != __builtin_inf()) {  // else the always-list / never hit: what it is
        const double D2 = pose_far2(c, a.o, farthest_corner2(c, a.lo, a.hi));
        const RadiusTerms t = registration_terms(c, b[3], b[4], (uint32_t)b[5], D2, pose_reach(a.o, a.S_max), a.cell);
        rg = (t.rg - t.rg) == 0.0 ? t.rg : 1.7976931348623157e308;
    }
    out[4ull * i] = spheres[4ull * i];
    out[4ull * i + 1] = spheres[4ull * i + 1];
    out[4ull * i + 2] = spheres[4ull * i + 2];
    out[4ull * i + 3] = rg;
}

__global__ __launch_bounds__(kBlock) void tile_rects(const PoseTileArgs a, const PoseTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long covered = 0ull;
    bool global = false;
    if (i < a.n_objs) {
        uint4 rc = make_uint4(1u, 0u, 1u, 0u);
        float key = -__builtin_inff();
        const double cx = b.spheres[4ull * i], cy = b.spheres[4ull * i + 1], cz = b.spheres[4ull * i + 2], R = b.spheres[4ull * i + 3];
        if (R >= 0 && R != __builtin_inf()) {
            const double d0 = cx - a.o[0], d1 = cy - a.o[1], d2 = cz - a.o[2];
            const double px = (a.n[0] * d0 + a.n[1] * d1) + a.n[2] * d2;
            const double py = (a.n[3] * d0 + a.n[4] * d1) + a.n[5] * d2;
            const double pz = (a.n[6] * d0 + a.n[7] * d1) + a.n[8] * d2;
            const double Rp = R * a.sig1 + a.absk * (((__builtin_fabs(cx) + __builtin_fabs(cy)) + __builtin_fabs(cz)) + a.o1);
            const double chk = ((px + py) + pz) + Rp;
            const bool finite = (chk - chk) == 0.0;
            if (!(finite && pz - Rp >= 0)) {  // else entirely behind the camera: in no list
                const double inf = __builtin_inf();
                double xlo = -inf, xhi = inf, ylo = -inf, yhi = inf;
                if (finite && !(pz + Rp >= 0)) {  // else it reaches the camera plane: the whole screen
                    extent(px, pz, Rp, a.z, a.pad, xlo, xhi);
                    extent(py, pz, Rp, a.z, a.pad, ylo, yhi);
                }
                const double c0 = xlo + a.half_w, c1 = xhi + a.half_w, r0 = a.top - yhi, r1 = a.top - ylo;
                const double wm = (double)(a.width - 1u), hm = (double)(a.height - 1u);
                const double cx0 = c0 >= 0 ? __builtin_floor(c0) : 0.0, ry0 = r0 >= 0 ? __builtin_floor(r0) : 0.0;  // (a NaN keeps the screen's edge)
                const double cx1 = c1 <= wm ? __builtin_ceil(c1) : wm, ry1 = r1 <= hm ? __builtin_ceil(r1) : hm;
                if (cx0 <= cx1 && ry0 <= ry1) {  // 0 <= cx0 <= cx1 <= W - 1 < 2^24: the conversions are exact
                    rc = make_uint4((uint32_t)cx0 >> 6, (uint32_t)cx1 >> 6, (uint32_t)ry0 >> 3, (uint32_t)ry1 >> 3);
                    covered = (unsigned long long)(rc.y - rc.x + 1u) * (rc.w - rc.z + 1u);
                    double kd = (pz + Rp) / a.zme;
                    kd = kd - __builtin_fabs(kd) * 0x1p-40;
                    if (kd == kd) key = float_below((float)kd);
                    const unsigned long long tiles = (unsigned long long)a.tiles_x * a.tiles_y;
                    if ((covered == tiles && tiles > 1ull) || R > a.whole_r) {  // the whole screen (or, off the box, as big as the scene): the global list
                        global = true;
                        covered = 0ull;
                        rc = make_uint4(1u, 0u, 1u, 0u);
                    }
                }
            }
        }
        b.rect[i] = rc;
        b.key[i] = key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) covered += __shfl_xor(covered, m, 64);
    if ((threadIdx.x & 63u) == 0u && covered != 0ull) atomicAdd(&b.record->pairs, covered);
    if (global) {
        const uint32_t slot = atomicAdd(&b.record->n_global, 1u);
        if (slot < kPoseMaxGlobal) b.record->global_ids[slot] = i;
    }
}

template <bool FILL>
__device__ __forceinline__ void emit(const PoseTileBuffers& b, uint32_t tile, uint32_t n_tiles, uint32_t object, uint32_t total) {
    if (tile >= n_tiles) return;
    if (FILL) {
        const uint32_t pos = atomicAdd(&b.cursor[tile], 1u);
        if (pos < total) b.scratch[pos] = object;
    } else {
        (void)__hip_atomic_fetch_add(&b.count[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // result unused: non-returning
    }
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void tile_expand(const PoseTileArgs a, const PoseTileBuffers b, uint32_t total) {
    if (!FILL && (b.record->pairs > a.budget || b.record->n_global > kPoseMaxGlobal)) return;  // the host refuses this table
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_tiles = a.tiles_x * a.tiles_y;
    const uint4 rc = i < a.n_objs ? b.rect[i] : make_uint4(1u, 0u, 1u, 0u);
    const bool listed = rc.y >= rc.x && rc.w >= rc.z;
    const uint32_t w = listed ? rc.y - rc.x + 1u : 0u, h = listed ? rc.w - rc.z + 1u : 0u;
    const uint32_t area = w * h;  // <= tiles <= 2^20
    if (area <= kOwnArea)
        for (uint32_t k = 0; k < area; ++k) emit<FILL>(b, (rc.z + k / w) * a.tiles_x + rc.x + k % w, n_tiles, i, total);
    unsigned long long big = __ballot(area > kOwnArea);
    while (big != 0ull) {  // one large rectangle at a time, 64 of its tiles per trip
        const int j = __ffsll((long long)big) - 1;
        big &= big - 1ull;
        const uint32_t bx = (uint32_t)__shfl((int)rc.x, j, 64), by = (uint32_t)__shfl((int)rc.z, j, 64);
        const uint32_t bw = (uint32_t)__shfl((int)w, j, 64), ba = (uint32_t)__shfl((int)area, j, 64);
        const uint32_t bi = (uint32_t)__shfl((int)i, j, 64);
        for (uint32_t k = lane; k < ba; k += 64u) emit<FILL>(b, (by + k / bw) * a.tiles_x + bx + k % bw, n_tiles, bi, total);
    }
}

// exclusive scan of one value per thread across a workgroup of kBlock threads; `all` = the workgroup's sum
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* lds, uint32_t& all) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kBlock; off <<= 1) {
        const uint32_t add = t >= off ? lds[t - off] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    all = lds[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kBlock) void tile_scan_sums(const PoseTileBuffers b, uint32_t n_tiles) {
    __shared__ uint32_t lds[kBlock], lmax[kBlock / 64];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t sum = 0, mx = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        const uint32_t v = base + k < n_tiles ? b.count[base + k] : 0u;
        sum += v;
        mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)mx, m, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0u) lmax[threadIdx.x / 64u] = mx;
    uint32_t all;
    (void)block_exclusive(sum, lds, all);  // (its barriers also publish lmax)
    if (threadIdx.x == 0u) {
        b.sums[blockIdx.x] = all;
        uint32_t m = lmax[0];
        for (uint32_t k = 1; k < kBlock / 64; ++k) m = lmax[k] > m ? lmax[k] : m;
        if (m != 0u) atomicMax(&b.record->max_list, m);
    }
}

__global__ __launch_bounds__(kBlock) void tile_scan_top(const PoseTileBuffers b, uint32_t n_blocks) {  // one workgroup; n_blocks <= 1024
    __shared__ uint32_t lds[kBlock];
    const uint32_t base = threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n_blocks ? b.sums[base + k] : 0u;
        sum += v[k];
    }
    uint32_t all;
    uint32_t run = block_exclusive(sum, lds, all);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (base + k < n_blocks) b.sums[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0u) b.record->total = all;
}

__global__ __launch_bounds__(kBlock) void tile_scan_add(const PoseTileBuffers b, uint32_t n_tiles) {
    __shared__ uint32_t lds[kBlock];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n_tiles ? b.count[base + k] : 0u;
        sum += v[k];
    }
    uint32_t all;
    uint32_t run = b.sums[blockIdx.x] + block_exclusive(sum, lds, all);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (base + k < n_tiles) { b.tile_start[base + k] = run; b.cursor[base + k] = run; }
        run += v[k];
        if (base + k + 1u == n_tiles) b.tile_start[n_tiles] = run;
    }
}

__device__ __forceinline__ bool entry_before(uint32_t ia, float ka, uint32_t ib, float kb) { return ka < kb || (ka == kb && ia < ib); }

// one wave per tile (and one for the global list, "tile" n_tiles): lists of up to 64 entries
__global__ __launch_bounds__(kBlock) void tile_sort_wave(const PoseTileBuffers b, uint32_t n_tiles, uint32_t total, uint32_t n_global) {
    const uint32_t tile = blockIdx.x * (kBlock / 64u) + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (tile > n_tiles) return;
    uint32_t e0, len, idx = 0xffffffffu;
    float key = __builtin_inff();
    if (tile < n_tiles) {
        e0 = b.tile_start[tile];
        len = b.tile_start[tile + 1u] - e0;
        if (len == 0u || len > 64u || e0 + len > total) return;
        if (lane < len) { idx = b.scratch[e0 + lane]; key = b.key[idx]; }
    } else {  // the global list: no key, by index; then the zeroed entry behind the last
        e0 = total;
        len = n_global < kPoseMaxGlobal ? n_global : kPoseMaxGlobal;
        if (lane < len) { idx = b.record->global_ids[lane]; key = 0.f; }
        if (lane == 0u) b.entries[total + len] = make_uint2(0u, 0u);
    }
    uint32_t rank = 0;
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t ij = (uint32_t)__shfl((int)idx, (int)j, 64);
        const float kj = __shfl(key, (int)j, 64);
        rank += entry_before(ij, kj, idx, key) ? 1u : 0u;
    }
    if (lane < len) b.entries[e0 + rank] = make_uint2(idx, __float_as_uint(key));
}

// one workgroup per tile: lists of 65 .. 1024 entries, ranked in LDS (8 KB)
__global__ __launch_bounds__(kBlock) void tile_sort_block(const PoseTileBuffers b, uint32_t total) {
    __shared__ uint2 list[kPoseMaxList];
    const uint32_t e0 = b.tile_start[blockIdx.x], len = b.tile_start[blockIdx.x + 1u] - e0;
    if (len <= 64u || len > kPoseMaxList || e0 + len > total) return;  // (uniform across the workgroup)
    for (uint32_t k = threadIdx.x; k < len; k += kBlock) {
        const uint32_t idx = b.scratch[e0 + k];
        list[k] = make_uint2(idx, __float_as_uint(b.key[idx]));
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < len; k += kBlock) {
        const uint2 mine = list[k];
        const float km = __uint_as_float(mine.y);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < len; ++j) {
            const uint2 o = list[j];
            rank += entry_before(o.x, __uint_as_float(o.y), mine.x, km) ? 1u : 0u;
        }
        b.entries[e0 + rank] = mine;
    }
}

}  // namespace

hipError_t launch_pose_tile_count(const PoseTileArgs& a, const PoseTileBuffers& b, hipStream_t stream) {
    const uint32_t n_tiles = a.tiles_x * a.tiles_y;
    if (a.n_objs == 0 || n_tiles == 0 || n_tiles > kPoseMaxTiles) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(b.record, 0, sizeof(PoseTileRecord), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.count, 0, sizeof(uint32_t) * n_tiles, stream)) != hipSuccess) return e;
    const uint32_t obj_blocks = (a.n_objs + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(tile_rects, dim3(obj_blocks), dim3(kBlock), 0, stream, a, b);
    return launch_tile_list_count(a, b, stream);
}

hipError_t launch_pose_spheres(const PoseSphereArgs& a, const double* bounds, const double* spheres, double* out, hipStream_t stream) {
    if (a.n_objs == 0 || !bounds || !spheres || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_spheres, dim3((a.n_objs + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, bounds, spheres, out);
    return hipGetLastError();
}

hipError_t launch_tile_list_count(const PoseTileArgs& a, const PoseTileBuffers& b, hipStream_t stream) {
    const uint32_t n_tiles = a.tiles_x * a.tiles_y;
    if (a.n_objs == 0 || n_tiles == 0 || n_tiles > kPoseMaxTiles) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_expand<false>, dim3((a.n_objs + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, b, 0u);
    return launch_tile_scan(b, n_tiles, stream);
}

hipError_t launch_tile_scan(const PoseTileBuffers& b, uint32_t n_tiles, hipStream_t stream) {
    if (n_tiles == 0 || n_tiles > kPoseMaxTiles) return hipErrorInvalidValue;
    const uint32_t scan_blocks = (n_tiles + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(tile_scan_sums, dim3(scan_blocks), dim3(kBlock), 0, stream, b, n_tiles);
    hipLaunchKernelGGL(tile_scan_top, dim3(1), dim3(kBlock), 0, stream, b, scan_blocks);
    hipLaunchKernelGGL(tile_scan_add, dim3(scan_blocks), dim3(kBlock), 0, stream, b, n_tiles);
    return hipGetLastError();
}

hipError_t launch_pose_tile_fill(const PoseTileArgs& a, const PoseTileBuffers& b, uint32_t total, uint32_t n_global, uint32_t max_list,
                                 hipStream_t stream) {
    const uint32_t n_tiles = a.tiles_x * a.tiles_y;
    if (a.n_objs == 0 || n_tiles == 0 || n_tiles > kPoseMaxTiles || n_global > kPoseMaxGlobal || max_list > kPoseMaxList) return hipErrorInvalidValue;
    const uint32_t obj_blocks = (a.n_objs + kBlock - 1) / kBlock;
    if (total) hipLaunchKernelGGL(tile_expand<true>, dim3(obj_blocks), dim3(kBlock), 0, stream, a, b, total);
    hipLaunchKernelGGL(tile_sort_wave, dim3((n_tiles + 1u + kBlock / 64u - 1u) / (kBlock / 64u)), dim3(kBlock), 0, stream, b, n_tiles, total, n_global);
    if (max_list > 64u) hipLaunchKernelGGL(tile_sort_block, dim3(n_tiles), dim3(kBlock), 0, stream, b, total);
    return hipGetLastError();
}

}  // namespace rt
