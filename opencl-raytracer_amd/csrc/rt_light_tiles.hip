// rt_light_tiles.hip - the light tiles of rt_grid.h's LightTiles, built where the objects are: rt_light_setup.cpp's build_light_tiles
// restated for the device, block form only (light_tiles.py is the executable definition, rt_grid.h has the margins).
//
// Passes on one stream, none of which waits on another workgroup (ordering is the stream's); the host synchronises four times:
//   lt_reduce        one lane per object, in double: |c| + r, |c - L| + r and, for the six (axis, sign) pairs, sg (c - L)[a] - r,
//                    reduced per wave and then with one integer atomic per wave on order-preserving keys       -> synchronise 1:
//                    the host forms kPad and picks the projection axis by the host builder's rule
//   lt_spans         per object the padded tangent spans in u and v (the host's span(): 1.5533 rad limit, 1e-5 (1 + |x|) padding),
//                    the no-tangent flag, the key, the lattice centre and the exact block-form radius wq; the bounds U0 U1 V0 V1,
//                    rmax and kmax by the same keyed atomics
//   lt_pair_totals   a second launch, because the tile origin and inverse step are not known inside lt_spans: it reads the bounds
//                    from the record and counts the (object, tile) pairs of EVERY candidate T of the halving rule at once
//                                                                                                                -> synchronise 2:
//                    the host chooses T, the tile origin and steps, the 8-bit steps, and refuses what the host builder refuses
//   lt_tile_rects    tile rectangles at the chosen T; then the list builder shared with the pose tiles (rt_tiles.h:
//                    launch_tile_list_count): count expansion and exclusive scan
//   lt_chain_count   further blocks per tile (len > 3 ? (len - 1) / 3 : 0), scanned by the shared scan                -> synchronise 3:
//                    the host reads total, longest list and block count, refuses or grows the arrays
//   fill + rank sort the shared launch_pose_tile_fill: per tile by (key, index), a total order, so two builds are the same bytes
//   lt_pack          per object {x16 | y16 << 16, z16 | r8 << 16 | k8 << 24}: r8 rounded UP until r8 rstep >= wq, k8 rounded DOWN
//                    until k8 kstep <= key, with the device's own fp32 products
//   lt_write_blocks  one lane per tile: its head (block t) and its chain behind the heads, every slot of every block written
//                                                                                                                -> synchronise 4
// Every loop is bounded by a rectangle's area, a list's length or a constant; every store is guarded by the size of its array.
#include "rt_light_tiles.h"

namespace rt {
namespace {

constexpr uint32_t kBlock = 256;

__device__ __forceinline__ float lt_float_below(float f) {  // nextafterf(f, -inf)
    if (!(f == f) || f == -__builtin_inff()) return f;
    if (f == 0.f) return -1.401298464e-45f;
    const uint32_t b = __float_as_uint(f);
    return __uint_as_float(f > 0.f ? b - 1u : b + 1u);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ bool usable(double r) { return r >= 0 && r != __builtin_inf(); }

__global__ __launch_bounds__(kBlock) void lt_reduce(const LightTileArgs a, const LightTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long lowest = lt_key_of(-__builtin_inf()), highest = lt_key_of(__builtin_inf());
    unsigned long long coord = lowest, reach = lowest, clear[6] = {highest, highest, highest, highest, highest, highest};
    if (i < a.n_objs) {
        const double c[3] = {b.spheres[4ull * i], b.spheres[4ull * i + 1], b.spheres[4ull * i + 2]}, r = b.spheres[4ull * i + 3];
        if (usable(r)) {
            double cl = 0, dl = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cl += c[k] * c[k];
                dl += (c[k] - a.L[k]) * (c[k] - a.L[k]);
            }
            coord = lt_key_of(__builtin_sqrt(cl) + r);
            reach = lt_key_of(__builtin_sqrt(dl) + r);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                clear[2 * k] = lt_key_of(-(c[k] - a.L[k]) - r);
                clear[2 * k + 1] = lt_key_of((c[k] - a.L[k]) - r);
            }
        }
    }
    coord = wave_max(coord);
    reach = wave_max(reach);
#pragma unroll
    for (int k = 0; k < 6; ++k) clear[k] = wave_min(clear[k]);
    if ((threadIdx.x & 63u) == 0u) {
        atomicMax(&b.record->coord_max, coord);
        atomicMax(&b.record->reach_max, reach);
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicMin(&b.record->clear[k], clear[k]);
    }
}

// directions (x', z') through the origin that meet the disc (cx, cz; r), as x' / -z': tan of [phi - alpha, phi + alpha], padded
__device__ __forceinline__ bool span(double cx, double cz, double r, double& lo, double& hi) {
    const double rho = __builtin_sqrt(cx * cx + cz * cz);
    if (!(rho > r)) return false;
    const double q = r / rho;
    const double phi = atan2(cx, -cz), alpha = asin(q < 1.0 ? q : 1.0);
    if (!(__builtin_fabs(phi) + alpha < 1.5533)) return false;
    lo = tan(phi - alpha);
    hi = tan(phi + alpha);
    lo -= 1e-5 * (1.0 + __builtin_fabs(lo));
    hi += 1e-5 * (1.0 + __builtin_fabs(hi));
    return true;
}

__global__ __launch_bounds__(kBlock) void lt_spans(const LightTileArgs a, const LightTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long lowest = lt_key_of(-__builtin_inf()), highest = lt_key_of(__builtin_inf());
    unsigned long long U0 = highest, U1 = lowest, V0 = highest, V1 = lowest, rmax = lowest, kmax = lowest;
    uint32_t flags = 0, listed = 0;
    if (i < a.n_objs) {
        double4 sp = make_double4(1.0, -1.0, 1.0, -1.0);
        float key = 0.f;
        double wq = 0.0;
        uint2 pk = make_uint2(0u, 0u);
        const double c[3] = {b.spheres[4ull * i], b.spheres[4ull * i + 1], b.spheres[4ull * i + 2]}, r0 = b.spheres[4ull * i + 3];
        if (usable(r0)) {
            const double r = r0 + a.kPad;
            const double q[3] = {c[0] - a.L[0], c[1] - a.L[1], c[2] - a.L[2]};
            const double qx = a.ax == 0u ? q[0] : (a.ax == 1u ? q[1] : q[2]);
            const double qy = a.ay == 0u ? q[0] : (a.ay == 1u ? q[1] : q[2]);
            const double qz = a.sz * (a.az == 0u ? q[0] : (a.az == 1u ? q[1] : q[2]));
            double u0, u1, v0, v1;
            if (!span(qx, qz, r, u0, u1) || !span(qy, qz, r, v0, v1)) {
                flags |= kLtFlagNoTangent;
            } else if (u1 >= u0) {
                sp = make_double4(u0, u1, v0, v1);
                listed = 1u;
                const double d = __builtin_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - (r0 + a.kPad);
                key = lt_float_below((float)(d * (1.0 - 1e-6)));
                // the centre on the lattice, decoded with the device's own fma; the quantisation error goes into the radius
                double d2 = 0;
                uint32_t q16[3] = {0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double u = __builtin_floor((c[k] - (double)a.lat_lo[k]) / (double)a.lat_step + 0.5);
                    if (!(u >= 0.0) || !(u <= 65535.0)) { flags |= kLtFlagOffLattice; continue; }  // (a centre outside the grid box: the host refuses the blocks)
                    q16[k] = (uint32_t)u;
                    const double dec = (double)__builtin_fmaf((float)u, a.lat_step, a.lat_lo[k]);
                    d2 += (c[k] - dec) * (c[k] - dec);
                }
                const double w = __builtin_fabs((double)b.pre[i]), dq = __builtin_sqrt(d2), sa = __builtin_sqrt(a.alpha);
                const double w2 = (w + dq) * (w + dq) + 2.0 * dq * sa * a.Dbox + a.alpha * (2.0 * dq * a.Dbox + dq * dq);
                wq = __builtin_sqrt(w2) * (1.0 + 2e-6);
                pk = make_uint2(q16[0] | (q16[1] << 16), q16[2]);
                U0 = lt_key_of(u0); U1 = lt_key_of(u1); V0 = lt_key_of(v0); V1 = lt_key_of(v1);
                rmax = lt_key_of(wq);
                kmax = lt_key_of((double)key);
            }
        }
        b.span[i] = sp;
        b.lists.key[i] = key;
        b.wq[i] = wq;
        b.packed[i] = pk;
    }
    U0 = wave_min(U0); V0 = wave_min(V0);
    U1 = wave_max(U1); V1 = wave_max(V1);
    rmax = wave_max(rmax); kmax = wave_max(kmax);
    const unsigned long long n_listed = wave_sum((unsigned long long)listed);
    if (flags) atomicOr(&b.record->flags, flags);  // (rare: such a table is refused)
    if ((threadIdx.x & 63u) == 0u && n_listed != 0ull) {
        atomicMin(&b.record->U0, U0); atomicMax(&b.record->U1, U1);
        atomicMin(&b.record->V0, V0); atomicMax(&b.record->V1, V1);
        atomicMax(&b.record->rmax, rmax); atomicMax(&b.record->kmax, kmax);
        atomicAdd(&b.record->n_listed, (uint32_t)n_listed);
    }
}

// the tile range of a span: the fp32 expression the kernel evaluates, in double, with 0.01 tile of slack (the host's tile_span)
__device__ __forceinline__ bool tile_span(double lo, double hi, float base, float inv, uint32_t T, uint32_t& t0, uint32_t& t1) {
    const double x = __builtin_floor((lo - (double)base) * (double)inv - 0.01), y = __builtin_floor((hi - (double)base) * (double)inv + 0.01);
    const double top = (double)T - 1.0;
    const double x0 = x > 0.0 ? (x < top ? x : top) : 0.0;  // (a NaN keeps the table's edge)
    const double y0 = y > 0.0 ? (y < top ? y : top) : 0.0;
    t0 = (uint32_t)x0;
    t1 = (uint32_t)y0;
    return t0 <= t1;
}

__global__ __launch_bounds__(kBlock) void lt_pair_totals(const LightTileArgs a, const LightTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const double U0 = lt_unkey(b.record->U0), U1 = lt_unkey(b.record->U1), V0 = lt_unkey(b.record->V0), V1 = lt_unkey(b.record->V1);
    const bool bounds = U1 > U0 && V1 > V0 && ((U0 + U1 + V0 + V1) - (U0 + U1 + V0 + V1)) == 0.0;
    double4 sp = make_double4(1.0, -1.0, 1.0, -1.0);
    if (bounds && i < a.n_objs) sp = b.span[i];
    const bool listed = sp.y >= sp.x;
    const float u0f = lt_float_below((float)U0), v0f = lt_float_below((float)V0);
    for (uint32_t k = 0; k < kLtMaxCandidates; ++k) {
        if (k >= a.n_cand) break;  // (uniform)
        const uint32_t T = a.cand[k];
        unsigned long long pairs = 0ull;
        if (listed) {
            const double du = (U1 - U0) / (double)T * (1.0 + 1e-6), dv = (V1 - V0) / (double)T * (1.0 + 1e-6);
            const float inv_du = (float)(1.0 / du), inv_dv = (float)(1.0 / dv);
            uint32_t a0, a1, b0, b1;
            if (tile_span(sp.x, sp.y, u0f, inv_du, T, a0, a1) && tile_span(sp.z, sp.w, v0f, inv_dv, T, b0, b1))
                pairs = (unsigned long long)(a1 - a0 + 1u) * (b1 - b0 + 1u);
        }
        pairs = wave_sum(pairs);
        if ((threadIdx.x & 63u) == 0u && pairs != 0ull) atomicAdd(&b.record->pairs[k], pairs);
    }
}

__global__ __launch_bounds__(kBlock) void lt_tile_rects(const LightTileArgs a, const LightTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long pairs = 0ull;
    if (i < a.n_objs) {
        uint4 rc = make_uint4(1u, 0u, 1u, 0u);
        const double4 sp = b.span[i];
        uint32_t a0, a1, b0, b1;
        if (sp.y >= sp.x && tile_span(sp.x, sp.y, a.u0, a.inv_du, a.T, a0, a1) && tile_span(sp.z, sp.w, a.v0, a.inv_dv, a.T, b0, b1)) {
            rc = make_uint4(a0, a1, b0, b1);
            pairs = (unsigned long long)(a1 - a0 + 1u) * (b1 - b0 + 1u);
        }
        b.lists.rect[i] = rc;
    }
    pairs = wave_sum(pairs);
    if ((threadIdx.x & 63u) == 0u && pairs != 0ull) atomicAdd(&b.lists.record->pairs, pairs);
}

__global__ __launch_bounds__(kBlock) void lt_chain_count(const LightTileBuffers b, uint32_t n_tiles) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t len = b.lists.tile_start[t + 1u] - b.lists.tile_start[t];
    b.chains.count[t] = len > 3u ? (len - 1u) / 3u : 0u;
}

__global__ __launch_bounds__(kBlock) void lt_pack(const LightTileArgs a, const LightTileBuffers b) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_objs) return;
    const double4 sp = b.span[i];
    if (!(sp.y >= sp.x)) return;
    const double wq = b.wq[i], key = (double)b.lists.key[i];
    const double rq = __builtin_ceil(wq / (double)a.rstep);
    uint32_t r8 = rq >= 0.0 ? (rq < 255.0 ? (uint32_t)rq : 255u) : 0u;
    for (uint32_t k = 0; k < 255u && r8 < 255u && (double)((float)r8 * a.rstep) < wq; ++k) ++r8;  // (the kernels' own product must not fall short)
    const double kq = __builtin_floor((key > 0.0 ? key : 0.0) / (double)a.kstep * (1.0 - 1e-6));
    uint32_t k8 = kq >= 0.0 ? (kq < 255.0 ? (uint32_t)kq : 255u) : 0u;
    for (uint32_t k = 0; k < 255u && k8 > 0u && (double)((float)k8 * a.kstep) > key; ++k) --k8;  // (rounded DOWN: an entry may only look nearer to the light)
    for (uint32_t k = 0; k < 255u && k8 < 255u && (double)((float)(k8 + 1u) * a.kstep) <= key; ++k) ++k8;  // (... but by less than one step: the estimate's 1e-6 can cost one)
    uint2 pk = b.packed[i];
    pk.y = (pk.y & 0xffffu) | (r8 << 16) | (k8 << 24);
    b.packed[i] = pk;
}

__global__ __launch_bounds__(kBlock) void lt_write_blocks(const LightTileArgs a, const LightTileBuffers b, uint32_t heads, uint32_t total, uint32_t n_blocks) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= heads) return;
    const uint32_t e0 = b.lists.tile_start[t];
    uint32_t len = b.lists.tile_start[t + 1u] - e0;
    if (len > kLtMaxList) len = kLtMaxList;
    const uint32_t chain0 = heads + b.chains.tile_start[t];
    const uint32_t nb = 1u + (len > 3u ? (len - 1u) / 3u : 0u);
    const uint32_t empty_hi = 0xff000000u;
    for (uint32_t bi = 0; bi < nb; ++bi) {  // <= 342 blocks
        const uint32_t at = bi == 0u ? t : chain0 + bi - 1u;
        const uint32_t next = bi + 1u < nb ? chain0 + bi : 0u;
        uint32_t w[6], id[3];
#pragma unroll
        for (uint32_t s = 0; s < 3u; ++s) {
            const uint32_t j = 3u * bi + s;
            w[2 * s] = 0u; w[2 * s + 1] = empty_hi; id[s] = a.n_objs;
            if (j < len && e0 + j < total) {
                const uint32_t obj = b.lists.entries[e0 + j].x;
                if (obj < a.n_objs) {
                    const uint2 pk = b.packed[obj];
                    w[2 * s] = pk.x; w[2 * s + 1] = pk.y; id[s] = obj;
                }
            }
        }
        if (at < n_blocks) {
            b.blocks[2ull * at] = make_uint4(next, 0u, w[0], w[1]);
            b.blocks[2ull * at + 1] = make_uint4(w[2], w[3], w[4], w[5]);
            *reinterpret_cast<uint4*>(b.block_ids + 4ull * at) = make_uint4(id[0], id[1], id[2], a.n_objs);
        }
    }
}

}  // namespace

hipError_t launch_light_tile_reduce(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream) {
    if (a.n_objs == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lt_reduce, dim3((a.n_objs + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, b);
    return hipGetLastError();
}

hipError_t launch_light_tile_spans(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream) {
    if (a.n_objs == 0 || a.n_cand == 0 || a.n_cand > kLtMaxCandidates) return hipErrorInvalidValue;
    const uint32_t obj_blocks = (a.n_objs + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(lt_spans, dim3(obj_blocks), dim3(kBlock), 0, stream, a, b);
    hipLaunchKernelGGL(lt_pair_totals, dim3(obj_blocks), dim3(kBlock), 0, stream, a, b);
    return hipGetLastError();
}

hipError_t launch_light_tile_count(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream) {
    const uint64_t n_tiles64 = (uint64_t)a.T * a.T;
    if (a.n_objs == 0 || a.T == 0 || n_tiles64 > kPoseMaxTiles) return hipErrorInvalidValue;
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    hipError_t e;
    if ((e = hipMemsetAsync(b.lists.record, 0, sizeof(PoseTileRecord), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.chains.record, 0, sizeof(PoseTileRecord), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.lists.count, 0, sizeof(uint32_t) * n_tiles, stream)) != hipSuccess) return e;
    PoseTileArgs pa = {};
    pa.n_objs = a.n_objs;
    pa.tiles_x = pa.tiles_y = a.T;
    pa.budget = a.budget;
    hipLaunchKernelGGL(lt_tile_rects, dim3((a.n_objs + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, b);
    if ((e = launch_tile_list_count(pa, b.lists, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(lt_chain_count, dim3((n_tiles + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, n_tiles);
    return launch_tile_scan(b.chains, n_tiles, stream);
}

hipError_t launch_light_tile_fill(const LightTileArgs& a, const LightTileBuffers& b, uint32_t total, uint32_t max_list, uint32_t n_blocks,
                                  hipStream_t stream) {
    const uint64_t n_tiles64 = (uint64_t)a.T * a.T;
    if (a.n_objs == 0 || a.T == 0 || n_tiles64 > kPoseMaxTiles || max_list > kLtMaxList || n_blocks < n_tiles64) return hipErrorInvalidValue;
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    PoseTileArgs pa = {};
    pa.n_objs = a.n_objs;
    pa.tiles_x = pa.tiles_y = a.T;
    pa.budget = a.budget;
    hipError_t e;
    if ((e = launch_pose_tile_fill(pa, b.lists, total, 0u, max_list, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(lt_pack, dim3((a.n_objs + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, b);
    hipLaunchKernelGGL(lt_write_blocks, dim3((n_tiles + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, b, n_tiles, total, n_blocks);
    return hipGetLastError();
}

}  // namespace rt
