// rt_ao_filter.hip - filtered ambient occlusion (hip_raytracer.h): an edge-aware box blur of the AO pass's counts, one launch.
//
// The library's first neighbourhood kernel. A workgroup of 256 lanes owns a tile of 64 columns x 16 rows and stages the tile plus a halo
// of R cells on every side in LDS as seven planes of (64 + 2R) x (16 + 2R) words: px, py, pz, nx, ny, nz and one word that holds the
// count in bits 0 .. 7 and the live bit in bit 8. A cell outside the array is staged dead and nothing outside the array is read. The
// staging hands consecutive lanes consecutive cells of a row, so the float4 loads of point and normal coalesce and the plane stores
// fall on consecutive banks; a lane issues the loads of all its 5 .. 7 cells before it waits for the first (a loop that loads, waits
// and stores cell by cell makes three dependent trips to memory per cell; DESIGN.md section 6 has both forms' times). R = 4 takes
// 72 x 24 x 28 = 48 384 bytes (three workgroups per CU of 160 KiB), R = 1 33 264.
//
// Then lane l of wave w keeps the FOUR centres of column l, rows 4w .. 4w + 3 in registers and walks its window column by column: per
// window column it reads the 4 + 2R cells of rows 4w - R .. 4w + 3 + R once and tests each against the centres it lies in the window
// of - 7 (4 + 2R) (2R + 1) words per four items instead of 7 (2R + 1)^2 per item, a third of the LDS reads at R = 4. A wave reads 64
// consecutive words of a row per plane: every ds_read is conflict-free whatever the row pitch. The radius is a template parameter
// (rows and centres unrolled, the column loop kept: the unrolled body of R = 4 would not fit the instruction cache).
//
// The tests are ao.py's: fp32, product then sum, nothing contracted in this unit in any arithmetic mode; a comparison with a NaN is
// false; the centre accepts itself untested. Weights are 0 or 1 and the sums integers, so the order of the walk is free. The division
// is the correctly rounded one (__fdiv_rn), the byte the table of "8-bit frames" (rt_pack.hip's quantise). Counters: live items and
// accepted taps, added up per lane, reduced per wave with shuffles, one atomic pair per wave into one of 64 slots on lines of their own.
#include "rt_ao_filter.h"

namespace rt {
namespace {

constexpr int kTileW = 64, kTileH = 16, kLaneRows = 4;
constexpr uint32_t kFilterBlock = 256;
constexpr uint64_t kFilterMaxBlocks = 1ull << 20;
constexpr uint32_t kLiveBit = 0x100u;

__device__ __forceinline__ bool finite_(float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // (NaN: false)

__device__ __forceinline__ uint32_t quantise(float v) {  // rt_pack.hip's: NaN and negatives 0, from 255 up 255
    const float f = floorf(v * 255.0f);
    return (uint32_t)fminf(fmaxf(f, 0.0f), 255.0f);
}

template <int R>
__global__ __launch_bounds__(kFilterBlock) void ao_filter(const AoFilterInputs in, const uint64_t tiles_x, const uint64_t n_tiles,
                                                          float* __restrict__ ao, uint8_t* __restrict__ grey, uint8_t* __restrict__ taps_out,
                                                          AoFilterCounters* __restrict__ counters) {
    constexpr int LW = kTileW + 2 * R, LH = kTileH + 2 * R, CELLS = LW * LH;
    constexpr int STEPS = (CELLS + (int)kFilterBlock - 1) / (int)kFilterBlock;   // cells a lane stages: 5 (R = 1) .. 7 (R = 4)
    __shared__ float planes[6 * CELLS];
    __shared__ uint32_t words[CELLS];
    float* const s_px = planes;
    float* const s_py = planes + CELLS;
    float* const s_pz = planes + 2 * CELLS;
    float* const s_nx = planes + 3 * CELLS;
    float* const s_ny = planes + 4 * CELLS;
    float* const s_nz = planes + 5 * CELLS;

    const int lx = (int)(threadIdx.x & 63u);
    const int ry = (int)(threadIdx.x >> 6) * kLaneRows;
    const float normal_min = in.normal_min, plane_max = in.plane_max;
    unsigned long long n_live = 0, accepted = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int64_t col0 = (int64_t)(tile_x * kTileW) - R, row0 = (int64_t)(tile_y * kTileH) - R;
        __syncthreads();  // (the previous tile's window reads have ended)
        // every load of the lane's STEPS cells is issued before the first is waited for: one trip to memory per tile, not one per
        // cell and array. A cell outside the array (or beyond CELLS) reads item 0 - inside the array - and is staged dead.
        uint64_t item[STEPS];
        bool inside[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int cell = (int)threadIdx.x + s * (int)kFilterBlock;
            const int cy = cell / LW, cx = cell - cy * LW;
            const int64_t col = col0 + cx, row = row0 + cy;
            inside[s] = cell < CELLS && col >= 0 && row >= 0 && (uint64_t)col < in.width && (uint64_t)row < in.rows;
            item[s] = inside[s] ? (uint64_t)row * in.width + (uint64_t)col : 0ull;
        }
        float4 p[STEPS], n[STEPS];
        int32_t object[STEPS];
        uint32_t count[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            p[s] = in.point[item[s]];
            n[s] = in.normal[item[s]];
            count[s] = in.unoccluded[item[s]];
            object[s] = 0;
        }
        if (in.index) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) object[s] = in.index[item[s]];
        }
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int cell = (int)threadIdx.x + s * (int)kFilterBlock;
            const bool live = inside[s] && object[s] >= 0 && finite_(p[s].x) && finite_(p[s].y) && finite_(p[s].z) && finite_(n[s].x) &&
                              finite_(n[s].y) && finite_(n[s].z);
            if (cell < CELLS) {
                s_px[cell] = p[s].x; s_py[cell] = p[s].y; s_pz[cell] = p[s].z;
                s_nx[cell] = n[s].x; s_ny[cell] = n[s].y; s_nz[cell] = n[s].z;
                words[cell] = inside[s] ? (count[s] | (live ? kLiveBit : 0u)) : 0u;
            }
        }
        __syncthreads();

        float cpx[kLaneRows], cpy[kLaneRows], cpz[kLaneRows], cnx[kLaneRows], cny[kLaneRows], cnz[kLaneRows];
        uint32_t sum[kLaneRows], taps[kLaneRows];
        bool live_p[kLaneRows];
#pragma unroll
        for (int c = 0; c < kLaneRows; ++c) {
            const int cell = (ry + c + R) * LW + lx + R;
            const uint32_t word = words[cell];
            live_p[c] = (word & kLiveBit) != 0u;
            cpx[c] = s_px[cell]; cpy[c] = s_py[cell]; cpz[c] = s_pz[cell];
            cnx[c] = s_nx[cell]; cny[c] = s_ny[cell]; cnz[c] = s_nz[cell];
            sum[c] = live_p[c] ? (word & 0xFFu) : 0u;  // a live centre accepts itself, untested
            taps[c] = live_p[c] ? 1u : 0u;
        }
#pragma unroll 1
        for (int dx = -R; dx <= R; ++dx) {
            const int column = lx + R + dx;
#pragma unroll
            for (int j = 0; j < kLaneRows + 2 * R; ++j) {
                const int cell = (ry + j) * LW + column;
                const uint32_t word = words[cell];
                const bool live_q = (word & kLiveBit) != 0u;
                const float qpx = s_px[cell], qpy = s_py[cell], qpz = s_pz[cell];
                const float qnx = s_nx[cell], qny = s_ny[cell], qnz = s_nz[cell];
#pragma unroll
                for (int c = 0; c < kLaneRows; ++c) {
                    const int dy = j - R - c;  // compile-time after unrolling
                    if (dy < -R || dy > R) continue;
                    const float cosine = (cnx[c] * qnx + cny[c] * qny) + cnz[c] * qnz;
                    const float ddx = qpx - cpx[c], ddy = qpy - cpy[c], ddz = qpz - cpz[c];
                    const float e = (cnx[c] * ddx + cny[c] * ddy) + cnz[c] * ddz;
                    bool ok = live_p[c] && live_q && cosine >= normal_min && __builtin_fabsf(e) <= plane_max;  // (a NaN: false)
                    if (dy == 0) ok = ok && dx != 0;  // the centre itself is counted above
                    taps[c] += ok ? 1u : 0u;
                    sum[c] += ok ? (word & 0xFFu) : 0u;
                }
            }
        }

        const uint64_t col = tile_x * kTileW + (uint64_t)lx;
        if (col < in.width) {
#pragma unroll
            for (int c = 0; c < kLaneRows; ++c) {
                const uint64_t row = tile_y * kTileH + (uint64_t)(ry + c);
                if (row >= in.rows) continue;
                const uint64_t i = row * in.width + col;
                const float a = live_p[c] ? __fdiv_rn((float)sum[c], (float)(taps[c] * in.samples)) : 1.0f;  // a dead item: taps 0, ao 1
                if (ao) ao[i] = a;
                if (grey) grey[i] = (uint8_t)quantise(a);
                if (taps_out) taps_out[i] = (uint8_t)taps[c];
                n_live += live_p[c] ? 1ull : 0ull;
                accepted += taps[c];
            }
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_live += __shfl_xor(n_live, off);
        accepted += __shfl_xor(accepted, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        AoFilterCounters* const slot = counters + (blockIdx.x % kAoFilterCounterSlots);  // (one address for all waves serialises them)
        if (n_live) atomicAdd(&slot->n_live, n_live);
        if (accepted) atomicAdd(&slot->accepted, accepted);
    }
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0; }

}  // namespace

hipError_t launch_ao_filter(const AoFilterInputs& in, const AoFilterOutputs& out, AoFilterCounters* d_counters, hipStream_t stream) {
    if (in.width == 0 || in.rows == 0) return hipSuccess;
    if (!in.unoccluded || !in.point || !in.normal || misaligned(in.point, 16) || misaligned(in.normal, 16) || misaligned(in.index, 4) ||
        (!out.ao && !out.grey && !out.taps) || misaligned(out.ao, 4) || !d_counters || in.samples == 0 || in.samples > 64 ||
        (in.samples & (in.samples - 1u)) || in.rows > (~0ull) / in.width)
        return hipErrorInvalidValue;
    const uint64_t tiles_x = (in.width + kTileW - 1) / kTileW, tiles_y = (in.rows + kTileH - 1) / kTileH;
    if (tiles_y > (~0ull) / tiles_x) return hipErrorInvalidValue;
    const uint64_t n_tiles = tiles_x * tiles_y;
    const dim3 blocks((uint32_t)(n_tiles < kFilterMaxBlocks ? n_tiles : kFilterMaxBlocks));
#define RT_AO_FILTER_LAUNCH(R)                                                                                                     \
    hipLaunchKernelGGL((ao_filter<R>), blocks, dim3(kFilterBlock), 0, stream, in, tiles_x, n_tiles, out.ao, out.grey, out.taps, d_counters)
    switch (in.radius) {
        case 1: RT_AO_FILTER_LAUNCH(1); break;
        case 2: RT_AO_FILTER_LAUNCH(2); break;
        case 3: RT_AO_FILTER_LAUNCH(3); break;
        case 4: RT_AO_FILTER_LAUNCH(4); break;
        default: return hipErrorInvalidValue;
    }
#undef RT_AO_FILTER_LAUNCH
    return hipGetLastError();
}

}  // namespace rt
