// rt_light_tiles.h - host-side launchers of the light-tile builder (rt_light_tiles.hip): the per-direction candidate lists of
// rt_grid.h's LightTiles for the shadow rays towards one positional light, built on the device from the objects' registration
// spheres, in the block form. rt_light_setup.cpp's build_light_tiles is the host builder it restates; opencl-raytracer_amd/light_tiles.py
// is the executable definition.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rt_tiles.h"

namespace rt {

constexpr uint32_t kLtMaxCandidates = 7;     // tile counts of the halving rule: T0, T0 / 2, ... down to 16
constexpr uint32_t kLtMaxList = kPoseMaxList;  // entries of one tile: what one workgroup sorts in 8 KB of LDS
constexpr uint32_t kLtFlagNoTangent = 1u;    // LightTileRecord::flags: an object without a usable tangent
constexpr uint32_t kLtFlagOffLattice = 2u;   // ... a centre outside the 16-bit lattice (no block form)

// What the passes need besides an object's own sphere. The host fills it in stages: the light for the reduction; kPad, the frame
// and the lattice for the spans; the candidates for the pair totals; the chosen T, the tile origin and the 8-bit steps for the rest.
struct LightTileArgs {
    double L[3];                // the light, converted exactly
    double kPad;
    double sz;                  // z' = sz (p - L)[az]
    uint32_t ax, ay, az;
    uint32_t n_objs;
    float lat_lo[3], lat_step;  // the 16-bit lattice over the grid box
    double Dbox, alpha;         // the grid box's diagonal and the pre-test's distance term
    uint32_t n_cand, cand[kLtMaxCandidates];
    uint32_t T;                 // the chosen tile count per axis
    float u0, v0, inv_du, inv_dv;
    float rstep, kstep;
    unsigned long long budget;  // (object, tile) pairs the table may hold
};

// Monotone map of a double onto an unsigned 64-bit key (and back), so that integer atomic min / max reduce doubles of either sign.
__host__ __device__ inline unsigned long long lt_key_of(double d) {
    unsigned long long b;
    __builtin_memcpy(&b, &d, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double lt_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}

// What the host reads back (all doubles as lt_key_of keys).
struct LightTileRecord {
    unsigned long long coord_max, reach_max;   // max: |c| + r, |c - L| + r
    unsigned long long clear[6];               // min of sg (c - L)[a] - r, index 2 a + (sg > 0)
    unsigned long long U0, U1, V0, V1;         // min / max of the padded spans
    unsigned long long rmax, kmax;             // max of the block-form radius and of the key
    unsigned long long pairs[kLtMaxCandidates];  // (object, tile) pairs at every candidate T (plain counts)
    uint32_t flags, n_listed;
};

// Device memory of the builder, owned by the context (grow-only). `lists` is the shared list builder's (rt_tiles.h): its rect / key /
// count / cursor / sums / record / scratch / tile_start / entries arrays serve the count, scan, fill and rank-sort.
struct LightTileBuffers {
    const double* spheres;      // 4 doubles per object: centre, registration radius
    const float* pre;           // per object: the pre-test radius as the grid's entry spheres carry it
    double4* span;              // per object: u0, u1, v0, v1 (u1 < u0: in no list)
    double* wq;                 // per object: the exact block-form radius
    uint2* packed;              // per object: the two words of its block entries
    LightTileRecord* record;
    PoseTileBuffers lists;
    PoseTileBuffers chains;     // count = chain blocks per tile, tile_start = chain_at (tiles + 1), record->total = their sum
    uint4* blocks;              // 2 x uint4 per block
    uint32_t* block_ids;        // 4 per block
};

// Pass 1: the reduction (record zeroed to the identities first). The host reads the record: synchronise 1.
hipError_t launch_light_tile_reduce(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream);
// Pass 2, two launches: spans / keys / radii and their reductions, then - the bounds now in the record - the pair totals of every
// candidate T. The host reads the record: synchronise 2.
hipError_t launch_light_tile_spans(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream);
// Pass 3, first half: tile rectangles at the chosen T, count, scan, chain blocks per tile and their scan. The host reads the two
// list records (total, longest list, chain blocks): synchronise 3.
hipError_t launch_light_tile_count(const LightTileArgs& a, const LightTileBuffers& b, hipStream_t stream);
// Pass 3, second half, and pass 4: fill, rank sort, pack, heads and chains. `total`, `max_list` and `n_blocks` are the records',
// accepted by the host (scratch holds total, entries total + 1, blocks n_blocks elements). The caller synchronises: 4.
hipError_t launch_light_tile_fill(const LightTileArgs& a, const LightTileBuffers& b, uint32_t total, uint32_t max_list, uint32_t n_blocks,
                                  hipStream_t stream);

}  // namespace rt
