// rt_ao_filter.h - launch interface of the filtered-ambient-occlusion pass (rt_ao_filter.hip): an edge-aware box blur of the AO pass's
// counts over a (2r + 1)^2 window of a row-major array (hip_raytracer.h, "filtered ambient occlusion"; ao.py: filter() is the
// executable definition).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

// Inputs of one pass, device pointers: width * rows items, row-major. unoccluded: bytes, any alignment. point / normal: float4, 16-byte
// aligned. index: null (every item may be live) or int32, 4-byte aligned. samples: 1, 2, 4 ... 64; radius: 1 .. 4.
struct AoFilterInputs {
    const uint8_t* unoccluded;
    const float4* point;
    const float4* normal;
    const int32_t* index;
    uint64_t width, rows;
    uint32_t samples, radius;
    float normal_min, plane_max;
};

// Outputs, device pointers: each may be null, not all. ao: floats, 4-byte aligned; grey and taps: bytes, any alignment.
struct AoFilterOutputs {
    float* ao;
    uint8_t* grey;
    uint8_t* taps;
};

// What a pass adds up, once per wave: the live items and the accepted taps (the sum of taps over all items). The counter block is
// kAoFilterCounterSlots such records of one 128-byte line each; a workgroup adds to slot blockIdx.x % kAoFilterCounterSlots and the
// reader sums the slots: 64-bit atomics of every wave on ONE address cost 11 ns each, 1.4 ms of a 1.6 ms pass over 16.8 M items.
struct AoFilterCounters {
    unsigned long long n_live, accepted;
    unsigned long long line[14];  // (to 128 bytes)
};
constexpr uint32_t kAoFilterCounterSlots = 64;

// d_counters: kAoFilterCounterSlots records, zeroed. One workgroup of 256 lanes per tile of 64 columns x 16 rows (workgroups loop over the tiles); width * rows == 0 launches nothing.
hipError_t launch_ao_filter(const AoFilterInputs& in, const AoFilterOutputs& out, AoFilterCounters* d_counters, hipStream_t stream);

}  // namespace rt
