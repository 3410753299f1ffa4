// The block walk's stash of prepared rays: the wave-uniform bookkeeping (rt_wavefront.hip: block_segment).
//
// A ray's set-up (queue entry, ray, walk_begin, first cell, slack) depends on nothing but the queue entry, yet at the moment
// lanes fall idle only ~18 of 64 want one. So the wave PREPARES up to 64 consecutive queue entries at once, all lanes taking
// part whatever they are walking, into a wave-private stash in LDS; idle lanes then TAKE their next ray from it, which is a
// copy. This header decides when to prepare, when to take, when to draw another run and when the wave's loop may end. It is
// plain integer arithmetic on wave-uniform values, compiled for the kernel and for the host (host/walk_stash_sim.cpp,
// tests/test_walk_stash_cpu.py): a mistake here is a wave that never ends.
//
// Order: slots are prepared in queue order and taken in slot order by the idle lanes in lane order - the order in which
// block_segment handed queue entries to lanes before there was a stash.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_STASH_HD __host__ __device__ __forceinline__
#else
#define RT_STASH_HD inline
#endif

constexpr uint32_t kStashSlots = 64u;  // one slot per lane of the preparing wave

struct WalkStash {
    uint32_t head = 0u, count = 0u;  // slots [head, head + count) hold prepared rays nobody has taken; head + count <= kStashSlots

    // lanes are given rays when enough of them idle to make it worth a round - or when nothing else is left to do
    static RT_STASH_HD bool refill(uint32_t n_idle, uint32_t refill_min) { return n_idle >= refill_min || n_idle == kStashSlots; }

    // how many queue entries to prepare now (0: none). Only into an empty stash, only while the run [next, seg_end) has entries.
    RT_STASH_HD uint32_t to_prepare(uint32_t n_idle, uint32_t refill_min, uint32_t next, uint32_t seg_end) const {
        if (count != 0u || next >= seg_end || !refill(n_idle, refill_min)) return 0u;
        const uint32_t left = seg_end - next;
        return left < kStashSlots ? left : kStashSlots;
    }
    // n entries [next, next + n) were written to slots 0 .. n-1; returns the new `next`
    RT_STASH_HD uint32_t prepared(uint32_t n, uint32_t next) {
        head = 0u;
        count = n;
        return next + n;
    }
    // after a prepare: is the run used up, so that another should be drawn (if any is left: `more`)?
    static RT_STASH_HD bool run_used_up(uint32_t next, uint32_t seg_end, bool more) { return next >= seg_end && more; }

    // how many slots the idle lanes take now (0: none): the idle lane of rank r < n reads slot head + r
    RT_STASH_HD uint32_t to_take(uint32_t n_idle, uint32_t refill_min) const {
        if (count == 0u || !refill(n_idle, refill_min)) return 0u;
        return n_idle < count ? n_idle : count;
    }
    RT_STASH_HD uint32_t take_from() const { return head; }
    RT_STASH_HD void taken(uint32_t n) {
        head += n;
        count -= n;
    }
    // with no live lane: may the loop end? Only when nothing is stashed and no entry of a run is left. (If not, all lanes
    // idle, refill() holds, and the next pass takes >= 1 slot or prepares >= 1 entry: the loop cannot idle.)
    RT_STASH_HD bool finished(uint32_t next, uint32_t seg_end) const { return count == 0u && next >= seg_end; }
};
