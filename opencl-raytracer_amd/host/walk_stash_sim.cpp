// The block walk's loop without the walk (tests/test_walk_stash_cpu.py): the wave-uniform bookkeeping of
// ../csrc/rt_walk_stash.h driven on the host exactly as block_segment (../csrc/rt_wavefront.hip) drives it - prepare, take,
// draw another run, end - with lanes that finish their rays at random times. No GPU, no HIP headers.
//
//   walk_stash_sim <n_queue> <run> <refill_min> <n_waves> <no_start_every> <max_trips> <seed> <max_steps> <out.bin>
//
// The queue is cut in runs of <run> entries; with more runs than waves they are drawn from one ticket counter (RunCursor of
// rt_wavefront.hip, one region), else wave i has run i. The waves take turns, one pass of the loop each. Every
// <no_start_every>-th queue entry (0: none) is a slot that starts no walk. <out.bin> receives one record of four uint32 per
// hand-out, in the order they happen: queue entry, wave, the wave's pass, lane. stdout: one line of totals.
// Exit status 3: a wave was still looping after <max_steps> passes (the hang this program exists to catch); 4: the stash
// broke one of its own bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../csrc/rt_walk_stash.h"

namespace {
struct Cursor {  // RunCursor without regions
    uint32_t seg, n_runs, next = 0, seg_end = 0;
    bool dynamic;
    bool grab(uint32_t n_queue, uint32_t& ticket) {
        const uint32_t r = ticket++;
        if (r >= n_runs) return false;
        next = r * seg;
        seg_end = (n_queue - next < seg) ? n_queue : next + seg;
        return true;
    }
    bool begin(uint32_t n_queue, uint32_t run, uint32_t wave, uint32_t n_waves, uint32_t& ticket) {
        seg = run;
        n_runs = (n_queue + seg - 1u) / seg;
        dynamic = n_runs > n_waves;
        if (dynamic) return grab(n_queue, ticket);
        if (wave >= n_runs) return false;
        next = wave * seg;
        seg_end = (n_queue - next < seg) ? n_queue : next + seg;
        return true;
    }
};
struct Wave {
    Cursor rc;
    WalkStash sh;
    bool running = false, more = false;
    uint32_t steps = 0;
    uint32_t slot_entry[kStashSlots];
    bool slot_starts[kStashSlots];
    uint32_t trips_left[64] = {};  // 0: the lane is idle
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s n_queue run refill_min n_waves no_start_every max_trips seed max_steps out.bin\n", argv[0]);
        return 2;
    }
    const uint32_t n_queue = (uint32_t)std::strtoul(argv[1], nullptr, 10), run = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const uint32_t refill_min = (uint32_t)std::strtoul(argv[3], nullptr, 10), n_waves = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const uint32_t no_start_every = (uint32_t)std::strtoul(argv[5], nullptr, 10), max_trips = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const uint32_t seed = (uint32_t)std::strtoul(argv[7], nullptr, 10), max_steps = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    if (run == 0u || n_waves == 0u || max_trips == 0u) return 2;
    std::mt19937 rng(seed);
    std::vector<uint32_t> log;
    std::vector<Wave> waves(n_waves);
    uint32_t ticket = 0, max_stash = 0, prepares = 0, takes = 0;
    unsigned long long total_steps = 0;
    if (n_queue != 0u)  // (wf_walk_blocks returns before the loop on an empty queue)
        for (uint32_t i = 0; i < n_waves; ++i) {
            waves[i].running = waves[i].rc.begin(n_queue, run, i, n_waves, ticket);
            waves[i].more = waves[i].rc.dynamic;
        }
    for (bool any = true; any;) {
        any = false;
        for (uint32_t wi = 0; wi < n_waves; ++wi) {
            Wave& v = waves[wi];
            if (!v.running) continue;
            any = true;
            if (++v.steps > max_steps) {
                std::printf("wave %u still looping after %u passes: stash %u+%u next %u seg_end %u\n", wi, max_steps, v.sh.head, v.sh.count, v.rc.next, v.rc.seg_end);
                return 3;
            }
            ++total_steps;
            // ---- one pass of block_segment's loop ----
            uint32_t n_idle = 0;
            for (uint32_t l = 0; l < 64u; ++l) n_idle += v.trips_left[l] == 0u;
            const uint32_t n_prep = v.sh.to_prepare(n_idle, refill_min, v.rc.next, v.rc.seg_end);
            if (n_prep != 0u) {
                ++prepares;
                if (n_prep > kStashSlots || v.rc.next + n_prep > v.rc.seg_end) return 4;
                for (uint32_t j = 0; j < n_prep; ++j) {
                    v.slot_entry[j] = v.rc.next + j;
                    v.slot_starts[j] = !(no_start_every != 0u && (v.rc.next + j) % no_start_every == no_start_every - 1u);
                }
                v.rc.next = v.sh.prepared(n_prep, v.rc.next);
                if (WalkStash::run_used_up(v.rc.next, v.rc.seg_end, v.more)) v.more = v.rc.grab(n_queue, ticket);
            }
            if (v.sh.head + v.sh.count > kStashSlots) return 4;
            if (v.sh.count > max_stash) max_stash = v.sh.count;
            const uint32_t n_take = v.sh.to_take(n_idle, refill_min);
            if (n_take != 0u) {
                ++takes;
                uint32_t rank = 0;
                for (uint32_t l = 0; l < 64u && rank < n_take; ++l) {
                    if (v.trips_left[l] != 0u) continue;
                    const uint32_t slot = v.sh.take_from() + rank++;
                    if (slot >= kStashSlots) return 4;
                    const uint32_t rec[4] = {v.slot_entry[slot], wi, v.steps, l};
                    log.insert(log.end(), rec, rec + 4);
                    if (v.slot_starts[slot]) v.trips_left[l] = 1u + rng() % max_trips;
                }
                v.sh.taken(n_take);
            }
            uint32_t n_live = 0;
            for (uint32_t l = 0; l < 64u; ++l) n_live += v.trips_left[l] != 0u;
            if (n_live == 0u) {
                if (v.sh.finished(v.rc.next, v.rc.seg_end)) v.running = false;
                continue;
            }
            for (uint32_t l = 0; l < 64u; ++l)  // a trip
                if (v.trips_left[l] != 0u) --v.trips_left[l];
        }
    }
    std::FILE* f = std::fopen(argv[9], "wb");
    if (!f) return 2;
    if (!log.empty() && std::fwrite(log.data(), sizeof(uint32_t), log.size(), f) != log.size()) return 2;
    std::fclose(f);
    uint32_t longest = 0;
    for (const Wave& v : waves) longest = v.steps > longest ? v.steps : longest;
    std::printf("handed %zu prepares %u takes %u max_stash %u passes %llu longest_wave %u\n", log.size() / 4, prepares, takes, max_stash, total_steps, longest);
    return 0;
}
