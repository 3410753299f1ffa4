"""CPU: the block walk's stash of prepared rays - its wave-uniform bookkeeping (csrc/rt_walk_stash.h: when to prepare, take,
draw another run, end) driven on the host by host/walk_stash_sim, which runs block_segment's loop without the walk: lanes
finish at random times (seeded), waves take turns, runs come from a ticket counter. A mistake here is a wave that never
ends on a GPU; here it is an exit status."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SIM = ROOT / "opencl-raytracer_amd" / "host" / "walk_stash_sim"

QUEUES = [0, 1, 63, 64, 65, 255, 256, 257, 33005]
MAX_TRIPS = 12


@pytest.fixture(scope="module")
def sim():
    if not SIM.exists():
        import __graft_entry__
        __graft_entry__.build()
    return SIM


def step_bound(n_queue):
    """Passes one wave can need for a queue of n entries, all of them its own. A pass with a live lane is a trip, and every trip
    uses up one of at most MAX_TRIPS trips of at least one ray: <= n * MAX_TRIPS such passes. A pass without a live lane either
    ends the loop or hands out work: it takes at least one slot (<= n such passes in all) or prepares at least one entry and then
    takes (counted already). One more for the pass that ends the loop, one for slack."""
    return n_queue * MAX_TRIPS + n_queue + 2


def run_sim(sim, tmp_path, n_queue, run, refill_min, n_waves, no_start_every, seed):
    out = tmp_path / "handed.bin"
    cmd = [str(sim), str(n_queue), str(run), str(refill_min), str(n_waves), str(no_start_every), str(MAX_TRIPS), str(seed),
           str(step_bound(n_queue)), str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, f"exit {res.returncode}: {res.stdout}{res.stderr}"
    words = dict(zip(res.stdout.split()[0::2], map(int, res.stdout.split()[1::2])))
    rec = np.fromfile(out, dtype=np.uint32).reshape(-1, 4)
    return rec, words


@pytest.mark.parametrize("refill_min", [1, 8, 16, 64])  # (8: the stash path's RT_WALK3_TAKE_MIN; 16: the mesh instances')
@pytest.mark.parametrize("run", [64, 256])
@pytest.mark.parametrize("n_queue", QUEUES)
def test_every_entry_is_handed_out_once_in_order_and_the_loop_ends(sim, tmp_path, n_queue, run, refill_min):
    for n_waves, no_start_every in ((1, 0), (3, 8), (7, 3), (700, 8)):  # (700 waves: more waves than runs - wave i has run i, most have none)
        rec, words = run_sim(sim, tmp_path, n_queue, run, refill_min, n_waves, no_start_every, seed=n_queue * 7 + run + refill_min)
        entry, wave, step, lane = rec.T if len(rec) else (np.zeros(0, np.uint32),) * 4
        # exactly once
        assert len(entry) == n_queue == words["handed"]
        assert np.array_equal(np.sort(entry), np.arange(n_queue, dtype=np.uint32))
        # the stash never holds more than a wave's 64 rays; the loop ended inside the bound (the simulator fails beyond it)
        assert words["max_stash"] <= 64
        assert words["longest_wave"] <= step_bound(n_queue)
        # a run is one wave's, and its entries reach lanes in queue order: later entries at later passes, and within a pass
        # ascending with the lane (the idle lane of rank r reads slot head + r)
        runs = entry // run
        for r in np.unique(runs):
            m = runs == r
            assert len(np.unique(wave[m])) == 1
            e, s, l = entry[m], step[m].astype(np.int64), lane[m].astype(np.int64)
            assert np.array_equal(e, np.sort(e)), "the log is in hand-out order: a run's entries must ascend in it"
            key = s * 64 + l
            assert np.all(np.diff(key) > 0)
        assert np.all(lane < 64)


def test_a_wave_that_never_ends_is_reported_not_waited_for(sim, tmp_path):
    """The simulator's own guard: with a bound too small for the queue it stops with exit status 3 instead of looping."""
    res = subprocess.run([str(sim), "257", "64", "16", "1", "0", str(MAX_TRIPS), "1", "3", str(tmp_path / "o.bin")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 3 and "still looping" in res.stdout
