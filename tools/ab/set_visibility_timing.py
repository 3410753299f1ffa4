#!/usr/bin/env python3
"""Replaceable visibility (hip_raytracer.h) on one workload (cfg4: 100 k spheres, 32 lights, 4096^2, depth 3), ONE process, warmed,
the routes alternating round by round, a new mask every round:

(a) rt_set_visibility (a host mask) and rt_set_visibility_device (a torch bool tensor) on a live context, for ALL objects and for
    ONE: wall of the whole call, and the device time of the upload and of the patch kernel (csrc/rt_visibility.hip) from the event
    pairs RT_VISIBILITY_TRACE=1 makes the library record and print on stderr;
(b) a FRESH context created with records.with_visibility(objects, mask) in the same process - what a caller pays today: the
    wall of constructing it and create_ms of rt_get_setup_times;
(c) the frame's kernel time on the live context before any call (its own repeated frames: the spread), behind masks that hide
    0 %, 50 % and 99 % of the objects, and on the fresh context created with the same records. No table is rebuilt by the call, so
    the live frame still tests the hidden objects' registrations: live / fresh is the argument for or against a later rebuild.
With --parent-lib PATH (a library built from the parent commit) the untouched frame is also measured in child processes that
alternate between that library and this one (RT_LIB_OVERRIDE), three pairs: no kernel of the frame changed, so the two must agree
within the spread. Walls are host clocks around calls that end in a device synchronise; every figure is given as best / median /
max and all rounds.
usage: python tools/ab/set_visibility_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
import json, os, re, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera, records as R  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402

argv = sys.argv[1:]
parent_lib = None
if "--parent-lib" in argv:
    k = argv.index("--parent-lib")
    parent_lib = os.path.abspath(argv[k + 1])
    del argv[k:k + 2]
frame_only = "--frame-only" in argv
if frame_only:
    argv.remove("--frame-only")
wl = argv[0] if len(argv) > 0 else "cfg4"
rounds = max(10, int(argv[1])) if len(argv) > 1 else 20
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "set_visibility_timing.json")
HIDDEN = (0, 50, 99)   # per cent of the objects


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def frame_kernel_ms(rt, d_frame, n=3):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return statistics.median(ms[1:])


def stderr_of(fn):
    """What the library prints on stderr (fd 2) during fn()."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n = W * H
z = float(camera.camera_z(H))
n_objs = len(objs)

if frame_only:   # a child of the --parent-lib comparison: the frame of whatever library RT_LIB_OVERRIDE names, one JSON line
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
    d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    frame_kernel_ms(rt, d_frame)
    ms = [frame_kernel_ms(rt, d_frame) for _ in range(rounds)]
    rt.close()
    print(json.dumps({"library_sha16": bench.library_sha16(), "frame_kernel_ms": summary(ms)}))
    sys.exit(0)


def mask_for(rnd, per_cent):
    """A new mask every round: `per_cent` of the objects hidden, picked by a generator seeded with the round."""
    rng = np.random.default_rng(1000 * rnd + per_cent)
    m = np.ones(n_objs, dtype=np.uint8)
    m[rng.permutation(n_objs)[:n_objs * per_cent // 100]] = 0
    return m


res = {"what": "rt_set_visibility / rt_set_visibility_device on a live context (all objects, one object) against a fresh context created with "
               "records.with_visibility; device time of the upload and of the patch kernel; kernel time of the frame before the first call, "
               "behind masks hiding 0 / 50 / 99 per cent on the live context and on the fresh context with the same records; one process, "
               "warmed, alternating round by round",
       "workload": desc, "frame": [W, H], "rays": n, "objects": n_objs, "mask_bytes": n_objs, "rounds": rounds,
       "library_sha16": bench.library_sha16(), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
frame_kernel_ms(live, d_frame)
untouched = [frame_kernel_ms(live, d_frame) for _ in range(rounds)]   # the context's own repeated frames: the spread every margin below is
res["frame_untouched_ms"] = summary(untouched)
os.environ["RT_VISIBILITY_TRACE"] = "1"
names = ("host_all", "host_one", "device_all", "device_one")
rows = {f"{k}_{what}": [] for k in names for what in ("wall_ms", "copy_device_ms", "patch_device_ms")}
rows.update({k: [] for k in ("fresh_wall_ms", "fresh_create_ms")})
rows.update({f"frame_{side}_hidden{p}_ms": [] for side in ("live", "fresh") for p in HIDDEN})
picked = n_objs // 2
equal = {}
for rnd in range(rounds + 1):   # round 0 warms up: the support arrays, the staging buffer, code objects
    half = mask_for(rnd, 50)
    one = np.array([rnd % 2], dtype=np.uint8)   # the object under the mouse: hidden in one round, shown in the next
    d_all = torch.from_numpy(half != 0).cuda()  # torch.bool
    d_one = torch.from_numpy(one != 0).cuda()
    torch.cuda.synchronize()
    calls = {"host_all": lambda: live.set_visibility(half), "host_one": lambda: live.set_visibility(one, picked),
             "device_all": lambda: live.set_visibility(d_all), "device_one": lambda: live.set_visibility(d_one, picked)}
    got = {}
    for k in names:
        def timed(call=calls[k]):
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3
        wall, err = stderr_of(timed)
        m = re.search(r"\[rt_set_visibility\] copy ([0-9.]+) ms patch ([0-9.]+) ms objects (\d+)", err)
        assert m and int(m.group(3)) == (1 if k.endswith("one") else n_objs), err
        got[k] = (wall, float(m.group(1)), float(m.group(2)))
    frames = {}
    for p in HIDDEN:
        mask = mask_for(rnd, p)
        live.set_visibility(mask)
        frames[("live", p)] = frame_kernel_ms(live, d_frame)
        changed = R.with_visibility(objs, mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh = HIPRaytracer(changed, lights, None, depth, kernel=kernel, camera=(W, H, z))   # what a caller pays today
        wall_fresh = (time.perf_counter() - t0) * 1e3
        create_ms = float(fresh.setup_times()["create_ms"])
        frames[("fresh", p)] = frame_kernel_ms(fresh, d_frame)
        if rnd == rounds:   # the contract, at this size: the same frame, bit for bit
            a = torch.empty_like(d_frame)
            live.render_device(a.data_ptr(), 0)
            fresh.render_device(d_frame.data_ptr(), 0)
            torch.cuda.synchronize()
            equal[p] = bool(torch.equal(a.view(torch.int32), d_frame.view(torch.int32)))
        fresh.close()
        if p == 50 and rnd:
            rows["fresh_wall_ms"].append(wall_fresh)
            rows["fresh_create_ms"].append(create_ms)
    if rnd == 0:
        continue
    for k in names:
        for what, v in zip(("wall_ms", "copy_device_ms", "patch_device_ms"), got[k]):
            rows[f"{k}_{what}"].append(v)
    for (side, p), v in frames.items():
        rows[f"frame_{side}_hidden{p}_ms"].append(v)
os.environ.pop("RT_VISIBILITY_TRACE")
live.set_visibility(np.ones(n_objs, dtype=np.uint8))
shown_again = [frame_kernel_ms(live, d_frame) for _ in range(rounds)]
live.close()
res["last_round_frame_equals_fresh"] = equal
res.update({k: summary(v) for k, v in rows.items()})
res["frame_all_shown_again_ms"] = summary(shown_again)
spread = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
res["frame_spread_ms"] = spread
res["frame_shown_again_minus_untouched_median_ms"] = res["frame_all_shown_again_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]
res["shown_again_not_slower_beyond_spread"] = bool(res["frame_shown_again_minus_untouched_median_ms"] <= spread)
res["live_over_fresh_frame_ratio"] = {str(p): res[f"frame_live_hidden{p}_ms"]["median_ms"] / res[f"frame_fresh_hidden{p}_ms"]["median_ms"] for p in HIDDEN}
res["patch_bytes_per_object"] = {"read": 9, "written": 20}

if parent_lib:   # the untouched frame from the parent commit's library and from this one, in child processes, alternating: three pairs
    runs = {"parent": [], "this": []}
    for _ in range(3):
        for which, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("RT_LIB_OVERRIDE", None)
            if lib:
                env["RT_LIB_OVERRIDE"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), wl, str(rounds), "--frame-only"], env=env, capture_output=True,
                                 text=True, timeout=600, check=True).stdout
            runs[which].append(json.loads(out.strip().splitlines()[-1]))
    res["frame_parent_library"] = runs["parent"]
    res["frame_this_library_fresh_process"] = runs["this"]
    med = {k: statistics.median(r["frame_kernel_ms"]["median_ms"] for r in v) for k, v in runs.items()}
    res["frame_this_minus_parent_median_ms"] = med["this"] - med["parent"]
    res["this_library_within_spread_of_parent"] = bool(abs(med["this"] - med["parent"]) <= spread)

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items()
                  if k not in ("what", "frame_parent_library", "frame_this_library_fresh_process")}, indent=1))
