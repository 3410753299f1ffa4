#!/usr/bin/env python3
"""Replaceable transforms (hip_raytracer.h) on one workload (cfg4: 100 k spheres, 32 lights, 4096^2, depth 3), ONE process, warmed,
a new position every round:

(a) rt_set_transforms on a live context for ONE object and for 64: wall of the whole call, split into upload + patch (the event
    pair of rt_get_geometry_info: patch_device_ms), the light tiles' rebuild (rt_get_light_tiles_info: build_device_ms) and the
    host remainder (bounds, refusals, registration spheres, the builder's host plan and its four synchronisations);
(b) a FRESH context with the same object array in the same process - what a caller pays today: the wall of constructing it and
    create_ms of rt_get_setup_times;
(c) the frame's kernel time on the live contexts before the first call, behind 1 and behind 64 dynamic objects, and on the fresh
    contexts; object_tests (rt_get_stats of a counted frame) of the live and the fresh frame - the always-loop's extra tests.
With --parent-lib PATH (a library built from the parent commit) the untouched frame is also measured in child processes that
alternate between that library and this one (RT_LIB_OVERRIDE), three runs each: no frame-path kernel changed, so the two sets
must overlap.
Walls are host clocks around calls that end in a device synchronise; every figure is given as best / median / max and all rounds.
usage: python tools/ab/set_transforms_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
import json, os, statistics, subprocess, sys, time
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
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "set_transforms_timing.json")


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def frame_kernel_ms(rt, d_frame, n=3):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return statistics.median(ms[1:])


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

res = {"what": "rt_set_transforms on a live context (one object, 64 objects) against a fresh context with the same object array; the call "
               "split into upload + patch, light-tile rebuild and host remainder; kernel time of the frame before the first call, behind 1 "
               "and 64 dynamic objects and on the fresh contexts, with object_tests; one process, warmed, a new position every round",
       "workload": desc, "frame": [W, H], "rays": n, "objects": n_objs, "rounds": rounds,
       "library_sha16": bench.library_sha16(), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
COUNTS = {"one": 1, "64": 64}
first = n_objs // 2
live = {k: HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z)) for k in COUNTS}
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
box = live["one"].rays_info()
assert box["grid_built"] == 1, "the workload has no grid: nothing of the dynamic set to measure"
mid = 0.5 * (box["box_lo"] + box["box_hi"])
for rt in live.values():
    frame_kernel_ms(rt, d_frame)
res["frame_untouched_ms"] = summary([frame_kernel_ms(live["64"], d_frame) for _ in range(rounds)])   # the spread every margin below is held against
live["64"].count_rays()
res["object_tests_untouched"] = int(live["64"].stats().object_tests)


def moved(count, rnd):
    """Objects first .. first + count - 1 pulled towards the middle of the grid's box, a little further every round (a convex
    combination of two places that are inside: no move leaves the box). Rotation and scale stay."""
    xf = R.transforms_of(objs[first:first + count])
    for k in range(count):
        mv = xf["mv"][k].reshape(4, 4).T.astype(np.float64)
        mv[:3, 3] += (mid - mv[:3, 3]) * 0.02 * (1 + rnd % 16)
        xf["mv"][k] = mv.T.astype(np.float32).reshape(16)
        xf["mvInverse"][k] = np.linalg.inv(mv).T.astype(np.float32).reshape(16)
        xf["mvInverse"][k][[3, 7, 11, 15]] = (0.0, 0.0, 0.0, 1.0)
    return xf


rows = {f"{k}_{what}": [] for k in COUNTS for what in ("wall_ms", "patch_device_ms", "light_tiles_device_ms", "host_remainder_ms", "fresh_wall_ms",
                                                        "fresh_create_ms", "frame_live_ms", "frame_fresh_ms")}
for rnd in range(rounds + 1):   # round 0 warms up: the staging buffer, the builder's memory, code objects
    for k, count in COUNTS.items():
        xf = moved(count, rnd)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        live[k].set_transforms(xf, first)
        wall = (time.perf_counter() - t0) * 1e3
        geo, lt = live[k].geometry_info(), live[k].light_tiles_info()
        assert geo["n_dynamic"] == count and lt["source"] == 2, (geo, lt)
        f_live = frame_kernel_ms(live[k], d_frame)
        changed = R.with_transforms(objs, xf, first)   # what a caller pays today
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh = HIPRaytracer(changed, lights, None, depth, kernel=kernel, camera=(W, H, z))
        wall_fresh = (time.perf_counter() - t0) * 1e3
        create_ms = float(fresh.setup_times()["create_ms"])
        f_fresh = frame_kernel_ms(fresh, d_frame)
        if rnd == rounds:   # the contract, at this size: the same frame, bit for bit; and what the always-loop costs in tests
            a = torch.empty_like(d_frame)
            live[k].render_device(a.data_ptr(), 0)
            fresh.render_device(d_frame.data_ptr(), 0)
            torch.cuda.synchronize()
            res[f"{k}_last_round_frame_equals_fresh"] = bool(torch.equal(a.view(torch.int32), d_frame.view(torch.int32)))
            live[k].count_rays()
            fresh.count_rays()
            res[f"{k}_object_tests_live"] = int(live[k].stats().object_tests)
            res[f"{k}_object_tests_fresh"] = int(fresh.stats().object_tests)
            res[f"{k}_light_tiles_enabled"] = [int(lt["enabled"]), int(fresh.light_tiles_info()["enabled"])]
        fresh.close()
        if rnd == 0:
            continue
        for what, v in (("wall_ms", wall), ("patch_device_ms", geo["patch_device_ms"]), ("light_tiles_device_ms", lt["build_device_ms"]),
                        ("host_remainder_ms", wall - geo["patch_device_ms"] - lt["build_device_ms"]), ("fresh_wall_ms", wall_fresh),
                        ("fresh_create_ms", create_ms), ("frame_live_ms", f_live), ("frame_fresh_ms", f_fresh)):
            rows[f"{k}_{what}"].append(float(v))
for rt in live.values():
    rt.close()
res.update({k: summary(v) for k, v in rows.items()})
res["frame_spread_ms"] = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
for k in COUNTS:
    res[f"{k}_frame_live_minus_untouched_median_ms"] = res[f"{k}_frame_live_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]
    res[f"{k}_frame_live_minus_fresh_median_ms"] = res[f"{k}_frame_live_ms"]["median_ms"] - res[f"{k}_frame_fresh_ms"]["median_ms"]

if parent_lib:   # the untouched frame from the parent commit's library and from this one, in child processes, alternating
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
    med = {k: [r["frame_kernel_ms"]["median_ms"] for r in v] for k, v in runs.items()}
    res["frame_medians_parent_ms"], res["frame_medians_this_ms"] = med["parent"], med["this"]
    res["frame_sets_overlap"] = bool(min(med["this"]) <= max(med["parent"]) and min(med["parent"]) <= max(med["this"]))

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items()
                  if k not in ("what", "frame_parent_library", "frame_this_library_fresh_process")}, indent=1))
