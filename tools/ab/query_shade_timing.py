#!/usr/bin/env python3
"""Shaded queries (hip_raytracer.h, "shaded queries") on one workload (cfg4: 100 k spheres, 4096^2, depth 3), warmed, medians of 20
after one warm-up call per case, on ONE live shade_and_reflect context in one process:

(a) rt_query_shade_device (rgba out) for 1 ray (the centre pixel's), 4 096 and 1 M of the pinhole frame's own rays (a random sample
    of the frame, in frame order) and 1 M random rays with origins in the grid's box: wall per call (enqueue + a device synchronise),
    device_ms and the counters of rt_get_query_shade_info;
(b) beside each: the same rays rendered by a SECOND shade_and_reflect context of matching ray count - rt_set_rays_device +
    rt_render_device, wall per pair of calls and the frame's kernel time - and the time to create that second context (wall of the
    constructor, 3 times);
(c) the frame's kernel time before any query and after all of them on the same context (its own repeated frames: the spread).
With --parent-lib PATH (a library built from the parent commit) child processes that alternate between that library and this one
(RT_LIB_OVERRIDE), three pairs, measure
(d) the untouched frame, parent against this library: no frame code changed, so the two must agree within the spread.
usage: python tools/ab/query_shade_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402

argv = sys.argv[1:]
parent_lib = None
if "--parent-lib" in argv:
    k = argv.index("--parent-lib")
    parent_lib = os.path.abspath(argv[k + 1])
    del argv[k:k + 2]
child = "--frame-only" in argv
if child:
    argv.remove("--frame-only")
wl = argv[0] if len(argv) > 0 else "cfg4"
rounds = max(10, int(argv[1])) if len(argv) > 1 else 20
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "query_shade_timing.json")


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def frame_kernel_ms(rt, d_frame, n=3):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return statistics.median(ms[1:])


def wall_of(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n_frame = W * H
z = float(camera.camera_z(H))

if child:   # the frame of whatever library RT_LIB_OVERRIDE names, one JSON line
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
    d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
    frame_kernel_ms(rt, d_frame)
    ms = [frame_kernel_ms(rt, d_frame) for _ in range(rounds)]
    rt.close()
    print(json.dumps({"library_sha16": bench.library_sha16(), "frame_kernel_ms": summary(ms)}))
    sys.exit(0)

res = {"what": "rt_query_shade_device on one live context against a second context of matching ray count (rt_set_rays_device + "
               "rt_render_device) and that context's creation; the untouched frame against the parent library in alternating fresh processes",
       "workload": desc, "frame": [W, H], "objects": len(objs), "rounds": rounds, "library_sha16": bench.library_sha16(),
       "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
frame_kernel_ms(live, d_frame)
res["frame_untouched_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
info = live.rays_info()
lo, hi = torch.tensor(info["box_lo"], device="cuda"), torch.tensor(info["box_hi"], device="cuda")
gen = torch.Generator(device="cuda").manual_seed(7)
frame_rays = live.generate_rays(W, H, z, np.eye(3))   # the identity pose: the pinhole grid itself, bit for bit
mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.99
n_random = 1 << 20
random_rays = torch.zeros((n_random, 8), dtype=torch.float32, device="cuda")
random_rays[:, :3] = (mid + (torch.rand((n_random, 3), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1) * half).float()
random_rays[:, 3] = 1.0
random_rays[:, 4:7] = torch.randn((n_random, 3), generator=gen, device="cuda") * 10.0
torch.cuda.synchronize()


def sample(rays, n):
    total = rays.shape[0]
    if n == 1:
        mid_ray = (H // 2) * W + W // 2 if total == n_frame else total // 2
        return rays[mid_ray:mid_ray + 1].contiguous()
    if n == total:
        return rays
    picked = torch.randperm(total, generator=gen, device="cuda")[:n].sort().values   # a sample of the whole set, in its order
    return rays[picked].contiguous()


cases = {}
for label, rays, n in (("one_ray", frame_rays, 1), ("frame_rays_n4096", frame_rays, 4096), ("frame_rays_n1048576", frame_rays, 1 << 20),
                       ("random_in_box_rays_n1048576", random_rays, 1 << 20)):
    r = sample(rays, n)
    out = live.query_shade(r)            # allocated once per case: the calls measure the query, not torch's allocator
    wall_of(lambda: live.query_shade(r, out=out))
    wall, device = [], []
    for _ in range(rounds):
        wall.append(wall_of(lambda: live.query_shade(r, out=out)))
        device.append(live.query_shade_info()["device_ms"])
    q = live.query_shade_info()
    dev = statistics.median(device)
    case = {"query_shade": {"wall_ms": summary(wall), "device_ms": summary(device), "mrays_per_s": q["n_rays"] / dev / 1e3 if dev > 0 else None,
                            **{k: q[k] for k in ("n_rays", "n_grid", "n_brute", "n_literal", "hit_rays", "rays_traced", "rays_reference", "object_tests")}}}
    # the second context: created with rays of this count (the first `n` of the set), then given the case's rays from the device
    host_rays = r.cpu().numpy()
    create = []
    second = None
    for _ in range(3):
        if second is not None:
            second.close()
        t0 = time.perf_counter()
        second = HIPRaytracer(objs, lights, host_rays, depth, kernel=kernel, raygen=False)
        torch.cuda.synchronize()
        create.append((time.perf_counter() - t0) * 1e3)
    d_out = torch.empty((n, 4), dtype=torch.float32, device="cuda")

    def through_the_frame():
        second._check(second._lib.rt_set_rays_device(second._ctx, r.data_ptr(), n, None))
        second.render_device(d_out.data_ptr(), 0)
    wall_of(through_the_frame)
    wall, kern = [], []
    for _ in range(rounds):
        wall.append(wall_of(through_the_frame))
        kern.append(float(second.stats().last_kernel_ms))
    case["second_context"] = {"set_rays_and_render_wall_ms": summary(wall), "frame_kernel_ms": summary(kern), "create_wall_ms": summary(create),
                              "wavefront": int(second.stats().wavefront)}
    case["same_bits"] = bool(torch.equal(out["rgba"].view(torch.int32), d_out.view(torch.int32)))
    second.close()
    case["query_over_frame"] = {"device": dev / statistics.median(kern), "wall": case["query_shade"]["wall_ms"]["median_ms"] / statistics.median(wall)}
    cases[label] = case
res["cases"] = cases
res["frame_after_the_queries_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
live.close()
spread = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
res["frame_spread_ms"] = spread
res["frame_after_minus_untouched_median_ms"] = res["frame_after_the_queries_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]

if parent_lib:
    runs = {"frame_parent": [], "frame_this": []}
    for _ in range(3):
        for which, lib in (("frame_this", None), ("frame_parent", parent_lib)):
            env = dict(os.environ)
            env.pop("RT_LIB_OVERRIDE", None)
            if lib:
                env["RT_LIB_OVERRIDE"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), wl, str(rounds), "--frame-only"], env=env, capture_output=True, text=True,
                                 timeout=600, check=True).stdout
            runs[which].append(json.loads(out.strip().splitlines()[-1]))
    res["frame_parent_library"] = runs["frame_parent"]
    res["frame_this_library_fresh_process"] = runs["frame_this"]
    med = {k: statistics.median(r["frame_kernel_ms"]["median_ms"] for r in runs[k]) for k in runs}
    res["frame_this_minus_parent_median_ms"] = med["frame_this"] - med["frame_parent"]
    res["this_library_within_spread_of_parent"] = bool(abs(med["frame_this"] - med["frame_parent"]) <= spread)

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
brief = {k: {"query_wall_ms": v["query_shade"]["wall_ms"]["median_ms"], "query_device_ms": v["query_shade"]["device_ms"]["median_ms"],
             "mrays_per_s": v["query_shade"]["mrays_per_s"], "n_grid": v["query_shade"]["n_grid"], "n_brute": v["query_shade"]["n_brute"],
             "second_wall_ms": v["second_context"]["set_rays_and_render_wall_ms"]["median_ms"], "second_kernel_ms": v["second_context"]["frame_kernel_ms"]["median_ms"],
             "second_create_ms": v["second_context"]["create_wall_ms"]["median_ms"], "same_bits": v["same_bits"], "query_over_frame": v["query_over_frame"]}
         for k, v in cases.items()}
print(json.dumps({"cases": brief, "frame_untouched_ms": res["frame_untouched_ms"]["median_ms"], "frame_spread_ms": spread,
                  "frame_after_minus_untouched_median_ms": res["frame_after_minus_untouched_median_ms"],
                  "frame_this_minus_parent_median_ms": res.get("frame_this_minus_parent_median_ms"),
                  "this_library_within_spread_of_parent": res.get("this_library_within_spread_of_parent")}, indent=1))
