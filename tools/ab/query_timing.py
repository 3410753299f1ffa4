#!/usr/bin/env python3
"""Ray queries (hip_raytracer.h, "ray queries") on one workload (cfg4: 100 k spheres, 4096^2, depth 3), warmed, medians of 20 with
one warm-up call per case:

(a) rt_query_closest_device / rt_query_occluded_device on a live shade_and_reflect context, for n in (1, 4 096, 1 M, 4096^2) rays of
    two populations - the pinhole frame's own rays (a random sample of the frame, in frame order, for n below the frame) and random rays with
    origins in the grid's box: wall per call (enqueue + a device synchronise), device_ms of rt_get_query_info, Mrays/s from the
    device time, rays per route and exact tests;
(b) one brute-force ray (its origin outside the box) and one pick (rt_query_primary of the centre pixel), the same figures;
(c) the frame's kernel time before any query and after all of them on the same context (its own repeated frames: the spread).
With --parent-lib PATH (a library built from the parent commit) child processes that alternate between that library and this one
(RT_LIB_OVERRIDE), three pairs, measure
(d) the way the parent answers the same questions: for n = 4096^2 a SECOND RT_KERNEL_HITTEST context (its creation once: wall and
    create_ms), then rt_set_rays_device + rt_render_device with aux buffers per call; for n = 1 one rt_render_aux frame on the live
    context (and the kernel time of one rt_render_device with aux buffers, without the 128 MB read-back);
(e) the untouched frame, parent against this library: no frame code changed, so the two must agree within the spread.
usage: python tools/ab/query_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
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
child = None
for flag in ("--frame-only", "--parent-way"):
    if flag in argv:
        argv.remove(flag)
        child = flag
wl = argv[0] if len(argv) > 0 else "cfg4"
rounds = max(10, int(argv[1])) if len(argv) > 1 else 20
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "query_timing.json")
SIZES = (1, 4096, 1 << 20, None)   # None: the whole frame


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

if child == "--frame-only":   # the frame of whatever library RT_LIB_OVERRIDE names, one JSON line
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
    d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
    frame_kernel_ms(rt, d_frame)
    ms = [frame_kernel_ms(rt, d_frame) for _ in range(rounds)]
    rt.close()
    print(json.dumps({"library_sha16": bench.library_sha16(), "frame_kernel_ms": summary(ms)}))
    sys.exit(0)

if child == "--parent-way":   # what a caller does without ray queries, with the entry points the parent commit has
    live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
    d_rays = live.generate_rays(W, H, z, np.eye(3))   # "N rays on the GPU": here the frame's own
    d_t = torch.empty(n_frame, dtype=torch.float32, device="cuda")
    d_i = torch.empty(n_frame, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    second = HIPRaytracer(objs, lights, None, 0, kernel="hittest", camera=(W, H, z))
    create_wall = (time.perf_counter() - t0) * 1e3
    create_ms = float(second.setup_times()["create_ms"])
    d_out = torch.empty(n_frame, dtype=torch.float32, device="cuda")

    def second_context_call():
        second.set_rays(d_rays)
        second._check(second._lib.rt_set_aux_device(second._ctx, d_t.data_ptr(), d_i.data_ptr()))
        second.render_device(d_out.data_ptr(), 0)

    def aux_frame_kernel():
        live._check(live._lib.rt_set_aux_device(live._ctx, d_t.data_ptr(), d_i.data_ptr()))
        live.render_device(d_frame.data_ptr(), 0)

    d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
    rows = {"second_context_set_rays_and_render_wall_ms": [], "second_context_render_kernel_ms": [], "one_ray_render_aux_wall_ms": [],
            "one_ray_aux_frame_kernel_ms": []}
    for rnd in range(rounds + 1):
        a = wall_of(second_context_call)
        b = float(second.stats().last_kernel_ms)
        c = wall_of(live.render_aux)
        wall_of(aux_frame_kernel)
        d = float(live.stats().last_kernel_ms)
        if rnd:
            for k, v in zip(rows, (a, b, c, d)):
                rows[k].append(v)
    print(json.dumps(dict({k: summary(v) for k, v in rows.items()}, library_sha16=bench.library_sha16(),
                          second_context_create_wall_ms=create_wall, second_context_create_ms=create_ms)))
    sys.exit(0)

res = {"what": "rt_query_closest_device / rt_query_occluded_device / rt_query_primary on a live context: wall per call (enqueue + synchronise), "
               "device_ms, Mrays/s, rays per route, exact tests; the parent's way to the same answers in alternating fresh processes",
       "workload": desc, "frame": [W, H], "objects": len(objs), "rounds": rounds, "library_sha16": bench.library_sha16(),
       "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
frame_kernel_ms(live, d_frame)
res["frame_untouched_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
info = live.rays_info()
lo, hi = torch.tensor(info["box_lo"], device="cuda"), torch.tensor(info["box_hi"], device="cuda")
res["box_lo"], res["box_hi"] = [float(v) for v in info["box_lo"]], [float(v) for v in info["box_hi"]]
gen = torch.Generator(device="cuda").manual_seed(7)
frame_rays = live.generate_rays(W, H, z, np.eye(3))   # the identity pose: the pinhole grid itself, bit for bit
random_rays = torch.zeros((n_frame, 8), dtype=torch.float32, device="cuda")
mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.99
random_rays[:, :3] = (mid + (torch.rand((n_frame, 3), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1) * half).float()
random_rays[:, 3] = 1.0
random_rays[:, 4:7] = torch.randn((n_frame, 3), generator=gen, device="cuda") * 10.0
torch.cuda.synchronize()


def sample(rays, n):
    if n is None:
        return rays
    if n == 1:
        return rays[(H // 2) * W + W // 2:(H // 2) * W + W // 2 + 1].contiguous()
    picked = torch.randperm(n_frame, generator=gen, device="cuda")[:n].sort().values   # a sample of the whole frame, in frame order
    return rays[picked].contiguous()


def measure(call):
    """One warm-up, then `rounds` calls: wall, and the counters of the last one."""
    wall_of(call)
    wall, device = [], []
    for _ in range(rounds):
        wall.append(wall_of(call))
        device.append(live.query_info()["device_ms"])
    q = live.query_info()
    dev = statistics.median(device)
    return {"wall_ms": summary(wall), "device_ms": summary(device), "mrays_per_s": q["n_rays"] / dev / 1e3 if dev > 0 else None,
            "n_rays": q["n_rays"], "n_grid": q["n_grid"], "n_brute": q["n_brute"], "object_tests": q["object_tests"],
            "tests_per_ray": q["object_tests"] / max(q["n_rays"], 1)}


cases = {}
for name, rays in (("frame_rays", frame_rays), ("random_in_box_rays", random_rays)):
    for n in SIZES:
        r = sample(rays, n)
        label = f"{name}_n{r.shape[0]}"
        cases[label + "_closest"] = measure(lambda: live.query_closest(r))
        cases[label + "_occluded"] = measure(lambda: live.query_occluded(r))
outside = torch.tensor([[float(info["box_hi"][0]) + 50.0, 0.0, float(mid[2]), 1.0, -1.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device="cuda")
cases["one_brute_force_ray_closest"] = measure(lambda: live.query_closest(outside))
cases["one_brute_force_ray_occluded"] = measure(lambda: live.query_occluded(outside))
cases["pick_centre_pixel"] = measure(lambda: live.pick([(H // 2) * W + W // 2]))
res["cases"] = cases
res["frame_after_the_queries_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
live.close()
spread = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
res["frame_spread_ms"] = spread
res["frame_after_minus_untouched_median_ms"] = res["frame_after_the_queries_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]

if parent_lib:
    runs = {"parent_way_on_parent": [], "frame_parent": [], "frame_this": []}
    for _ in range(3):
        for which, lib, mode in (("parent_way_on_parent", parent_lib, "--parent-way"), ("frame_this", None, "--frame-only"), ("frame_parent", parent_lib, "--frame-only")):
            env = dict(os.environ)
            env.pop("RT_LIB_OVERRIDE", None)
            if lib:
                env["RT_LIB_OVERRIDE"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), wl, str(rounds), mode], env=env, capture_output=True, text=True,
                                 timeout=600, check=True).stdout
            runs[which].append(json.loads(out.strip().splitlines()[-1]))
    res["parent_way"] = runs["parent_way_on_parent"]
    res["frame_parent_library"] = runs["frame_parent"]
    res["frame_this_library_fresh_process"] = runs["frame_this"]
    med = {k: statistics.median(r["frame_kernel_ms"]["median_ms"] for r in runs[k]) for k in ("frame_parent", "frame_this")}
    res["frame_this_minus_parent_median_ms"] = med["frame_this"] - med["frame_parent"]
    res["this_library_within_spread_of_parent"] = bool(abs(med["frame_this"] - med["frame_parent"]) <= spread)
    pw = runs["parent_way_on_parent"]
    res["parent_way_medians"] = {k: statistics.median(r[k]["median_ms"] for r in pw) for k in pw[0] if isinstance(pw[0][k], dict)}
    res["parent_way_medians"]["second_context_create_wall_ms"] = statistics.median(r["second_context_create_wall_ms"] for r in pw)

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
brief = {k: {"wall_ms": v["wall_ms"]["median_ms"], "device_ms": v["device_ms"]["median_ms"], "mrays_per_s": v["mrays_per_s"], "n_grid": v["n_grid"],
             "n_brute": v["n_brute"], "tests_per_ray": v["tests_per_ray"]} for k, v in cases.items()}
print(json.dumps({"cases": brief, "frame_untouched_ms": res["frame_untouched_ms"]["median_ms"], "frame_spread_ms": spread,
                  "frame_after_minus_untouched_median_ms": res["frame_after_minus_untouched_median_ms"],
                  "parent_way_medians": res.get("parent_way_medians"), "frame_this_minus_parent_median_ms": res.get("frame_this_minus_parent_median_ms"),
                  "this_library_within_spread_of_parent": res.get("this_library_within_spread_of_parent")}, indent=1))
