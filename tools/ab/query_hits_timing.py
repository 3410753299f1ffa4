#!/usr/bin/env python3
"""Hit-record queries (hip_raytracer.h, "hit-record queries") on one workload (cfg4: 100 k spheres, 4096^2, depth 3), warmed, medians
of 20 with one warm-up call per case, all on ONE live shade_and_reflect context in one process:

(a) rt_query_closest_device (32 bytes per ray in, 8 out) against rt_query_hits_device with every output (t, index, point, normal,
    reflected: 32 in, 72 out) and with point + normal only (32 in, 32 out), for n in (1, 4 096, 1 M) rays of two populations - the pinhole frame's own
    rays (a random sample of the frame, in frame order) and random rays with origins in the grid's box: wall per call (enqueue + a
    device synchronise), device_ms of rt_get_query_info, the ratio to query_closest, rays per route;
(b) a 3-bounce chain on the 1 M rays of each population with the mask (hits.chain): wall, the device time and the traced rays of
    every bounce - and that no bounce sent a missed ray down the brute-force route;
(c) one brute-force ray (its origin outside the box) as query_closest and as query_hits, side by side; 1 M rays of each population on
    a second context created with RT_FLAG_UNFUSED (whose hit-record kernels hold fewer waves per SIMD), query_closest against
    query_hits with every output;
(d) the frame's kernel time before any query and after all of them on the same context (its own repeated frames: the spread).
With --parent-lib PATH (a library built from the parent commit) child processes that alternate between that library and this one
(RT_LIB_OVERRIDE), three pairs, measure
(e) the untouched frame, parent against this library: no frame code changed, so the two must agree within the spread.
usage: python tools/ab/query_hits_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera, hits as HT  # noqa: E402
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
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "query_hits_timing.json")
SIZES = (1, 4096, 1 << 20)
BYTES_PER_RAY = {"closest": {"in": 32, "out": 8, "total": 40}, "hits_all": {"in": 32, "out": 8 + 16 + 16 + 32, "total": 104},
                 "hits_point_normal": {"in": 32, "out": 32, "total": 64}}


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

res = {"what": "rt_query_hits_device against rt_query_closest_device on one live context: wall per call (enqueue + synchronise), device_ms, the "
               "ratio, rays per route; a 3-bounce chain with the mask; the untouched frame against the parent library in alternating fresh processes",
       "workload": desc, "frame": [W, H], "objects": len(objs), "rounds": rounds, "library_sha16": bench.library_sha16(),
       "bytes_per_ray": BYTES_PER_RAY, "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
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


def measure(call, rt=None):
    """One warm-up, then `rounds` calls: wall, and the counters of the last one."""
    rt = live if rt is None else rt
    wall_of(call)
    wall, device = [], []
    for _ in range(rounds):
        wall.append(wall_of(call))
        device.append(rt.query_info()["device_ms"])
    q = rt.query_info()
    dev = statistics.median(device)
    return {"wall_ms": summary(wall), "device_ms": summary(device), "mrays_per_s": q["n_rays"] / dev / 1e3 if dev > 0 else None,
            "n_rays": q["n_rays"], "n_grid": q["n_grid"], "n_brute": q["n_brute"], "object_tests": q["object_tests"]}


cases, ratios, chains = {}, {}, {}
for name, rays in (("frame_rays", frame_rays), ("random_in_box_rays", random_rays)):
    for n in SIZES:
        r = sample(rays, n)
        label = f"{name}_n{r.shape[0]}"
        # outputs allocated once per case: the calls measure the query, not torch's allocator
        out_all = {k: v for k, v in live.query_hits(r).items()}
        out_pn = {k: out_all[k] for k in ("point", "normal")}
        cases[label + "_closest"] = measure(lambda: live.query_closest(r))
        cases[label + "_hits_all"] = measure(lambda: live.query_hits(r, out=out_all))
        cases[label + "_hits_point_normal"] = measure(lambda: live.query_hits(r, want=("point", "normal"), out=out_pn))
        base = cases[label + "_closest"]
        ratios[label] = {k: {"device": cases[f"{label}_{k}"]["device_ms"]["median_ms"] / base["device_ms"]["median_ms"],
                             "wall": cases[f"{label}_{k}"]["wall_ms"]["median_ms"] / base["wall_ms"]["median_ms"]} for k in ("hits_all", "hits_point_normal")}
        hit = out_all["index"] >= 0
        cases[label + "_hits_all"]["hits"] = int(hit.sum())
    # (b) the chain on the 1 M rays
    r = sample(rays, 1 << 20)
    per_bounce = []

    def query(q_rays, q_mask):
        h = live.query_hits(q_rays, q_mask)
        per_bounce.append(live.query_info())
        return h
    HT.chain(query, r, 3)   # warm-up, and the counters of every bounce
    bounces = list(per_bounce)
    wall = [wall_of(lambda: HT.chain(live.query_hits, r, 3)) for _ in range(rounds)]
    chains[name] = {"wall_ms": summary(wall), "bounces": [{k: b[k] for k in ("n_rays", "n_grid", "n_brute", "device_ms")} for b in bounces]}
outside = torch.tensor([[float(info["box_hi"][0]) + 50.0, 0.0, float(mid[2]), 1.0, -1.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device="cuda")
cases["one_brute_force_ray_closest"] = measure(lambda: live.query_closest(outside))
cases["one_brute_force_ray_hits_all"] = measure(lambda: live.query_hits(outside))
ratios["one_brute_force_ray"] = {"hits_all": {"device": cases["one_brute_force_ray_hits_all"]["device_ms"]["median_ms"] / cases["one_brute_force_ray_closest"]["device_ms"]["median_ms"]}}
cases["pick_hit_centre_pixel"] = measure(lambda: live.pick_hit([(H // 2) * W + W // 2]))
unfused = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z), fused=False)
for name, rays in (("frame_rays", frame_rays), ("random_in_box_rays", random_rays)):
    r = sample(rays, 1 << 20)
    label = f"unfused_{name}_n{r.shape[0]}"
    out_all = unfused.query_hits(r)
    cases[label + "_closest"] = measure(lambda: unfused.query_closest(r), unfused)
    cases[label + "_hits_all"] = measure(lambda: unfused.query_hits(r, out=out_all), unfused)
    ratios[label] = {"hits_all": {"device": cases[label + "_hits_all"]["device_ms"]["median_ms"] / cases[label + "_closest"]["device_ms"]["median_ms"],
                                  "wall": cases[label + "_hits_all"]["wall_ms"]["median_ms"] / cases[label + "_closest"]["wall_ms"]["median_ms"]}}
unfused.close()
res["cases"], res["ratio_to_query_closest"], res["chain_3_bounces_1M"] = cases, ratios, chains
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
brief = {k: {"wall_ms": v["wall_ms"]["median_ms"], "device_ms": v["device_ms"]["median_ms"], "mrays_per_s": v["mrays_per_s"], "n_grid": v["n_grid"],
             "n_brute": v["n_brute"]} for k, v in cases.items()}
print(json.dumps({"cases": brief, "ratio_to_query_closest": ratios,
                  "chain_3_bounces_1M": {k: {"wall_ms": v["wall_ms"]["median_ms"], "bounces": v["bounces"]} for k, v in chains.items()},
                  "frame_untouched_ms": res["frame_untouched_ms"]["median_ms"], "frame_spread_ms": spread,
                  "frame_after_minus_untouched_median_ms": res["frame_after_minus_untouched_median_ms"],
                  "frame_this_minus_parent_median_ms": res.get("frame_this_minus_parent_median_ms"),
                  "this_library_within_spread_of_parent": res.get("this_library_within_spread_of_parent")}, indent=1))
