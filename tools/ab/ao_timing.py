#!/usr/bin/env python3
"""Ambient-occlusion frames (hip_raytracer.h, "ambient-occlusion frames") on one workload (cfg4: 100 k spheres, 4096^2), K = 4, 8, 16,
warmed, medians of 20 after one warm-up call per case, on ONE live context in one process; every case timed twice over - by an event
pair on the stream and by wall time with a device synchronise:

    render_ao      the frame form: the G-buffer pass and the AO kernel (gbuffer_ms / ao_ms of rt_get_ao_info beside it);
    ao_pass        the pass alone on a G-buffer already on the device; its rays per second from ao_ms;
    four steps     the route without the feature, which the parent library can run too: render_gbuffer (index, point, normal), the
                   n * K rays built in torch by ao.py's definition (the live items compacted first, as a caller who does not want to
                   trace dead rays would: one host synchronisation), query_occluded, the reduction in torch; and query_occluded's own
                   device_ms on those rays - the same rays the pass traces - as rays per second.
    The counts of the three routes are compared once per K.
With --parent-lib PATH (a library built from the parent commit) child processes that alternate between that library and this one
(RT_LIB_OVERRIDE), three pairs, measure the untouched frame; the difference at the medians is reported against the spread of the
context's own repeated frames.
usage: python tools/ab/ao_timing.py cfg4 [rounds >= 5] [out.json] [--parent-lib PATH]"""
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
rounds = max(5, int(argv[1])) if len(argv) > 1 else 20
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "ao_timing.json")
KS = (4, 8, 16)
N_SETS, RADIUS, BIAS = 64, 2.0, 1e-3


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def frame_kernel_ms(rt, d_frame, n=3):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return statistics.median(ms[1:])


def timed(fn):
    """(wall ms with a synchronise, ms between two events on the stream) of one call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def measure(fn, after=None):
    timed(fn)
    wall, events, extra = [], [], []
    for _ in range(rounds):
        w, e = timed(fn)
        wall.append(w)
        events.append(e)
        if after:
            extra.append(after())
    return {"wall_ms": summary(wall), "event_ms": summary(events)}, extra


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

from opencl_raytracer_amd import ao as AO  # noqa: E402

res = {"what": "rt_render_ao_device and rt_ao_device on one live context against render_gbuffer + a torch ray build + query_occluded + a torch "
               "reduction: wall per call (enqueue + synchronise) and an event pair; rays per second of the pass and of query_occluded on the same "
               "rays; the untouched frame against the parent library in alternating fresh processes",
       "workload": desc, "frame": [W, H], "objects": len(objs), "rounds": rounds, "n_sets": N_SETS, "radius": RADIUS, "bias": BIAS,
       "library_sha16": bench.library_sha16(), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
frame_kernel_ms(live, d_frame)
res["frame_untouched_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])

gb = {"index": torch.empty(n_frame, dtype=torch.int32, device="cuda"), "point": torch.empty((n_frame, 4), dtype=torch.float32, device="cuda"),
      "normal": torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")}
out = {"unoccluded": torch.empty(n_frame, dtype=torch.uint8, device="cuda"), "ao": torch.empty(n_frame, dtype=torch.float32, device="cuda")}
items = torch.arange(n_frame, dtype=torch.int64, device="cuda")


def torch_rays(d_dirs, K):
    """ao.rays in torch for the live items only: (rays float32 (n_live * K, 8), the live items' numbers)"""
    p, nr = gb["point"], gb["normal"]
    live_mask = (gb["index"] >= 0) & torch.isfinite(p[:, :3]).all(dim=1) & torch.isfinite(nr[:, :3]).all(dim=1)
    who = torch.nonzero(live_mask).squeeze(1)                      # (a host synchronisation: the count)
    p, nr = p[who], nr[who]
    h = (who * AO.HASH) & 0xFFFFFFFF
    sets = (h >> 16) % N_SETS
    d = d_dirs[(sets * K)[:, None] + torch.arange(K, device="cuda")[None, :], :3]          # (n_live, K, 3)
    s = (d[..., 0] * nr[:, None, 0] + d[..., 1] * nr[:, None, 1]) + d[..., 2] * nr[:, None, 2]
    d = torch.where((s < 0)[..., None], -d, d)
    rays = torch.zeros((len(who), K, 8), dtype=torch.float32, device="cuda")
    rays[..., 0:3] = (p[:, :3] + BIAS32 * nr[:, :3])[:, None, :]
    rays[..., 3] = 1.0
    rays[..., 4:7] = d
    return rays.view(-1, 8), who


BIAS32 = float(np.float32(BIAS))
cases = {}
for K in KS:
    dirs = AO.directions(K, N_SETS, RADIUS, seed=K)
    d_dirs = torch.from_numpy(dirs).cuda()
    case = {}

    case["render_ao"], infos = measure(lambda: live.render_ao(d_dirs, K, BIAS, want=("unoccluded", "ao"), out=out), live.ao_info)
    case["render_ao"]["gbuffer_ms"] = summary([i["gbuffer_ms"] for i in infos])
    case["render_ao"]["ao_ms"] = summary([i["ao_ms"] for i in infos])
    info = infos[-1]
    case["counts"] = {k: info[k] for k in ("n_items", "n_live", "n_rays", "n_grid", "n_brute", "object_tests")}
    frame_counts = out["unoccluded"].clone()

    live.render_gbuffer(want=("index", "point", "normal"), out=gb)
    case["ao_pass"], infos = measure(lambda: live.ao_pass(gb["point"], gb["normal"], gb["index"], d_dirs, K, BIAS, want=("unoccluded", "ao"), out=out),
                                     live.ao_info)
    ao_ms = statistics.median(i["ao_ms"] for i in infos)
    case["ao_pass"]["ao_ms"] = summary([i["ao_ms"] for i in infos])
    case["ao_pass"]["rays_per_s"] = info["n_rays"] / ao_ms * 1e3
    case["ao_pass"]["bytes_per_item"] = {"read": 36, "written": 5}
    pass_counts = out["unoccluded"].clone()

    four_counts = torch.empty(n_frame, dtype=torch.uint8, device="cuda")

    def four_steps():
        live.render_gbuffer(want=("index", "point", "normal"), out=gb)
        rays, who = torch_rays(d_dirs, K)
        occluded = live.query_occluded(rays)
        four_counts.fill_(K)
        four_counts[who] = (K - occluded.view(-1, K).sum(dim=1)).to(torch.uint8)

    case["four_steps"], infos = measure(four_steps, live.query_info)
    q_ms = statistics.median(i["device_ms"] for i in infos)
    case["four_steps"]["query_occluded_device_ms"] = summary([i["device_ms"] for i in infos])
    case["four_steps"]["query_occluded_rays_per_s"] = infos[-1]["n_rays"] / q_ms * 1e3
    case["four_steps"]["query_counts"] = {k: infos[-1][k] for k in ("n_rays", "n_grid", "n_brute")}
    case["four_steps"]["extra_bytes_per_live_item"] = 33 * K
    case["same_counts"] = {"ao_pass_as_render_ao": bool(torch.equal(pass_counts, frame_counts)),
                           "four_steps_as_render_ao": bool(torch.equal(four_counts, frame_counts))}
    case["speedup_over_four_steps"] = {
        "render_ao_wall": case["four_steps"]["wall_ms"]["median_ms"] / case["render_ao"]["wall_ms"]["median_ms"],
        "render_ao_events": case["four_steps"]["event_ms"]["median_ms"] / case["render_ao"]["event_ms"]["median_ms"],
        "ao_kernel_over_query_occluded_kernel": q_ms / ao_ms}
    cases[f"K{K}"] = case
    del d_dirs

res["cases"] = cases
res["frame_after_the_passes_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
live.close()
spread = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
res["frame_spread_ms"] = spread
res["frame_after_minus_untouched_median_ms"] = res["frame_after_the_passes_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]

if parent_lib:
    runs = {"frame_parent": [], "frame_this": []}
    for _ in range(3):
        for which, lib in (("frame_this", None), ("frame_parent", parent_lib)):
            env = dict(os.environ)
            env.pop("RT_LIB_OVERRIDE", None)
            if lib:
                env["RT_LIB_OVERRIDE"] = lib
            text = subprocess.run([sys.executable, os.path.abspath(__file__), wl, str(rounds), "--frame-only"], env=env, capture_output=True, text=True,
                                  timeout=600, check=True).stdout
            runs[which].append(json.loads(text.strip().splitlines()[-1]))
    res["frame_parent_library"] = runs["frame_parent"]
    res["frame_this_library_fresh_process"] = runs["frame_this"]
    med = {k: statistics.median(r["frame_kernel_ms"]["median_ms"] for r in runs[k]) for k in runs}
    res["frame_this_minus_parent_median_ms"] = med["frame_this"] - med["frame_parent"]
    res["this_library_within_spread_of_parent"] = bool(abs(med["frame_this"] - med["frame_parent"]) <= spread)

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)


def brief(v):
    if isinstance(v, dict):
        if "median_ms" in v and "all_ms" in v:
            return round(v["median_ms"], 3)
        return {k: brief(x) for k, x in v.items()}
    return v


print(json.dumps({"cases": brief(cases), "frame_untouched_ms": res["frame_untouched_ms"]["median_ms"], "frame_spread_ms": spread,
                  "frame_after_minus_untouched_median_ms": res["frame_after_minus_untouched_median_ms"],
                  "frame_this_minus_parent_median_ms": res.get("frame_this_minus_parent_median_ms"),
                  "this_library_within_spread_of_parent": res.get("this_library_within_spread_of_parent")}))
