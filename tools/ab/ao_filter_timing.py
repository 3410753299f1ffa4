#!/usr/bin/env python3
"""Filtered ambient occlusion (hip_raytracer.h, "filtered ambient occlusion") on one workload (cfg4: 100 k spheres, 4096^2), K = 4,
medians of 20 after one warm-up call per case; every case timed twice over - by an event pair on the stream and by wall time with a
device synchronise. Three steps, each a child process of its own under its own time limit, started one after the other; the first
that fails ends the run:

    a   ao_filter alone on a G-buffer and counts already on the device, r = 1, 2, 4: wall, event pair, filter_ms of
        rt_get_ao_filter_info and the GB/s of filter_ms over 41 bytes per item (37 read: a count, point, normal, index; 4 written:
        ao) - beside the G-buffer record kernel's rate in profiles/gbuffer_timing.json;
    b   render_ao_filtered (r = 2) against the route it replaces: render_ao, render_gbuffer and the same definition written with
        torch ops on shifted slices on the device; taps and ao of the two compared once;
    c   with --parent-lib PATH (a library built from the parent commit): the untouched frame, that library against this one
        (RT_LIB_OVERRIDE) in alternating fresh processes, three pairs, beside the spread of the context's own repeated frames.
usage: python tools/ab/ao_filter_timing.py cfg4 [rounds >= 5] [out.json] [--parent-lib PATH]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
parent_lib = None
if "--parent-lib" in argv:
    k = argv.index("--parent-lib")
    parent_lib = os.path.abspath(argv[k + 1])
    del argv[k:k + 2]
step = None
if "--step" in argv:
    k = argv.index("--step")
    step = argv[k + 1]
    del argv[k:k + 2]
wl = argv[0] if len(argv) > 0 else "cfg4"
rounds = max(5, int(argv[1])) if len(argv) > 1 else 20
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "ao_filter_timing.json")
K, N_SETS, RADIUS, BIAS = 4, 64, 2.0, 1e-3
NORMAL_MIN, PLANE_MAX = 0.9, 0.05
STEP_LIMIT_S = {"a": 300, "b": 420, "frame": 240}


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def child(which, env=None):
    """one step in a fresh process under its own time limit; its last line is the step's JSON"""
    text = subprocess.run([sys.executable, os.path.abspath(__file__), wl, str(rounds), "--step", which], env=env, capture_output=True, text=True,
                          timeout=STEP_LIMIT_S[which], check=True).stdout
    print(f"step {which}: done", file=sys.stderr, flush=True)
    return json.loads(text.strip().splitlines()[-1])


if step is None:   # the driver: opens no GPU itself
    import bench
    res = {"what": "rt_ao_filter_device alone (a), rt_render_ao_filtered_device against render_ao + render_gbuffer + the definition in torch ops "
                   "(b), the untouched frame against the parent library in alternating fresh processes (c)",
           "workload": wl, "samples": K, "n_sets": N_SETS, "radius_of_the_rays": RADIUS, "bias": BIAS, "normal_min": NORMAL_MIN,
           "plane_max": PLANE_MAX, "rounds": rounds, "library_sha16": bench.library_sha16(),
           "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
    res["a_filter_alone"] = child("a")
    try:
        with open(os.path.join(ROOT, "profiles", "gbuffer_timing.json")) as f:
            res["a_filter_alone"]["gbuffer_record_kernel_gb_per_s"] = json.load(f)["cases"]["gbuffer_all_outputs"]["record_kernel_gb_per_s"]
    except (OSError, KeyError):
        pass
    res["b_frame_form_against_torch"] = child("b")
    if parent_lib:
        runs = {"frame_parent": [], "frame_this": []}
        for _ in range(3):
            for which, lib in (("frame_this", None), ("frame_parent", parent_lib)):
                env = dict(os.environ)
                env.pop("RT_LIB_OVERRIDE", None)
                if lib:
                    env["RT_LIB_OVERRIDE"] = lib
                runs[which].append(child("frame", env))
        med = {k: statistics.median(r["frame_kernel_ms"]["median_ms"] for r in runs[k]) for k in runs}
        spread = statistics.median(r["frame_kernel_ms"]["max_ms"] - r["frame_kernel_ms"]["best_ms"] for r in runs["frame_this"])
        res["c_untouched_frame"] = {"frame_parent_library": runs["frame_parent"], "frame_this_library": runs["frame_this"],
                                    "frame_spread_ms": spread, "frame_this_minus_parent_median_ms": med["frame_this"] - med["frame_parent"],
                                    "this_library_within_spread_of_parent": bool(abs(med["frame_this"] - med["frame_parent"]) <= spread)}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)

    def brief(v):
        if isinstance(v, dict):
            if "median_ms" in v and "all_ms" in v:
                return round(v["median_ms"], 3)
            return {k: brief(x) for k, x in v.items() if k not in ("frame_parent_library", "frame_this_library")}
        return v
    print(json.dumps(brief(res)))
    sys.exit(0)

# ---- the steps: each its own process ---------------------------------------------------------------------------------------------------
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import ao as AO  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402

desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n = W * H
z = float(camera.camera_z(H))
rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))


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


if step == "frame":   # the frame of whatever library RT_LIB_OVERRIDE names
    d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ms = []
    for _ in range(rounds + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    rt.close()
    print(json.dumps({"library_sha16": bench.library_sha16(), "frame_kernel_ms": summary(ms[1:])}))
    sys.exit(0)

d_dirs = torch.from_numpy(AO.directions(K, N_SETS, RADIUS, seed=K)).cuda()
gb = {"index": torch.empty(n, dtype=torch.int32, device="cuda"), "point": torch.empty((n, 4), dtype=torch.float32, device="cuda"),
      "normal": torch.empty((n, 4), dtype=torch.float32, device="cuda")}
counts = {"unoccluded": torch.empty(n, dtype=torch.uint8, device="cuda")}
out = {"ao": torch.empty(n, dtype=torch.float32, device="cuda")}

if step == "a":
    rt.render_gbuffer(want=("index", "point", "normal"), out=gb)
    rt.render_ao(d_dirs, K, BIAS, want=("unoccluded",), out=counts)
    torch.cuda.synchronize()
    res = {"frame": [W, H], "workload": desc, "bytes_per_item": {"read": 37, "written": 4}}
    for r in (1, 2, 4):
        case, infos = measure(lambda: rt.ao_filter(counts["unoccluded"], gb["point"], gb["normal"], gb["index"], W, K, r, NORMAL_MIN, PLANE_MAX,
                                                   want=("ao",), out=out), rt.ao_filter_info)
        ms = statistics.median(i["filter_ms"] for i in infos)
        case["filter_ms"] = summary([i["filter_ms"] for i in infos])
        case["gb_per_s"] = 41.0 * n / ms / 1e6
        case["counts"] = {k: infos[-1][k] for k in ("n_items", "n_live", "accepted")}
        case["taps_per_live_item"] = infos[-1]["accepted"] / max(1, infos[-1]["n_live"])
        res[f"r{r}"] = case
    rt.close()
    print(json.dumps(res))
    sys.exit(0)

# ---- b: the frame form against render_ao + render_gbuffer + the definition in torch ops --------------------------------------------------
R = 2


def torch_filter():
    """ao.filter on the device with shifted slices: (ao float32[n], taps int32[n])"""
    P, N = gb["point"].view(H, W, 4)[..., :3], gb["normal"].view(H, W, 4)[..., :3]
    live = (gb["index"].view(H, W) >= 0) & torch.isfinite(P).all(dim=2) & torch.isfinite(N).all(dim=2)
    U = counts["unoccluded"].view(H, W).to(torch.int32)
    taps, total = live.to(torch.int32), torch.where(live, U, torch.zeros_like(U))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx == 0 and dy == 0:
                continue
            pr, qr = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
            pc, qc = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
            Np, Nq, Pp, Pq = N[pr, pc], N[qr, qc], P[pr, pc], P[qr, qc]
            c = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
            d = Pq - Pp
            e = (Np[..., 0] * d[..., 0] + Np[..., 1] * d[..., 1]) + Np[..., 2] * d[..., 2]
            ok = live[pr, pc] & live[qr, qc] & (c >= NORMAL_MIN32) & (e.abs() <= PLANE_MAX32)
            taps[pr, pc] += ok
            total[pr, pc] += torch.where(ok, U[qr, qc], torch.zeros_like(U[qr, qc]))
    ao = torch.where(live, total.to(torch.float32) / (taps * K).clamp(min=1).to(torch.float32), torch.ones((), device="cuda"))
    return ao.view(-1), taps.view(-1)


NORMAL_MIN32, PLANE_MAX32 = float(np.float32(NORMAL_MIN)), float(np.float32(PLANE_MAX))
held = {}


def torch_route():
    rt.render_ao(d_dirs, K, BIAS, want=("unoccluded",), out=counts)
    rt.render_gbuffer(want=("index", "point", "normal"), out=gb)
    held["ao"], held["taps"] = torch_filter()


both = {"ao": out["ao"], "taps": torch.empty(n, dtype=torch.uint8, device="cuda")}
res = {"frame": [W, H], "workload": desc, "radius": R}
res["render_ao_filtered"], infos = measure(lambda: rt.render_ao_filtered(d_dirs, K, BIAS, R, NORMAL_MIN, PLANE_MAX, want=("ao", "taps"), out=both),
                                           rt.ao_filter_info)
for key in ("gbuffer_ms", "ao_ms", "filter_ms"):
    res["render_ao_filtered"][key] = summary([i[key] for i in infos])
res["render_ao"], _ = measure(lambda: rt.render_ao(d_dirs, K, BIAS, want=("unoccluded",), out=counts))
res["render_ao_plus_torch_filter"], _ = measure(torch_route)
res["same_results"] = {"taps": bool(torch.equal(held["taps"].to(torch.uint8), both["taps"])),
                       "ao_bits": bool(torch.equal(held["ao"].view(torch.int32), both["ao"].view(torch.int32))),
                       "ao_items_that_differ": int((held["ao"].view(torch.int32) != both["ao"].view(torch.int32)).sum())}
res["speedup_over_torch_route"] = {k: res["render_ao_plus_torch_filter"][k]["median_ms"] / res["render_ao_filtered"][k]["median_ms"]
                                   for k in ("wall_ms", "event_ms")}
res["filter_cost_over_render_ao_ms"] = res["render_ao_filtered"]["event_ms"]["median_ms"] - res["render_ao"]["event_ms"]["median_ms"]
rt.close()
print(json.dumps(res))
