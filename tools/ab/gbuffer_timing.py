#!/usr/bin/env python3
"""G-buffer frames (hip_raytracer.h, "G-buffer frames") on one workload (cfg4: 100 k spheres, 4096^2, depth 3), warmed, medians of 20
after one warm-up call per case, on ONE live shade_and_reflect context in one process:

    render_gbuffer with every output and with t + normal only: wall per call (enqueue + a device synchronise) and trace_ms /
    records_ms of rt_get_gbuffer_info; the bytes the record kernel moves and its rate;
(a) generate_rays + query_hits of the same work-items on the same context (t, index, point, normal): wall, the query's device_ms;
(b) rt_render_aux (the whole shaded frame for a (t, index) pair): wall;
(c) a second RT_KERNEL_HITTEST context: its creation time, and its rt_render_device with aux buffers (wall, kernel ms);
    the pose one box diagonal outside the grid's box: render_gbuffer of the whole posed frame (wall, trace_ms, records_ms,
    tiles_info().source) against (a) for 4 096 of its rays (the query takes brute force there; more would take minutes);
(d) the frame's kernel time before any pass and after all of them on the same context (its own repeated frames: the spread).
With --parent-lib PATH (a library built from the parent commit) child processes that alternate between that library and this one
(RT_LIB_OVERRIDE), three pairs, measure
(e) the untouched frame, parent against this library: only host code on that path changed, so the two must agree within the spread.
usage: python tools/ab/gbuffer_timing.py cfg4 [rounds >= 10] [out.json] [--parent-lib PATH]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import GBUFFER_FIELDS, HIPRaytracer  # noqa: E402

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
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "gbuffer_timing.json")


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

res = {"what": "rt_render_gbuffer_device on one live context: wall per call (enqueue + synchronise), trace_ms and records_ms; beside it "
               "generate_rays + query_hits of the same work-items, rt_render_aux, a second hittest context; a pose outside the grid's box; "
               "the untouched frame against the parent library in alternating fresh processes",
       "workload": desc, "frame": [W, H], "objects": len(objs), "rounds": rounds, "library_sha16": bench.library_sha16(),
       "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n_frame, 4), dtype=torch.float32, device="cuda")
frame_kernel_ms(live, d_frame)
res["frame_untouched_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
shapes = {"t": ((n_frame,), torch.float32), "index": ((n_frame,), torch.int32), "point": ((n_frame, 4), torch.float32),
          "normal": ((n_frame, 4), torch.float32), "albedo": ((n_frame, 4), torch.float32)}
out_all = {k: torch.empty(s, dtype=d, device="cuda") for k, (s, d) in shapes.items()}   # allocated once: the calls measure the pass


def measure_gbuffer(rt, want):
    out = {k: out_all[k] for k in want}
    call = lambda: rt.render_gbuffer(want=want, out=out)  # noqa: E731
    wall_of(call)
    wall, trace, records = [], [], []
    for _ in range(rounds):
        wall.append(wall_of(call))
        info = rt.gbuffer_info()
        trace.append(info["trace_ms"])
        records.append(info["records_ms"])
    info = rt.gbuffer_info()
    written = sum(16 if k in ("point", "normal", "albedo") else 0 for k in want)
    rec_ms = statistics.median(records)
    return {"want": list(want), "wall_ms": summary(wall), "trace_ms": summary(trace), "records_ms": summary(records), "n_items": info["n_items"],
            "hits": info["hits"], "wavefront": info["wavefront"],
            "record_kernel_bytes_per_item": {"read": 8, "written": written},
            "record_kernel_gb_per_s": (8 + written) * info["n_items"] / rec_ms / 1e6 if rec_ms > 0 else None}


cases = {}
cases["gbuffer_all_outputs"] = measure_gbuffer(live, GBUFFER_FIELDS)
cases["gbuffer_t_normal"] = measure_gbuffer(live, ("t", "normal"))


def measure_query(rt, make_rays, want=("t", "index", "point", "normal")):
    """(a): the rays generated and queried, each call; wall, and the query's own device_ms."""
    rays = make_rays()
    out = rt.query_hits(rays, want=want)

    def call():
        r = make_rays()
        rt.query_hits(r, want=want, out=out)
    wall_of(call)
    wall, device = [], []
    for _ in range(rounds):
        wall.append(wall_of(call))
        device.append(rt.query_info()["device_ms"])
    q = rt.query_info()
    return {"want": list(want), "wall_ms": summary(wall), "query_device_ms": summary(device), "n_rays": q["n_rays"], "n_grid": q["n_grid"],
            "n_brute": q["n_brute"]}


frame_rays_buffer = torch.empty((n_frame, 8), dtype=torch.float32, device="cuda")
cases["a_generate_rays_plus_query_hits"] = measure_query(live, lambda: live.generate_rays(W, H, z, np.eye(3), out=frame_rays_buffer))

# (b) rt_render_aux: the whole shaded frame, a (t, index) pair copied to the host
wall_of(live.render_aux)
cases["b_render_aux"] = {"wall_ms": summary([wall_of(live.render_aux) for _ in range(max(5, rounds // 4))])}

# (c) a second hittest context
t0 = time.perf_counter()
second = HIPRaytracer(objs, lights, None, 0, kernel="hittest", camera=(W, H, z))
torch.cuda.synchronize()
create_ms = (time.perf_counter() - t0) * 1e3
d_t = torch.empty(n_frame, dtype=torch.float32, device="cuda")
d_aux_t, d_aux_i = torch.empty(n_frame, dtype=torch.float32, device="cuda"), torch.empty(n_frame, dtype=torch.int32, device="cuda")
import ctypes  # noqa: E402


def second_frame():
    second._check(second._lib.rt_set_aux_device(second._ctx, ctypes.c_void_p(d_aux_t.data_ptr()), ctypes.c_void_p(d_aux_i.data_ptr())))
    second.render_device(d_t.data_ptr(), 0)


wall_of(second_frame)
wall, kern = [], []
for _ in range(rounds):
    wall.append(wall_of(second_frame))
    kern.append(float(second.stats().last_kernel_ms))
cases["c_second_hittest_context"] = {"create_ms": create_ms, "render_device_with_aux_wall_ms": summary(wall), "kernel_ms": summary(kern)}
second.close()

# the pose one box diagonal outside the grid's box
info = live.rays_info()
lo, hi = info["box_lo"], info["box_hi"]
centre, diag = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
o = centre + np.array([0.0, 0.15, 0.1]) * diag
o[0] = hi[0] + diag
o = o.astype(np.float32)
pz = float(np.float32(-0.5 * max(W, H) * np.linalg.norm(o - centre) / (0.5 * diag)))
M = camera.look_at(o, centre)
live.set_pose(W, H, pz, M, o)
off = {"origin": o.tolist(), "z": pz}
off["gbuffer_all_outputs"] = measure_gbuffer(live, GBUFFER_FIELDS)
off["tiles_source"] = int(live.tiles_info()["source"])
off["primary_outside_box"] = int(live.rays_info()["primary_outside_box"])
posed = live.generate_rays(W, H, pz, M, o)
gen = torch.Generator(device="cuda").manual_seed(7)
picked = torch.randperm(n_frame, generator=gen, device="cuda")[:4096].sort().values
some = posed[picked].contiguous()
del posed
q_out = live.query_hits(some, want=("t", "index", "point", "normal"))
q_wall = [wall_of(lambda: live.query_hits(some, want=("t", "index", "point", "normal"), out=q_out)) for _ in range(3)]
q = live.query_info()
off["a_query_hits_of_4096_of_its_rays"] = {"wall_ms": summary(q_wall), "device_ms": q["device_ms"], "n_grid": q["n_grid"], "n_brute": q["n_brute"],
                                           "ms_per_ray": q["device_ms"] / 4096.0,
                                           "whole_frame_at_that_rate_s": q["device_ms"] / 4096.0 * n_frame / 1e3}
g_idx = out_all["index"][picked]
off["agrees_on_index_with_the_query"] = bool(torch.equal(g_idx, q_out["index"]))
cases["off_box_pose"] = off
live.set_camera(W, H, z)

res["cases"] = cases
res["frame_after_the_passes_ms"] = summary([frame_kernel_ms(live, d_frame) for _ in range(rounds)])
live.close()
spread = res["frame_untouched_ms"]["max_ms"] - res["frame_untouched_ms"]["best_ms"]
res["frame_spread_ms"] = spread
res["frame_after_minus_untouched_median_ms"] = res["frame_after_the_passes_ms"]["median_ms"] - res["frame_untouched_ms"]["median_ms"]
g_wall = cases["gbuffer_all_outputs"]["wall_ms"]["median_ms"]
res["speedup_of_the_pass"] = {"over_a_generate_rays_plus_query_hits": cases["a_generate_rays_plus_query_hits"]["wall_ms"]["median_ms"] / g_wall,
                              "over_b_render_aux": cases["b_render_aux"]["wall_ms"]["median_ms"] / g_wall}

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


def brief(v):
    if isinstance(v, dict):
        if "median_ms" in v and "all_ms" in v:
            return v["median_ms"]
        return {k: brief(x) for k, x in v.items()}
    return v


print(json.dumps({"cases": brief(cases), "speedup_of_the_pass": res["speedup_of_the_pass"], "frame_untouched_ms": res["frame_untouched_ms"]["median_ms"],
                  "frame_spread_ms": spread, "frame_after_minus_untouched_median_ms": res["frame_after_minus_untouched_median_ms"],
                  "frame_this_minus_parent_median_ms": res.get("frame_this_minus_parent_median_ms"),
                  "this_library_within_spread_of_parent": res.get("this_library_within_spread_of_parent")}))
