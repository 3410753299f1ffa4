#!/usr/bin/env python3
"""Replaceable lights (hip_raytracer.h) on one workload (cfg4: 100 k spheres, 32 lights, 4096^2, depth 3), ONE process, warmed,
the routes alternating round by round, the last light moved a little every round:

(a) rt_set_lights on a live context: wall of the whole call and rt_light_tiles_info_t::build_device_ms (events around the
    device builder's four stages, csrc/rt_light_tiles.hip);
(b) a FRESH context with the same lights - what a caller pays today: create_ms and light_tiles_ms (the host's build_light_tiles)
    of rt_get_setup_times, plus the wall of constructing it;
(c) the frame's kernel time after rt_set_lights (device-built table) against the fresh context's (host-built table), with the
    tables' shapes (T, entries, blocks, longest list) beside them;
(d) the frame after rt_set_lights with RT_LIGHT_TILES_DEVICE=0: no table, the grid walk serves the last light - what a moving
    light would cost per frame without the builder.
Walls are host clocks around calls that end in a device synchronise; every figure is given as best / median / max and all rounds.
usage: python tools/ab/set_lights_timing.py cfg4 [rounds >= 20] [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
rounds = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "set_lights_timing.json")


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def frame_kernel_ms(rt, d_frame, n=3):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return statistics.median(ms[1:])


def table(info):
    return {k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in info.items()
            if k in ("enabled", "source", "tiles_u", "n_entries", "n_blocks", "max_list", "refused", "build_device_ms")}


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n = W * H
z = float(camera.camera_z(H))


def moved(rnd):
    lts = lights.copy()
    lts["position"][-1][:3] += np.float32(0.05 * rnd) * np.array([1.0, 0.5, -0.25], dtype=np.float32)
    return lts


res = {"what": "rt_set_lights on a live context against a fresh context per light change, and the frames behind the device-built table, "
               "the host-built table and no table (RT_LIGHT_TILES_DEVICE=0); one process, warmed, alternating round by round",
       "workload": desc, "frame": [W, H], "rays": n, "rounds": rounds, "library_sha16": bench.library_sha16(),
       "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
os.environ.pop("RT_LIGHT_TILES_DEVICE", None)
live = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
res["frame_kernel_ms_as_created"] = frame_kernel_ms(live, d_frame)
res["table_as_created"] = table(live.light_tiles_info())
rows = {k: [] for k in ("set_lights_wall_ms", "build_device_ms", "fresh_wall_ms", "fresh_create_ms", "fresh_light_tiles_ms",
                        "frame_device_table_ms", "frame_host_table_ms", "set_lights_no_table_wall_ms", "frame_no_table_ms")}
tables = {}
for rnd in range(rounds + 1):   # round 0 warms up: the builder's buffers, code objects
    lts = moved(rnd)
    # (a) + (c): the live context
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    live.set_lights(lts)
    wall = (time.perf_counter() - t0) * 1e3
    info = live.light_tiles_info()
    f_dev = frame_kernel_ms(live, d_frame)
    # (d): the same lights, no table
    os.environ["RT_LIGHT_TILES_DEVICE"] = "0"
    t0 = time.perf_counter()
    live.set_lights(lts)
    wall_off = (time.perf_counter() - t0) * 1e3
    info_off = live.light_tiles_info()
    f_off = frame_kernel_ms(live, d_frame)
    os.environ.pop("RT_LIGHT_TILES_DEVICE")
    # (b) + (c): what a caller pays today
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = HIPRaytracer(objs, lts, None, depth, kernel=kernel, camera=(W, H, z))
    wall_fresh = (time.perf_counter() - t0) * 1e3
    setup = fresh.setup_times()
    info_host = fresh.light_tiles_info()
    f_host = frame_kernel_ms(fresh, d_frame)
    fresh.close()
    if rnd == 0:
        continue
    rows["set_lights_wall_ms"].append(wall)
    rows["build_device_ms"].append(float(info["build_device_ms"]))
    rows["fresh_wall_ms"].append(wall_fresh)
    rows["fresh_create_ms"].append(float(setup["create_ms"]))
    rows["fresh_light_tiles_ms"].append(float(setup["light_tiles_ms"]))
    rows["frame_device_table_ms"].append(f_dev)
    rows["frame_host_table_ms"].append(f_host)
    rows["set_lights_no_table_wall_ms"].append(wall_off)
    rows["frame_no_table_ms"].append(f_off)
    tables = {"device": table(info), "host": table(info_host), "off": table(info_off)}
live.close()
res.update({k: summary(v) for k, v in rows.items()})
res["tables_last_round"] = tables
dev, host = res["frame_device_table_ms"], res["frame_host_table_ms"]
spread = max(dev["max_ms"] - dev["best_ms"], host["max_ms"] - host["best_ms"])
res["frame_device_minus_host_median_ms"] = dev["median_ms"] - host["median_ms"]
res["frame_spread_ms"] = spread
res["device_table_frame_not_slower_beyond_spread"] = bool(dev["median_ms"] - host["median_ms"] <= spread)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items() if k not in ("what",)}, indent=1))
