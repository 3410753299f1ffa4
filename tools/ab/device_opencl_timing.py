#!/usr/bin/env python3
"""Frame time of cfg3 and cfg4 with and without RT_FLAG_DEVICE_OPENCL (HIPRaytracer(device_opencl=...)), alternating the two
contexts frame by frame; device time per frame from the library's HIP events (rt_timing_summary, as bench.py's kernel_ms).
usage: python tools/ab/device_opencl_timing.py [frames] [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from opencl_raytracer_amd import camera
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 10
result = {"what": "frame device ms (mean over the frames), HIP events around the render's kernels; default flags vs RT_FLAG_DEVICE_OPENCL",
          "frames": frames, "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
for wl in ("cfg3", "cfg4"):
    desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
    cam = (W, H, float(camera.camera_z(H)))
    ctx = {flag: HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=cam, device_opencl=flag) for flag in (False, True)}
    for rt in ctx.values():
        rt.Render()  # warm-up
        rt.timing_reset()
    for _ in range(frames):
        for rt in ctx.values():
            rt.Render()
    ms = {}
    for flag, rt in ctx.items():
        total, n = rt.timing_summary()
        ms[flag] = total / max(n, 1)
        rt.close()
    result[wl] = {"workload": desc, "default_ms": ms[False], "device_opencl_ms": ms[True]}
    print(wl, f"default {result[wl]['default_ms']:.3f} ms, device_opencl {result[wl]['device_opencl_ms']:.3f} ms", flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
