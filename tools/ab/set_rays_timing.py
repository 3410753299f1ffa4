#!/usr/bin/env python3
"""Replaceable rays (hip_raytracer.h) on one workload (cfg3 or cfg4: 4096^2, 16.7 M rays, 537 MB of rays), ONE process:

1. rt_set_rays_device on a device tensor: wall of the whole call, and inside it the device time of the scan kernel
   (csrc/rt_rays.hip) and of the library's device-to-device copy (RT_RAYS_TRACE=1: an event pair each, read from stderr);
2. the runtime's device-to-device copy of the same buffer from the caller's side (torch), timed with events in the same run:
   the scan reads the buffer once and writes nothing, the copy reads and writes it - the scan should not take longer;
3. rt_set_rays (the host twin: 537 MB host-to-device, then the same route);
4. the only route to the same frame before this entry point: rt_destroy + rt_create with the host array (RT_FLAG_NO_RAYGEN);
5. the frame's kernel time rendered from the buffer, beside the pinhole frame's on the same context.
The rays are the workload's pinhole grid panned about the origin (rays.posed_rays).
usage: python tools/ab/set_rays_timing.py cfg3|cfg4 [repeats >= 5] [out.json]"""
import json, os, re, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera, rays as RY  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402

wl = sys.argv[1]
repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def rotation(yaw, pitch, roll):
    def axis(a, k):
        c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][k]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return axis(yaw, 1) @ axis(pitch, 0) @ axis(roll, 2)


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


def frame_kernel_ms(rt, d_frame, n=5):
    ms = []
    for _ in range(n + 1):
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return summary(ms[1:])


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n = W * H
z = float(camera.camera_z(H))
pan = RY.posed_rays(W, H, z, rotation(12, -7, 30))
result = {"what": "rt_set_rays_device / rt_set_rays on a live context against rt_destroy + rt_create with the host array; device time of the "
                  "scan kernel and of the copies; kernel time of the frame from the buffer and from the pinhole camera",
          "workload": desc, "frame": [W, H], "rays": n, "ray_bytes": 32 * n, "repeats": repeats, "library_sha16": bench.library_sha16(),
          "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
result["frame_kernel_ms_pinhole"] = frame_kernel_ms(rt, d_frame)
d_rays = torch.from_numpy(pan.view(np.float32).reshape(-1, 8)).cuda()
other = torch.empty_like(d_rays)
torch.cuda.synchronize()

os.environ["RT_RAYS_TRACE"] = "1"
walls, scans, copies, torch_copies = [], [], [], []
for rep in range(repeats + 1):
    def call():
        t0 = time.perf_counter()
        rt.set_rays(d_rays)
        return (time.perf_counter() - t0) * 1e3
    wall, err = stderr_of(call)
    m = re.search(r"\[rt_set_rays\] scan ([0-9.]+) ms copy ([0-9.]+) ms", err)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    other.copy_(d_rays)
    b.record()
    b.synchronize()
    if rep:   # (the first round is the warm-up: the context's ray buffer is allocated there)
        walls.append(wall)
        scans.append(float(m.group(1)))
        copies.append(float(m.group(2)))
        torch_copies.append(a.elapsed_time(b))
os.environ.pop("RT_RAYS_TRACE")
result["set_rays_device_wall_ms"] = summary(walls)
result["scan_kernel_ms"] = summary(scans)
result["library_copy_ms"] = summary(copies)
result["runtime_copy_ms_torch"] = summary(torch_copies)
result["scan_TB_per_s_best"] = 32 * n / (min(scans) * 1e-3) / 1e12
result["copy_TB_per_s_best_read_plus_written"] = 64 * n / (min(torch_copies) * 1e-3) / 1e12
result["scan_not_slower_than_the_copy"] = bool(statistics.median(scans) <= statistics.median(torch_copies))
info = rt.rays_info()
result["rays_info"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in info.items()}
result["frame_kernel_ms_buffer"] = frame_kernel_ms(rt, d_frame)

host_walls = []
for rep in range(4):
    t0 = time.perf_counter()
    rt.set_rays(pan)
    host_walls.append((time.perf_counter() - t0) * 1e3)
result["set_rays_host_wall_ms"] = summary(host_walls[1:])
rt.close()

recreate = []
for rep in range(3):
    old = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z)) if rep == 0 else new
    t0 = time.perf_counter()
    old.close()
    new = HIPRaytracer(objs, lights, pan, depth, kernel=kernel, raygen=False)
    recreate.append((time.perf_counter() - t0) * 1e3)
result["destroy_create_wall_ms"] = summary(recreate)
result["create_setup_times_ms"] = new.setup_times()
new.close()
for k in ("frame_kernel_ms_pinhole", "frame_kernel_ms_buffer", "scan_kernel_ms", "library_copy_ms", "runtime_copy_ms_torch", "set_rays_device_wall_ms",
          "set_rays_host_wall_ms", "destroy_create_wall_ms"):
    print(f"{wl} {k:28s} best {result[k]['best_ms']:9.3f}  median {result[k]['median_ms']:9.3f} ms", flush=True)
print(f"{wl} scan {result['scan_TB_per_s_best']:.2f} TB/s read; copy {result['copy_TB_per_s_best_read_plus_written']:.2f} TB/s read + written; "
      f"grid_in_use {info['grid_in_use']}", flush=True)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(result, f, indent=1)
