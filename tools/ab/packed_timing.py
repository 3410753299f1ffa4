#!/usr/bin/env python3
"""8-bit frames against the float frame, cfg3 and cfg4, ONE process per run, the settings alternating call by call:

1. wall clock of rt_render (float) - must reproduce bench.py's render_wall_ms_incl_d2h of the same box;
2. wall clock of rt_render_packed, RGBA8 and RGB8; for cfg4 also under RT_RENDER_PASSES=1 and several RT_RENDER_SPLIT
   settings (both variables are read per call);
3. device time of the pack pass alone on a resident 4096^2 frame (HIP events around `inner` back-to-back rt_pack_device calls)
   as bytes read + written per second - four pixels per lane (RT_PACK_LANE_PIXELS=4) and one (RGBA8 only, RT_PACK_LANE_PIXELS=1) -
   beside a device-to-device copy of the float frame timed the same way in the same run (torch's Tensor.copy_, which for
   contiguous tensors of one type on one device is hipMemcpyAsync device-to-device).

Walls are through the C ABI without the Python wrapper's numpy copy. The multi-GPU exchange is NOT measured (one-GPU box).
usage: python tools/ab/packed_timing.py [repeats >= 5] [out.json]"""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer, pixel_format  # noqa: E402

repeats = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
KNOBS = ("RT_RENDER_PASSES", "RT_RENDER_SPLIT", "RT_PACK_LANE_PIXELS")


def with_env(env, fn):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "all_ms": ms}


def wall_settings(wl):
    s = [("float", None, {}), ("rgba8", "rgba8", {}), ("rgb8", "rgb8", {})]
    if wl == "cfg4":
        s += [("float passes=1", None, {"RT_RENDER_PASSES": "1"}), ("rgba8 passes=1", "rgba8", {"RT_RENDER_PASSES": "1"}),
              ("rgb8 passes=1", "rgb8", {"RT_RENDER_PASSES": "1"})]
        s += [(f"rgba8 split {sp}", "rgba8", {"RT_RENDER_SPLIT": sp}) for sp in ("1,1", "3,1", "7,1", "15,1")]
    return s


result = {"what": "wall ms of rt_render / rt_render_packed through the C ABI (no numpy copy) and device time of the pack pass; settings "
                  "alternate call by call in one process; the multi-GPU exchange is not measured (one-GPU box)",
          "repeats": repeats, "library_sha16": bench.library_sha16(), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
for wl in ("cfg3", "cfg4"):
    desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, float(camera.camera_z(H))))
    lib, ctx = rt._lib, rt._ctx
    f_out, b_out = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_uint8)()

    def call(fmt):
        rc = lib.rt_render(ctx, ctypes.byref(f_out)) if fmt is None else lib.rt_render_packed(ctx, pixel_format(fmt), ctypes.byref(b_out))
        rt._check(rc)

    settings = wall_settings(wl)
    for _ in range(2):  # warm-up: buffers, screen tiles, pinned frames
        for _, fmt, env in settings:
            with_env(env, lambda: call(fmt))
    ms = {name: [] for name, _, _ in settings}
    for _ in range(repeats):
        for name, fmt, env in settings:
            def timed():
                t0 = time.perf_counter()
                call(fmt)
                return (time.perf_counter() - t0) * 1e3
            ms[name].append(with_env(env, timed))
    entry = {"workload": desc, "kernel_ms_last_launch_float": None, "wall": {name: summary(v) for name, v in ms.items()}}
    call(None)
    entry["kernel_ms_last_launch_float"] = float(rt.stats().last_kernel_ms)
    fl = entry["wall"]["float"]
    entry["rgba8_below_float_by_more_than_float_spread"] = bool(fl["best_ms"] - entry["wall"]["rgba8"]["best_ms"] > fl["spread_ms"])
    for name, v in entry["wall"].items():
        print(f"{wl} {name:18s} best {v['best_ms']:8.3f}  median {v['median_ms']:8.3f}  spread {v['spread_ms']:6.3f} ms", flush=True)
    if wl == "cfg4":  # the pass alone, on this frame resident in device memory
        n = W * H
        frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        other = torch.empty_like(frame)
        out = torch.empty((n * 4,), dtype=torch.uint8, device="cuda")
        rt.render_device(frame.data_ptr(), 0)
        torch.cuda.synchronize()
        inner = 5
        kinds = {"pack rgba8 (4 pixels per lane)": ("rgba8", {"RT_PACK_LANE_PIXELS": "4"}, 20), "pack rgba8 (1 pixel per lane)": ("rgba8", {"RT_PACK_LANE_PIXELS": "1"}, 20),
                 "pack rgb8 (4 pixels per lane)": ("rgb8", {}, 19), "device-to-device copy of the float frame": (None, {}, 32)}

        def device_ms(fmt, env):
            def run():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(inner):
                    if fmt is None: other.copy_(frame)
                    else: rt.pack_device(frame.data_ptr(), n, out.data_ptr(), fmt, 0)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / inner
            return with_env(env, run)

        dev = {k: [] for k in kinds}
        for rep in range(repeats + 1):
            for k, (fmt, env, _) in kinds.items():
                t = device_ms(fmt, env)
                if rep: dev[k].append(t)   # (the first round is the warm-up)
        entry["pack_pass"] = {"pixels": n, "inner_calls_per_event_pair": inner}
        for k, (_, _, bytes_per_pixel) in kinds.items():
            s = summary(dev[k])
            s["bytes_per_pixel"] = bytes_per_pixel
            s["TB_per_s_best"] = n * bytes_per_pixel / (s["best_ms"] * 1e-3) / 1e12
            entry["pack_pass"][k] = s
            print(f"{wl} {k:42s} best {s['best_ms']:.4f} ms  {s['TB_per_s_best']:.3f} TB/s (read + written)", flush=True)
        entry["pack_rate_not_below_copy_rate"] = bool(entry["pack_pass"]["pack rgba8 (1 pixel per lane)"]["TB_per_s_best"] >=
                                                      entry["pack_pass"]["device-to-device copy of the float frame"]["TB_per_s_best"])
        del frame, other, out
    result[wl] = entry
    rt.close()
print("acceptance:", {wl: result[wl]["rgba8_below_float_by_more_than_float_spread"] for wl in ("cfg3", "cfg4")},
      "pack >= copy rate:", result["cfg4"]["pack_rate_not_below_copy_rate"], flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
