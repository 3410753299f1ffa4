#!/usr/bin/env python3
"""Supersampled frames against the unfiltered sample frame, ONE process per workload (cfg3 or cfg4, sample grid 4096^2), the
settings alternating call by call:

1. wall clock of rt_render (float) and rt_render_packed (RGBA8) with factor 1 - the whole sample frame crosses the bus, the way to
   these samples before the filter existed (its host-side filter not even counted) - and with factor 2 on the SAME context;
2. for a frame that goes through rt_render's passes (cfg4): factor 2 under RT_RENDER_PASSES=1 and several RT_RENDER_SPLIT settings
   (both variables are read per call) - the table the default split of a filtered frame is chosen from;
3. device time of the filter alone on the resident sample frame (HIP events around `inner` back-to-back rt_resolve_device calls) as
   bytes read + written per second, per factor, output and kernel form (RT_RESOLVE_FORM, read per call), beside a device-to-device
   copy of that frame timed the same way in the same run. Factor 3 filters the 4095 x 4095 corner of the buffer.

With RT_LIB_OVERRIDE naming a library from before supersampled frames only the factor-1 rows are measured (the "nothing else
moved" comparison). Walls are through the C ABI without the Python wrapper's numpy copy. NOT measured (one-GPU box): the exchange
of filtered tiles between GPUs.
usage: python tools/ab/supersample_timing.py cfg3|cfg4 [repeats >= 5] [out.json]"""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer, pixel_format  # noqa: E402

wl = sys.argv[1]
repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
KNOBS = ("RT_RENDER_PASSES", "RT_RENDER_SPLIT", "RT_RESOLVE_FORM")


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


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, float(camera.camera_z(H))))
lib, ctx = rt._lib, rt._ctx
have = hasattr(lib, "rt_set_supersampling")
f_out, b_out = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_uint8)()


def call(fmt, s):
    if have:
        rt._check(lib.rt_set_supersampling(ctx, s))
    rt._check(lib.rt_render(ctx, ctypes.byref(f_out)) if fmt is None else lib.rt_render_packed(ctx, pixel_format(fmt), ctypes.byref(b_out)))


settings = [("float s=1", None, 1, {}), ("rgba8 s=1", "rgba8", 1, {})]
if have:
    settings += [("float s=2", None, 2, {}), ("rgba8 s=2", "rgba8", 2, {})]
    if wl == "cfg4":
        for name, fmt in (("float", None), ("rgba8", "rgba8")):
            settings.append((f"{name} s=2 passes=1", fmt, 2, {"RT_RENDER_PASSES": "1"}))
            settings += [(f"{name} s=2 split {sp}", fmt, 2, {"RT_RENDER_SPLIT": sp}) for sp in ("1,1", "3,1", "7,1", "15,1")]
result = {"what": "wall ms of rt_render / rt_render_packed through the C ABI (no numpy copy) with supersampling factor 1 and 2 on one context, "
                  "and device time of the filter alone; settings alternate call by call in one process; the exchange between GPUs is not "
                  "measured (one-GPU box)",
          "workload": desc, "sample_grid": [W, H], "repeats": repeats, "library_sha16": bench.library_sha16(),
          "library_has_supersampling": have, "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
for _ in range(2):  # warm-up: buffers, screen tiles, pinned frames
    for _, fmt, s, env in settings:
        with_env(env, lambda: call(fmt, s))
ms = {name: [] for name, _, _, _ in settings}
for _ in range(repeats):
    for name, fmt, s, env in settings:
        def timed():
            if have:
                rt._check(lib.rt_set_supersampling(ctx, s))
            t0 = time.perf_counter()
            rt._check(lib.rt_render(ctx, ctypes.byref(f_out)) if fmt is None else lib.rt_render_packed(ctx, pixel_format(fmt), ctypes.byref(b_out)))
            return (time.perf_counter() - t0) * 1e3
        ms[name].append(with_env(env, timed))
result["wall"] = {name: summary(v) for name, v in ms.items()}
for name, v in result["wall"].items():
    print(f"{wl} {name:26s} best {v['best_ms']:8.3f}  median {v['median_ms']:8.3f}  spread {v['spread_ms']:6.3f} ms", flush=True)
if have:
    rt._check(lib.rt_set_supersampling(ctx, 1))
    call(None, 1)
    result["kernel_ms_last_launch_s1"] = float(rt.stats().last_kernel_ms)
    call(None, 2)
    result["kernel_ms_last_launch_s2"] = float(rt.stats().last_kernel_ms)   # the render's kernels: the filter is behind the event pair
    rt._check(lib.rt_set_supersampling(ctx, 1))
    w = result["wall"]
    for name in ("float", "rgba8"):
        one, two = w[f"{name} s=1"], w[f"{name} s=2"]
        result[f"{name}_gain_ms_best"] = one["best_ms"] - two["best_ms"]
        result[f"{name}_s2_faster_by_more_than_s1_spread"] = bool(one["best_ms"] - two["best_ms"] > one["spread_ms"])
        result[f"{name}_s2_not_slower_beyond_s1_spread"] = bool(two["best_ms"] <= one["best_ms"] + one["spread_ms"])
    # the filter alone, on this sample frame resident in device memory
    n = W * H
    frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    other = torch.empty_like(frame)
    out = torch.empty((n // 4, 4), dtype=torch.float32, device="cuda")
    rt.render_device(frame.data_ptr(), 0)
    torch.cuda.synchronize()
    inner = 5
    out_bytes = {None: 16, "rgba8": 4, "rgb8": 3}
    kinds = {"device-to-device copy of the sample frame": None}
    for s in (2, 3, 4):
        for fmt in (None, "rgba8", "rgb8"):
            for form in ("pixel", "sample"):
                kinds[f"s={s} {fmt or 'float'} lane per {form}"] = (s, fmt, form)

    def device_ms(kind):
        def run():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                if kind is None: other.copy_(frame)
                else:
                    s, fmt, _ = kind
                    rt.resolve_device(frame.data_ptr(), W // s * s, H // s * s, s, out.data_ptr(), fmt, 0)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / inner
        return with_env({} if kind is None else {"RT_RESOLVE_FORM": kind[2]}, run)

    dev = {k: [] for k in kinds}
    for rep in range(repeats + 1):
        for k, kind in kinds.items():
            t = device_ms(kind)
            if rep: dev[k].append(t)   # (the first round is the warm-up)
    result["filter_pass"] = {"inner_calls_per_event_pair": inner}
    for k, kind in kinds.items():
        sm = summary(dev[k])
        if kind is None:
            pixels, per_pixel = n, 32
        else:
            s, fmt, _ = kind
            pixels, per_pixel = (W // s) * (H // s), 16 * s * s + out_bytes[fmt]
        sm["pixels"], sm["bytes_per_pixel"] = pixels, per_pixel
        sm["TB_per_s_best"] = pixels * per_pixel / (sm["best_ms"] * 1e-3) / 1e12
        sm["TB_per_s_median"] = pixels * per_pixel / (sm["median_ms"] * 1e-3) / 1e12
        sm["TB_per_s_worst"] = pixels * per_pixel / (sm["max_ms"] * 1e-3) / 1e12
        result["filter_pass"][k] = sm
        print(f"{wl} {k:44s} best {sm['best_ms']:.4f} ms  median {sm['median_ms']:.4f}  {sm['TB_per_s_best']:.3f} TB/s (read + written)", flush=True)
    cp = result["filter_pass"]["device-to-device copy of the sample frame"]
    result["copy_rate_spread_TB_per_s"] = cp["TB_per_s_best"] - cp["TB_per_s_worst"]
rt.close()
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(result, f, indent=1)
