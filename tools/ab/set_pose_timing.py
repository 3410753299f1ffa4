#!/usr/bin/env python3
"""Posed cameras (hip_raytracer.h) on one workload (cfg4: 4096^2, 16.7 M rays, 537 MB of rays), ONE process, the three routes to
the same ray buffer alternating round by round:

1. rt_set_pose: wall of the whole call, and inside it the device time of the verdict kernel and of the generation kernel
   (csrc/rt_raygen.hip; RT_RAYS_TRACE=1: an event pair each, read from stderr) - 537 MB written, nothing read;
2. the device route without it: the same rays computed with torch on the GPU in posed_rays' rounding order (checked bit for bit
   against the generator here), then rt_set_rays_device (the scan reads 537 MB, the copy reads and writes 537 MB) - the torch
   kernels and the call timed separately and together;
3. the host route: rays.posed_rays (numpy) + rt_set_rays (537 MB host-to-device, then the device route), fewer rounds;
4. the kernel time of the cfg4 frame from the posed buffer (identity pose: the same rays) beside the rt_set_camera frame's on the
   same context - what the primary-tile kernel, which needs the fixed camera, is worth.
Walls are host clocks around calls that end in a device synchronise. usage: python tools/ab/set_pose_timing.py cfg4 [repeats >= 5] [out.json]

With a fourth argument "tiles" (python tools/ab/set_pose_timing.py cfg4 7 profiles/pose_tiles_timing.json tiles) the script measures
instead what a viewer pays per frame when the pose changes before EVERY frame, with and without the pose's screen tiles
(csrc/rt_tiles.hip; RT_POSE_TILES=0 is the parent commit's route): the panned pose (its yaw moves a little every round) and the
identity pose, the two settings of the knob alternating round by round in this one process, medians of >= 7 rounds after a warm-up
round. Per frame: the wall of rt_set_pose, the tile build (device events: rt_tiles_info_t::build_device_ms; wall: the
rt_get_tiles_info call that builds), the frame's kernel time, and their sum; the rt_set_camera frame beside them; the knob's 0
position against profiles/set_pose_timing.json; and the verdict the default rests on (build + frame with tiles below the sum
without, by more than the spread between the rounds of one setting)."""
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
host_repeats = 3


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


def torch_posed_rays(W, H, z, M, origin, out):
    """rays.posed_rays on the GPU with torch's elementwise kernels, every product and sum a kernel of its own (nothing fused), into
    the (H, W, 8) view of `out`."""
    f32 = dict(dtype=torch.float32, device=out.device)
    half_w, half_h = np.float32(np.float32(W) / np.float32(2.0)), np.float32(np.float32(H) / np.float32(2.0))
    x = torch.arange(W, **f32) - float(half_w)
    y = (float(np.float32(H)) - torch.arange(H, **f32)) - float(half_h)
    Mf = np.asarray(M, dtype=np.float64).astype(np.float32)
    zf = np.float32(z)
    v = out.view(H, W, 8)
    for r in range(3):
        acc = (x * float(Mf[r, 0]))[None, :] + (y * float(Mf[r, 1]))[:, None]
        v[:, :, 4 + r] = acc + float(np.float32(Mf[r, 2] * zf))
    o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    for k in range(3):
        v[:, :, k] = float(o[k])
    v[:, :, 3] = 1.0
    v[:, :, 7] = 0.0


desc, objs, lights, W, H, kernel, depth = bench.load_workload(wl)
n = W * H
z = float(camera.camera_z(H))
M, origin = rotation(12, -7, 30), (0.0, 0.0, 0.0)


def pose_tiles_timing(out_path):
    rounds = max(7, repeats)
    res = {"what": "a pose changed before every frame, with the pose's screen tiles built on the device (RT_POSE_TILES=1) and without "
                   "(RT_POSE_TILES=0, the parent commit's route), alternating round by round in one process; per frame: rt_set_pose wall, "
                   "tile build (device events and wall), frame kernel time, their sum",
           "workload": desc, "frame": [W, H], "rays": n, "rounds": rounds, "library_sha16": bench.library_sha16(),
           "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
    d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    res["frame_kernel_ms_pinhole"] = frame_kernel_ms(rt, d_frame)
    res["tiles_info_pinhole"] = rt.tiles_info()
    rows = {(knob, pose): {"set_pose_wall_ms": [], "build_wall_ms": [], "build_device_ms": [], "frame_kernel_ms": [], "sum_ms": []}
            for knob in "01" for pose in ("pan", "identity")}
    infos = {}
    for rnd in range(rounds + 1):   # round 0 warms up: buffers, the spheres' upload, code objects
        for knob in "01":
            os.environ["RT_POSE_TILES"] = knob
            for pose in ("pan", "identity"):
                Mp = rotation(12 + 0.05 * rnd, -7, 30) if pose == "pan" else np.eye(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rt.set_pose(W, H, z, Mp, origin)
                t1 = time.perf_counter()
                info = rt.tiles_info()   # builds the table of the new pose (knob 0: refuses at once)
                t2 = time.perf_counter()
                rt.render_device(d_frame.data_ptr(), 0)
                torch.cuda.synchronize()
                k_ms = float(rt.stats().last_kernel_ms)
                infos[(knob, pose)] = info
                if rnd:
                    r = rows[(knob, pose)]
                    r["set_pose_wall_ms"].append((t1 - t0) * 1e3)
                    r["build_wall_ms"].append((t2 - t1) * 1e3)
                    r["build_device_ms"].append(info["build_device_ms"])
                    r["frame_kernel_ms"].append(k_ms)
                    r["sum_ms"].append((t2 - t0) * 1e3 + k_ms)
    os.environ.pop("RT_POSE_TILES")
    rt.set_camera(W, H, z)
    res["frame_kernel_ms_pinhole_after"] = frame_kernel_ms(rt, d_frame)
    rt.close()
    before = {}
    try:
        with open(os.path.join(ROOT, "profiles", "set_pose_timing.json")) as f:
            old = json.load(f)
        before = {"pan": old["frame_kernel_ms_posed_pan"], "identity": old["frame_kernel_ms_posed_identity"], "pinhole": old["frame_kernel_ms_pinhole"]}
    except (OSError, KeyError, ValueError):
        pass
    res["profiles_set_pose_timing_json"] = before
    for pose in ("pan", "identity"):
        off, on = rows[("0", pose)], rows[("1", pose)]
        entry = {"without_tiles": {k: summary(v) for k, v in off.items()}, "with_tiles": {k: summary(v) for k, v in on.items()},
                 "tiles_info_with": infos[("1", pose)], "tiles_info_without": infos[("0", pose)]}
        spread = max(max(off["sum_ms"]) - min(off["sum_ms"]), max(on["sum_ms"]) - min(on["sum_ms"]))
        gain = statistics.median(off["sum_ms"]) - statistics.median(on["sum_ms"])
        entry["sum_gain_median_ms"] = gain
        entry["sum_spread_between_rounds_ms"] = spread
        entry["tiles_pay"] = bool(gain > spread)
        pin = res["frame_kernel_ms_pinhole"]["median_ms"]
        gap = statistics.median(off["frame_kernel_ms"]) - pin
        entry["frame_gap_to_pinhole_without_ms"] = gap
        entry["frame_gap_to_pinhole_with_ms"] = statistics.median(on["frame_kernel_ms"]) - pin
        entry["gap_recovered_by_the_frame_ms"] = gap - entry["frame_gap_to_pinhole_with_ms"]
        if pose in before:
            lo, hi = before[pose]["best_ms"], before[pose]["max_ms"]
            m0 = statistics.median(off["frame_kernel_ms"])
            entry["knob_0_frame_matches_the_earlier_profile"] = bool(lo <= m0 <= hi)   # (inside that file's own best .. max)
        res[pose] = entry
        for label, r in (("without", off), ("with", on)):
            print(f"{wl} {pose:8s} {label:7s} tiles: set_pose {statistics.median(r['set_pose_wall_ms']):7.3f}  build wall {statistics.median(r['build_wall_ms']):7.3f} "
                  f"(device {statistics.median(r['build_device_ms']):6.3f})  frame {statistics.median(r['frame_kernel_ms']):7.3f}  sum {statistics.median(r['sum_ms']):7.3f} ms "
                  f"[{min(r['sum_ms']):.3f} .. {max(r['sum_ms']):.3f}]", flush=True)
        print(f"{wl} {pose:8s} gain of the sum {gain:.3f} ms, spread between rounds {spread:.3f} ms, tiles pay: {entry['tiles_pay']}; table "
              f"{infos[('1', pose)]}", flush=True)
    print(f"{wl} pinhole frame {res['frame_kernel_ms_pinhole']['median_ms']:.3f} ms (after: {res['frame_kernel_ms_pinhole_after']['median_ms']:.3f})", flush=True)
    res["default_on"] = bool(res["pan"]["tiles_pay"] and res["identity"]["tiles_pay"])
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if len(sys.argv) > 4 and sys.argv[4] == "tiles":
    pose_tiles_timing(sys.argv[3])
    sys.exit(0)

result = {"what": "rt_set_pose on a live context against the two routes to the same ray buffer without it (torch on the device + "
                  "rt_set_rays_device; numpy posed_rays + rt_set_rays); device time of the verdict and generation kernels; kernel time of the "
                  "frame from the posed buffer and from the pinhole camera",
          "workload": desc, "frame": [W, H], "rays": n, "ray_bytes": 32 * n, "repeats": repeats, "library_sha16": bench.library_sha16(),
          "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, z))
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
result["frame_kernel_ms_pinhole"] = frame_kernel_ms(rt, d_frame)
d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
torch_posed_rays(W, H, z, M, origin, d_rays)
generated = rt.generate_rays(W, H, z, M, origin)
torch.cuda.synchronize()
result["torch_rays_equal_the_generator_bit_for_bit"] = bool(torch.equal(d_rays.view(torch.int32), generated.view(torch.int32)))
del generated

os.environ["RT_RAYS_TRACE"] = "1"
pose_walls, verdicts, gens, torch_ms, set_rays_walls, device_route = [], [], [], [], [], []
for rep in range(repeats + 1):
    def pose():
        t0 = time.perf_counter()
        rt.set_pose(W, H, z, M, origin)
        return (time.perf_counter() - t0) * 1e3
    wall, err = stderr_of(pose)
    m = re.search(r"\[rt_set_pose\] verdict ([0-9.]+) ms generate ([0-9.]+) ms", err)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch_posed_rays(W, H, z, M, origin, d_rays)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _, _ = stderr_of(lambda: rt.set_rays(d_rays))
    t2 = time.perf_counter()
    if rep:   # (the first round is the warm-up: the context's ray buffer is allocated there, torch's kernels are loaded)
        pose_walls.append(wall)
        verdicts.append(float(m.group(1)))
        gens.append(float(m.group(2)))
        torch_ms.append((t1 - t0) * 1e3)
        set_rays_walls.append((t2 - t1) * 1e3)
        device_route.append((t2 - t0) * 1e3)
os.environ.pop("RT_RAYS_TRACE")
result["set_pose_wall_ms"] = summary(pose_walls)
result["verdict_kernel_ms"] = summary(verdicts)
result["generation_kernel_ms"] = summary(gens)
result["generation_TB_per_s_best_written"] = 32 * n / (min(gens) * 1e-3) / 1e12
result["torch_rays_wall_ms"] = summary(torch_ms)
result["set_rays_device_wall_ms"] = summary(set_rays_walls)
result["torch_plus_set_rays_device_wall_ms"] = summary(device_route)

host_make, host_set, host_route = [], [], []
for rep in range(host_repeats + 1):
    t0 = time.perf_counter()
    rays = RY.posed_rays(W, H, z, M, origin)
    t1 = time.perf_counter()
    rt.set_rays(rays)
    t2 = time.perf_counter()
    if rep:
        host_make.append((t1 - t0) * 1e3)
        host_set.append((t2 - t1) * 1e3)
        host_route.append((t2 - t0) * 1e3)
    del rays
result["posed_rays_host_wall_ms"] = summary(host_make)
result["set_rays_host_wall_ms"] = summary(host_set)
result["posed_rays_plus_set_rays_wall_ms"] = summary(host_route)

# the frame: the identity pose generates the camera's own rays, so both frames trace the same rays
rt.set_pose(W, H, z, np.eye(3))
info = rt.rays_info()
result["rays_info_posed"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in info.items()}
result["frame_kernel_ms_posed_identity"] = frame_kernel_ms(rt, d_frame)
rt.set_pose(W, H, z, M, origin)
result["frame_kernel_ms_posed_pan"] = frame_kernel_ms(rt, d_frame)
rt.set_camera(W, H, z)
result["frame_kernel_ms_pinhole_after"] = frame_kernel_ms(rt, d_frame)
rt.close()
for k in ("set_pose_wall_ms", "verdict_kernel_ms", "generation_kernel_ms", "torch_rays_wall_ms", "set_rays_device_wall_ms", "torch_plus_set_rays_device_wall_ms",
          "posed_rays_host_wall_ms", "set_rays_host_wall_ms", "posed_rays_plus_set_rays_wall_ms", "frame_kernel_ms_pinhole", "frame_kernel_ms_posed_identity",
          "frame_kernel_ms_posed_pan", "frame_kernel_ms_pinhole_after"):
    print(f"{wl} {k:36s} best {result[k]['best_ms']:10.3f}  median {result[k]['median_ms']:10.3f} ms", flush=True)
print(f"{wl} generation {result['generation_TB_per_s_best_written']:.2f} TB/s written; torch rays equal the generator's: "
      f"{result['torch_rays_equal_the_generator_bit_for_bit']}; grid_in_use {info['grid_in_use']}", flush=True)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(result, f, indent=1)
