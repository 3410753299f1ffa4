#!/usr/bin/env python3
"""A posed camera OUTSIDE the grid's box (hip_raytracer.h, "outside the box") on cfg4, one process per call:

  frame [rounds] [out.json]     this library, 4096^2: the frame behind an orbit pose - origin outside the box, looking at the box's
                                centre, inside the FAR condition - against the identity pose's frame on the same context (kernel time,
                                medians of `rounds` frames, default 20); the per-pose cost: rt_tiles_info_t::build_device_ms of the
                                orbit pose (the spheres kernel + the table) beside an in-box pose's
  small W H [rounds] [out.json] the same orbit pose at a W x H frame, kernel time: small enough for a library that renders such a
                                pose by brute force (the parent commit's; RT_LIB_OVERRIDE picks the library)
  headline [rounds] [out.json]  the rt_set_camera frame at 4096^2 (the path this change must not touch), kernel time: run in
                                alternating fresh processes with RT_LIB_OVERRIDE = the parent's library and without

  thumb N [rounds] [out.json]   the threshold behind RT_TILES_REFUSED_SMALL: a synthetic scene of N objects, the orbit pose at 64 x 48,
                                64 x 64, 128 x 64 and 256 x 128, each frame once through the pose's tiles and the round machine
                                (RT_POSE_OUTSIDE_MIN_TILES=0) and once refused (RT_POSE_TILES=0: below 512 objects the small-scene kernel)

Every mode prints one JSON line and, given a path, merges its result into that file under its mode's key."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch ships its own ROCm runtime)
import bench  # noqa: E402
from opencl_raytracer_amd import camera, synthetic  # noqa: E402
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "best_ms": min(ms), "max_ms": max(ms), "frames": len(ms)}


def frame_kernel_ms(rt, d_frame, n):
    ms = []
    for _ in range(n + 1):   # (the first frame warms up: buffers, the pose's table)
        rt.render_device(d_frame.data_ptr(), 0)
        torch.cuda.synchronize()
        ms.append(float(rt.stats().last_kernel_ms))
    return summary(ms[1:])


def orbit_pose(info, W, H):
    """From one box diagonal outside the +x face, a little above the centre, looking at the box's centre; z lets the box span the frame."""
    lo, hi = info["box_lo"], info["box_hi"]
    centre, diag = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
    o = centre + np.array([0.0, 0.15, 0.1]) * diag
    o[0] = hi[0] + diag
    o = o.astype(np.float32)
    z = float(np.float32(-0.5 * max(W, H) * np.linalg.norm(o - centre) / (0.5 * diag)))
    return z, camera.look_at(o, centre), o


def keep(info, names):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in info.items() if k in names}


def thumb(n_objs, rounds, out_path):
    objs, lights = synthetic.spheres_and_lights(n_objs, 2)
    res = {"objects": n_objs, "rounds": rounds, "library_sha16": bench.library_sha16(), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded"),
           "what": "frame kernel ms of the orbit pose: served by its tiles (round machine) against refused (RT_POSE_TILES=0)", "frames": {}}
    for W, H in ((64, 48), (64, 64), (128, 64), (256, 128)):
        n = W * H
        d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        with HIPRaytracer(objs, lights, None, 3, kernel="shade_and_reflect", camera=(W, H, float(camera.camera_z(H)))) as rt:
            z, M, o = orbit_pose(rt.rays_info(), W, H)
            row = {}
            for label, env in (("tiles", {"RT_POSE_OUTSIDE_MIN_TILES": "0"}), ("refused", {"RT_POSE_TILES": "0"})):
                for k in ("RT_POSE_OUTSIDE_MIN_TILES", "RT_POSE_TILES"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                rt.set_pose(W, H, z, M, o)
                ri = rt.rays_info()
                ms = frame_kernel_ms(rt, d_frame, rounds)
                row[label] = {"frame_kernel_ms": ms, "grid_in_use": ri["grid_in_use"], "wavefront": int(rt.stats().wavefront)}
            res["frames"][f"{W}x{H}"] = row
    for k in ("RT_POSE_OUTSIDE_MIN_TILES", "RT_POSE_TILES"):
        os.environ.pop(k, None)
    print(json.dumps({"thumb": res}), flush=True)
    if out_path:
        merged = json.load(open(out_path)) if os.path.exists(out_path) else {}
        merged[f"thumb_{n_objs}"] = res
        with open(out_path, "w") as f:
            json.dump(merged, f, indent=1)


def main():
    mode = sys.argv[1]
    args = sys.argv[2:]
    if mode == "thumb":
        return thumb(int(args[0]), int(args[1]) if len(args) > 1 else 20, args[2] if len(args) > 2 else None)
    if mode == "small":
        W, H = int(args[0]), int(args[1])
        args = args[2:]
    rounds = int(args[0]) if args else 20
    out_path = args[1] if len(args) > 1 else None
    desc, objs, lights, W0, H0, kernel, depth = bench.load_workload("cfg4")
    if mode != "small":
        W, H = W0, H0
    n = W * H
    zc = float(camera.camera_z(H))
    res = {"workload": desc, "frame": [W, H], "rounds": rounds, "library_sha16": bench.library_sha16(),
           "library": os.environ.get("RT_LIB_OVERRIDE", "this commit's"), "measured_on": os.environ.get("RT_TIMING_WHERE", "not recorded")}
    rt = HIPRaytracer(objs, lights, None, depth, kernel=kernel, camera=(W, H, zc))
    d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    if mode == "headline":
        res["frame_kernel_ms_camera"] = frame_kernel_ms(rt, d_frame, rounds)
    else:
        info = rt.rays_info()
        z, M, o = orbit_pose(info, W, H)
        res["orbit_pose"] = {"origin": o.tolist(), "z": z, "box_lo": info["box_lo"].tolist(), "box_hi": info["box_hi"].tolist()}
        if mode == "frame":
            rt.set_pose(W, H, zc, np.eye(3))
            res["identity_pose"] = {"frame_kernel_ms": frame_kernel_ms(rt, d_frame, rounds), "tiles_info": rt.tiles_info()}
            inside = np.array([0.5, -0.5, -1.0], dtype=np.float32)   # (cfg4's box ends at z = 0, the create-time eye)
            assert bool(((inside >= info["box_lo"]) & (inside <= info["box_hi"])).all()), "the in-box pose is not inside the box"
            builds = []
            for k in range(5):   # an in-box pose's table, built again per pose
                rt.set_pose(W, H, zc, camera.look_at(inside, (0.1 * k, 0.0, -50.0)), inside)
                ti = rt.tiles_info()
                assert (ti["enabled"], ti["source"]) == (1, 2), f"the in-box pose's table: {ti}"
                builds.append(ti["build_device_ms"])
            res["in_box_pose"] = {"origin": inside.tolist(), "build_device_ms": summary(builds[1:]), "tiles_info": ti}
        builds = []
        for k in range(5 if mode == "frame" else 1):
            rt.set_pose(W, H, z, M, o)
            ti = rt.tiles_info()
            builds.append(ti["build_device_ms"])
        ri = keep(rt.rays_info(), ("source", "grid_built", "grid_in_use", "primary_outside_box", "literal"))
        res["outside_pose"] = {"rays_info": ri, "tiles_info": ti}
        if mode == "frame" and not ri.get("primary_outside_box"):   # brute force at 4096^2 is minutes per frame: not timed here
            res["outside_pose"]["frame_kernel_ms"] = None
            print(json.dumps({mode: res}), flush=True)
            sys.exit("the orbit pose was not accepted onto the grid path: see tiles_info.refused")
        res["outside_pose"]["frame_kernel_ms"] = frame_kernel_ms(rt, d_frame, rounds)
        if mode == "frame":
            res["outside_pose"]["build_device_ms"] = summary(builds[1:])
        st = rt.stats()
        res["outside_pose"]["wavefront"] = int(st.wavefront)
    rt.close()
    print(json.dumps({mode: res}), flush=True)
    if out_path:
        merged = {}
        if os.path.exists(out_path):
            with open(out_path) as f:
                merged = json.load(f)
        key = mode if mode != "small" else f"small_{W}x{H}"
        if mode in ("small", "headline"):
            merged.setdefault(key, []).append(res)
        else:
            merged[key] = res
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(merged, f, indent=1)


if __name__ == "__main__":
    main()
