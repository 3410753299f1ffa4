"""Fuzz: pinhole frames. (a) small scenes: monolithic kernel with per-bundle screen culling vs wavefront brute force;
(b) large scenes: screen-tile primaries + grid vs brute force. Bit for bit."""
import os, sys, time
ROOT = __import__('pathlib').Path(__file__).resolve().parents[2]; sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
import numpy as np
import _pkg; _pkg.load()
from helpers import same_floats, pinhole_fuzz_scene as scene, clear_lights, device_mismatch
DEVICE = bool(os.environ.get("FUZZ_DEVICE_OPENCL"))      # RT_FLAG_DEVICE_OPENCL; lights moved out of every object's reach
XCHECK = int(os.environ.get("FUZZ_XCHECK", "0"))         # every Nth seed also against oracle.DeviceReference (with DEVICE)
from opencl_raytracer_amd import camera
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer

bad = xchecked = 0
n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 100
t0 = time.time()
for seed in range(n_seeds):
    rng = np.random.default_rng(7000 + seed)
    small = seed % 2 == 0
    n = int(rng.choice([1, 3, 9, 30, 64])) if small else int(rng.choice([100, 400, 2000]))
    objs, lights = scene(rng, n)
    W, H = [(64, 64), (128, 72), (256, 128), (192, 200)][int(rng.integers(0, 4))]
    fov = float(rng.choice([20.0, 60.0, 120.0]))
    z = float(-(H / 2) / np.tan(np.radians(fov) / 2))
    kernel = ["shade_and_reflect", "shade", "hittest"][int(rng.integers(0, 3))]
    depth = int(rng.integers(0, 4))
    if DEVICE: lights, _ = clear_lights(objs, lights, rng)
    res = []
    for mode in (0, 1):
        kw = dict(path="monolithic") if (small and mode == 0) else (dict(path="wavefront", grid=True) if mode == 0 else dict(path="wavefront", grid=False))
        with HIPRaytracer(objs, lights, None, depth, camera=(W, H, z), kernel=kernel, device_opencl=DEVICE, **kw) as rt:
            out = rt.Render().copy(); t, i = rt.render_aux(); st = rt.count_rays()
            res.append((out, t.copy(), i.copy(), st.rays_reference))
    a, b = res
    ok = np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2], b[2]) and same_floats(a[1], b[1]) and a[3] == b[3]
    if not ok:
        bad += 1
        print('MISMATCH seed', seed, 'small' if small else 'large', n, kernel, depth, (W, H), fov, 'pixels', int(np.any(a[0].reshape(W * H, -1) != b[0].reshape(W * H, -1), axis=1).sum()), 'idx', int((a[2] != b[2]).sum()), flush=True)
    if DEVICE and XCHECK and seed % XCHECK == 0:
        rays = camera.primary_rays(W, H, fov)
        rays["direction"][:, 2] = np.float32(z)   # the camera's z as rt_set_camera takes it
        why = device_mismatch(objs, lights, rays, kernel, depth, a[0], a[1])
        xchecked += 1
        if why: bad += 1; print('DEVICE MISMATCH seed', seed, kernel, why, flush=True)
print('TOTAL mismatches', bad, 'device cross-checks', xchecked, f'{time.time()-t0:.0f}s')
