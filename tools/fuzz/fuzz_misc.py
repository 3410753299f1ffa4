"""Fuzz: sharding (interleaved tiles, ragged ends, tile order) and literal-vs-optimised, bit for bit."""
import os, sys, time
ROOT = __import__('pathlib').Path(__file__).resolve().parents[2]; sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
import numpy as np
import _pkg; _pkg.load()
from helpers import misc_fuzz_case, clear_lights, device_mismatch
from opencl_raytracer_amd import camera, sharding
from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
DEVICE = bool(os.environ.get("FUZZ_DEVICE_OPENCL"))      # RT_FLAG_DEVICE_OPENCL (fused only); lights moved out of every object's reach
XCHECK = int(os.environ.get("FUZZ_XCHECK", "0"))         # every Nth seed also against oracle.DeviceReference (with DEVICE)
bad = xchecked = 0
n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 100
t0 = time.time()
for seed in range(n_seeds):
    rng = np.random.default_rng(9000 + seed)
    c = misc_fuzz_case(rng)
    objs, lights, W, H, kernel, depth, fused, pin = (c[k] for k in ("objs", "lights", "W", "H", "kernel", "depth", "fused", "pin"))
    n_s_b = len(objs)
    if DEVICE:
        fused = True
        lights, _ = clear_lights(objs, lights, rng)
    z = float(camera.camera_z(H))
    rays = None if pin else camera.primary_rays(W, H)
    kw = dict(camera=(W, H, z)) if pin else dict(raygen=False)
    with HIPRaytracer(objs, lights, rays, depth, kernel=kernel, fused=fused, device_opencl=DEVICE, **kw) as rt:
        full = rt.Render().copy()
    # (a) shards
    world = int(rng.integers(2, 6))
    tile_rows = int(rng.choice([1, 3, 8, 16, 24]))
    tile_rays = W * tile_rows if rng.uniform() < 0.8 else int(rng.integers(17, 999))
    pieces = []
    for rank in range(world):
        with HIPRaytracer(objs, lights, rays, depth, kernel=kernel, fused=fused, device_opencl=DEVICE, **kw) as rt:
            rt.set_shard(tile_rays, rank, world)
            pieces.append(rt.Render().copy())
    import torch
    asm = sharding.assemble_frame([torch.from_numpy(p) for p in pieces], tile_rays, W * H).numpy()
    if not np.array_equal(asm.view(np.uint32).reshape(-1), full.view(np.uint32).reshape(-1)):
        bad += 1
        print('SHARD MISMATCH seed', seed, n_s_b, kernel, depth, (W, H), 'pin', pin, 'world', world, 'tile_rays', tile_rays, flush=True)
    # (b) literal
    if n_s_b <= 210:
        with HIPRaytracer(objs, lights, rays, depth, kernel=kernel, fused=fused, literal=True, device_opencl=DEVICE, **kw) as rt:
            lit = rt.Render().copy()
        if not np.array_equal(lit.view(np.uint32), full.view(np.uint32)):
            bad += 1
            print('LITERAL MISMATCH seed', seed, n_s_b, kernel, depth, (W, H), 'pin', pin, flush=True)
    if DEVICE and XCHECK and seed % XCHECK == 0:
        r = rays if rays is not None else camera.primary_rays(W, H)
        with HIPRaytracer(objs, lights, r, depth, kernel=kernel, device_opencl=True, raygen=False) as rt:
            o = rt.Render().copy(); t, _ = rt.render_aux()
        why = device_mismatch(objs, lights, r, kernel, depth, o, t)
        xchecked += 1
        if why: bad += 1; print('DEVICE MISMATCH seed', seed, kernel, why, flush=True)
print('TOTAL mismatches', bad, 'device cross-checks', xchecked, f'{time.time()-t0:.0f}s')
