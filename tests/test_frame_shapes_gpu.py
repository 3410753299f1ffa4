"""GPU: every listed frame shape (tests/test_frame_shapes_cpu.py proves the list complete) against the oracle, and the same
frame from every route the library has to it.

Per scene x shape, for hittest, shade and shade_and_reflect at depth 3:
  1. unsharded, in-kernel rays, path auto: primary t and hit index identical to the oracle's on every ray, rays_reference
     equal, RGB within 1e-5, hittest frames bit for bit (the bars of test_parity_gpu.py);
  2. bit for bit the same frame from uploaded rays, the other path, brute force, the literal loops; the unfused arithmetic
     against the unfused oracle; RT_FLAG_DEVICE_OPENCL as HIP against HIP (in-kernel = uploaded = brute force);
  3. every partition: the shards of all ranks stitched, Render() through forced passes with each split, the 8-bit frames,
     three contexts on one GPU - the unsharded frame, bit for bit.
`pytest -s` prints one summary line per scene."""
import time

import numpy as np
import pytest

from helpers import clear_lights, compare_frames, same_floats
from opencl_raytracer_amd import ppm, sharding
from test_frame_shapes_cpu import (ALL_SHAPES, DEPTH, KERNELS, SCENES, SHARDS, SPLITS, camera_z_for, launch_form, pinhole_rays, scene,
                                   shard_tile_rays)

pytestmark = pytest.mark.gpu
RGB_ATOL = 1e-5
FORMATS = (("rgba8", 4), ("rgb8", 3))
TALLY = {name: dict(shapes=0, renders=0, err=0.0, seconds=0.0) for name in SCENES}


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def snapshot(rt):
    """Everything a context says about its frame: pixels, primary t and index, the counted render's figures."""
    frame = rt.Render()
    t, idx = rt.render_aux()
    st = rt.count_rays()
    return dict(frame=frame, t=t, idx=idx, rays_ref=int(st.rays_reference), traced=int(st.rays_traced), hits=int(st.hit_pixels),
                wavefront=int(st.wavefront))


def assert_same_snapshot(got, want, label, counts=True):
    assert same_bits(got["frame"], want["frame"]), f"{label}: frame differs on {int((bits(got['frame']) != bits(want['frame'])).sum())} words"
    assert same_bits(got["t"], want["t"]) and np.array_equal(got["idx"], want["idx"]), f"{label}: primary t / index differ"
    if counts:
        assert (got["rays_ref"], got["hits"]) == (want["rays_ref"], want["hits"]), f"{label}: rays_reference / hit_pixels differ"


def packed_of(frame, fmt):
    return ppm.quantise_bytes(frame if fmt == "rgba8" else frame[:, :3])


def stitched(pieces, tile_rays, n_rays):
    return sharding.assemble_frame(pieces, tile_rays, n_rays)


def oracle_index(kernel, want):
    """The oracle's winner as rt_render_aux reports it: -1 wherever the KERNEL treats the ray as a miss. The oracle hands out the
    state of its object loop; for a ray whose time is NaN (a direction of 0: every test of the loop gives NaN and the last sphere
    or box keeps it) hittest and shade see a miss (`t < MAX_FLOAT` fails, shade_kernel.cl:167), shade_and_reflect sees a hit
    (`t == MAX_FLOAT` fails, shade_and_reflect_kernel.cl:173). For every other ray the two are the same thing."""
    if kernel == "shade_and_reflect":
        return want["hit_index"]
    with np.errstate(invalid="ignore"):
        return np.where(want["hit_t"] < np.float32(3.402823466e+38), want["hit_index"], -1).astype(np.int32)


def check_against_oracle(name, kernel, base, want, label):
    assert same_floats(base["t"], want["hit_t"]), f"{label}: primary t differs from the oracle on {int((base['t'] != want['hit_t']).sum())} rays"
    differ = base["idx"] != oracle_index(kernel, want)
    assert not differ.any(), f"{label}: hit index differs from the oracle on {int(differ.sum())} rays, first at {int(np.argmax(differ))}"
    assert base["rays_ref"] == want["rays_ref"], f"{label}: rays_reference {base['rays_ref']} != {want['rays_ref']}"
    if kernel == "hittest":
        assert same_floats(base["frame"], want["out"]), f"{label}: hittest frame"
        return 0.0
    err = compare_frames(base["frame"], want["out"])
    assert err <= RGB_ATOL, f"{label}: max |dRGB| {err:.3e}"
    return err


def check_partitions(monkeypatch, name, kernel, make, base, W, H, label):
    """Section 3: shards, passes, bytes, three contexts on one GPU."""
    n = W * H
    colour = kernel != "hittest"
    renders = 0
    for shard in SHARDS:
        tr, world = shard_tile_rays(shard, W), shard[3]
        pieces, ts, idxs = [], [], []
        packed = {fmt: [] for fmt, _ in FORMATS}
        with make() as rt:
            for rank in range(world):
                rt.set_shard(tr, rank, world)
                assert rt.local_rays == sharding.local_rays(n, tr, rank, world) == launch_form(W, H, -1.0, 0, tr, rank, world)["n_local"]
                pieces.append(rt.Render())
                t, idx = rt.render_aux()
                ts.append(t)
                idxs.append(idx)
                renders += 2
                if colour:
                    for fmt, _ in FORMATS:
                        packed[fmt].append(rt.render_packed(fmt))
                        renders += 1
        where = f"{label} {shard[0]}"
        assert same_bits(stitched(pieces, tr, n), base["frame"]), f"{where}: stitched shards differ from the unsharded frame"
        assert same_bits(stitched(ts, tr, n), base["t"]) and np.array_equal(stitched(idxs, tr, n), base["idx"]), f"{where}: render_aux of the shards"
        for fmt, _ in FORMATS if colour else ():
            assert np.array_equal(stitched(packed[fmt], tr, n), packed_of(base["frame"], fmt)), f"{where}: {fmt} shards"
    if base["wavefront"]:  # only the large-scene path renders in passes
        monkeypatch.setenv("RT_RENDER_PASSES", "2")
        for split in SPLITS:
            if split: monkeypatch.setenv("RT_RENDER_SPLIT", split)
            else: monkeypatch.delenv("RT_RENDER_SPLIT", raising=False)
            with make() as rt:
                assert same_bits(rt.Render(), base["frame"]), f"{label}: Render() in passes, split {split}"
                renders += 1
                for fmt, _ in FORMATS if colour else ():
                    assert np.array_equal(rt.render_packed(fmt), packed_of(base["frame"], fmt)), f"{label}: {fmt} in passes, split {split}"
                    renders += 1
                assert same_bits(rt.Render(), base["frame"]) and rt.local_rays == n, f"{label}: Render() after the passes, split {split}"
        monkeypatch.delenv("RT_RENDER_SPLIT", raising=False)
        monkeypatch.delenv("RT_RENDER_PASSES")
    if colour:
        with make() as rt:
            for fmt, _ in FORMATS:
                assert np.array_equal(rt.render_packed(fmt), packed_of(base["frame"], fmt)), f"{label}: {fmt}"
                renders += 1
    return renders


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_every_route_to_a_frame(monkeypatch, restatement, name, shape):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    for k in ("RT_RENDER_PASSES", "RT_RENDER_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    started = time.perf_counter()
    objs, lights = scene(name)
    tri = name == "tri"
    W, H = shape
    n = W * H
    z = camera_z_for(name, W, H)
    rays = pinhole_rays(W, H, z)
    cam = (W, H, z)
    tally = TALLY[name]
    cl_lights, _ = clear_lights(objs, lights, np.random.default_rng(5)) if not tri else (None, 0)
    for kernel in KERNELS:
        label = f"{name} {W}x{H} {kernel}"
        kw = dict(kernel=kernel)
        make = lambda **more: hip(objs, lights, None, DEPTH, camera=cam, **kw, **more)  # noqa: E731
        # 1. the oracle
        with make() as rt:
            base = snapshot(rt)
            assert rt.stats().pinhole == 1 and (rt.stats().width, rt.stats().height) == (W, H)
        assert base["wavefront"] == (1 if name in ("s300", "tri") else 0), label
        want = restatement[True].render(kernel, objs, lights, rays, DEPTH)
        tally["err"] = max(tally["err"], check_against_oracle(name, kernel, base, want, label))
        tally["renders"] += 3
        if name == "s300" and kernel == "shade_and_reflect" and n >= 256:
            assert base["traced"] < base["rays_ref"], f"{label}: no elimination at work - were the light tiles built?"
        # 2. other routes to the same frame
        routes = {"uploaded rays": lambda: hip(objs, lights, rays, DEPTH, raygen=False, **kw)}
        if not tri:
            routes["wavefront"] = lambda: make(path="wavefront")
            routes["monolithic"] = lambda: make(path="monolithic")
            routes["brute force"] = lambda: make(path="wavefront", grid=False)
            routes["literal"] = lambda: make(literal=True)
        for route, ctor in routes.items():
            with ctor() as rt:
                got = snapshot(rt)
                tally["renders"] += 3
            assert_same_snapshot(got, base, f"{label} {route}")
            if route in ("wavefront", "brute force"):
                assert got["wavefront"] == 1, f"{label} {route}"
            if route in ("monolithic", "literal"):
                assert got["wavefront"] == 0, f"{label} {route}"
        if kernel == "shade_and_reflect":
            with make(fused=False) as rt:
                got = snapshot(rt)
                tally["renders"] += 3
            check_against_oracle(name, kernel, got, restatement[False].render(kernel, objs, lights, rays, DEPTH), f"{label} unfused")
        if not tri:  # HIP against HIP only: the device arithmetic has its own reference elsewhere
            cl = []
            for ctor in (lambda: hip(objs, cl_lights, None, DEPTH, camera=cam, device_opencl=True, **kw),
                         lambda: hip(objs, cl_lights, rays, DEPTH, raygen=False, device_opencl=True, **kw),
                         lambda: hip(objs, cl_lights, None, DEPTH, camera=cam, device_opencl=True, path="wavefront", grid=False, **kw)):
                with ctor() as rt:
                    cl.append(snapshot(rt))
                    tally["renders"] += 3
            assert cl[0]["wavefront"] == base["wavefront"], f"{label} device_opencl left the default path"
            assert_same_snapshot(cl[1], cl[0], f"{label} device_opencl uploaded rays")
            assert_same_snapshot(cl[2], cl[0], f"{label} device_opencl brute force")
        # 3. partitions
        tally["renders"] += check_partitions(monkeypatch, name, kernel, make, base, W, H, label)
        with MultiHIPRaytracer(objs, lights, None, DEPTH, devices=(0, 0, 0), camera=cam, kernel=kernel) as m:
            assert m.frame_elems == sharding.n_tiles(n, 16 * W) * 16 * W
            assert same_bits(m.Render(), base["frame"]), f"{label}: three contexts on one GPU"
            tally["renders"] += 3
            for fmt, _ in FORMATS if kernel != "hittest" else ():
                assert np.array_equal(m.render_packed(fmt), packed_of(base["frame"], fmt)), f"{label}: three contexts, {fmt}"
                tally["renders"] += 3
    tally["shapes"] += 1
    tally["seconds"] += time.perf_counter() - started


def test_a_padded_shard_writes_background_behind_the_frame():
    """The ragged last tile's padding work-items (begin_pixel) write the background and a miss, on both paths, in both orders."""
    for name in ("s40", "s300"):
        objs, lights = scene(name)
        for (W, H), shard in (((128, 72), SHARDS[0]), ((72, 41), SHARDS[0]), ((63, 65), SHARDS[2]), ((72, 41), SHARDS[1])):
            tr, world = shard_tile_rays(shard, W), shard[3]
            ranks = [r for r in range(world) if launch_form(W, H, -1.0, 0, tr, r, world)["padded"]]
            assert len(ranks) == 1
            tiles = sharding.n_tiles(W * H, tr)
            pad = tiles * tr - W * H
            for kernel in ("hittest", "shade_and_reflect"):
                with hip(objs, lights, None, DEPTH, camera=(W, H, camera_z_for(name, W, H)), kernel=kernel) as rt:
                    rt.set_shard(tr, ranks[0], world)
                    frame = rt.Render()
                    t, idx = rt.render_aux()
                assert pad > 0 and np.all(idx[-pad:] == -1) and np.all(t[-pad:] == np.float32(3.402823466e+38))
                if kernel == "hittest":
                    assert np.all(frame[-pad:] == np.float32(3.402823466e+38))
                else:
                    assert np.array_equal(frame[-pad:], np.tile(np.float32([0, 0, 0, 1]), (pad, 1)))


def test_summary():
    """Not a check: the figures of this file (`-s`)."""
    total = 0.0
    for name, t in TALLY.items():
        total += t["seconds"]
        print(f"\n[frame shapes] {name}: {len(scene(name)[0])} objects, {t['shapes']} shapes, {t['renders']} renders, "
              f"largest |dRGB| against the oracle {t['err']:.3e}, {t['seconds']:.1f} s")
    print(f"[frame shapes] wall time of the scene x shape tests: {total:.1f} s")
