"""GPU: replaceable rays (hip_raytracer.h, "replaceable rays") - rt_set_rays_device, rt_set_rays, rt_get_rays_info.

1. the scan kernel (csrc/rt_rays.hip) against rays.ray_verdict on the cases of test_set_rays_cpu.scan_cases, through the host
   twin and through a device tensor;
2. frames on a live context walked through cameras and ray buffers: every step is the frame of a FRESH context created in that
   state, bit for bit, and meets the oracle with the project's bars;
3. the verdict's routes; 4. partitions; 5. ownership and streams; 6. a seeded walk over all three setters.
The reference of every bit-for-bit comparison is a fresh context created with those rays and RT_FLAG_NO_RAYGEN, or with that camera."""
import numpy as np
import pytest
import torch

from opencl_raytracer_amd import rays as RY, sharding
from test_context_lifecycle_gpu import INVALID_ARGUMENT, clean_env
from test_frame_shapes_cpu import DEPTH, FACTORS_9216, camera_z_for, pinhole_rays, scene
from test_frame_shapes_gpu import assert_same_snapshot, check_against_oracle, hip, packed_of, same_bits, snapshot, stitched
from test_set_rays_cpu import CONTEXTS, POSES, SCAN_COUNTS, check_verdict, pose_rays, scan_cases, sees_the_scene, tri_moved_origin

pytestmark = pytest.mark.gpu
F = np.float32


def device_tensor(rays):
    """A numpy ray array as the (n, 8) float32 device tensor set_rays takes."""
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def info_as_verdict(info):
    return dict(dir_w_zero=info["dir_w_zero"], directions_in_domain=info["directions_in_domain"], starts_ok=info["starts_ok"],
                origin_lo=info["origin_lo"], origin_hi=info["origin_hi"])


def fresh_snapshot(name, kernel, rays=None, cam=None, shard=None):
    objs, lights = scene(name)
    with (hip(objs, lights, rays, DEPTH, kernel=kernel, raygen=False) if rays is not None else hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel)) as rt:
        if shard:
            rt.set_shard(*shard)
        return snapshot(rt)


# ---- 1. the scan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCAN_COUNTS)
def test_scan_matches_ray_verdict(n):
    from helpers import random_scene
    objs, lights = random_scene(1, 1, 1, seed=3)
    cases = scan_cases(n)
    # created without rays: the context's own ray buffer is allocated by the first call
    with hip(objs, lights, None, 0, camera=(n, 1, -1.0), kernel="hittest") as rt:
        before = rt.rays_info()
        assert (before["source"], before["dir_w_zero"], before["starts_ok"], before["grid_built"]) == (1, 1, 1, 0)
        for label, rays, built in cases:
            want = RY.ray_verdict(rays)
            expect = dict(built)
            if built["box"] is not None:
                expect["origin_lo"], expect["origin_hi"] = built["box"]
            check_verdict(want, expect, f"ray_verdict, n = {n}, {label}")
            for route in ("host", "device"):
                rt.set_rays(rays if route == "host" else device_tensor(rays))
                info = rt.rays_info()
                where = f"n = {n}, {label}, {route} route"
                assert info["source"] == 2, where
                check_verdict(info_as_verdict(info), want, where)
                assert info["literal"] == (0 if want["directions_in_domain"] else 1) and info["grid_in_use"] == 0, where
                if not want["starts_ok"]:
                    assert not info["origin_lo"].any() and not info["origin_hi"].any(), where
        assert rt.stats().pinhole == 0
        rt.Render()   # the last case's rays, n work-items: the buffer the scan accepted is a whole frame's


def test_what_the_setters_refuse():
    from opencl_raytracer_amd.hip_raytracer import RTError
    objs, lights = scene("s40")
    W, H = 36, 50
    n = W * H
    cam = (W, H, camera_z_for("s40", W, H))
    pan = pose_rays("s40", W, H, "pan")
    longer = np.concatenate([pan, pan[:1]])
    d = device_tensor(longer)
    with hip(objs, lights, None, DEPTH, camera=cam) as rt:
        want = rt.Render()
        bad = {"one ray short": pan[:-1], "one ray more": longer, "one ray more, device": d,
               "a device pointer 4 bytes off a 16-byte boundary": d.reshape(-1)[1:1 + 8 * n]}
        for label, rays in bad.items():
            with pytest.raises(RTError) as refused:
                rt.set_rays(rays)
            assert refused.value.code == INVALID_ARGUMENT, label
            assert rt.rays_info()["source"] == 1, label
        assert rt._lib.rt_set_rays_device(rt._ctx, None, n, None) == INVALID_ARGUMENT
        assert rt._lib.rt_set_rays(rt._ctx, None, n) == INVALID_ARGUMENT
        assert rt._lib.rt_get_rays_info(rt._ctx, None) == INVALID_ARGUMENT
        assert same_bits(rt.Render(), want) and rt.stats().pinhole == 1
        rt.set_rays(d[:n])   # and the same tensor's first n rays are taken
        assert rt.rays_info()["source"] == 2


# ---- 2. frames on a live context -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel,shape", CONTEXTS)
def test_frames_follow_the_rays(monkeypatch, restatement, name, kernel, shape):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    objs, lights = scene(name)
    W, H = shape
    n = W * H
    cam = (W, H, camera_z_for(name, W, H))
    oracle = lambda rays: restatement[True].render(kernel, objs, lights, rays, DEPTH)   # noqa: E731
    history = [f"create {cam}"]
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        first = snapshot(rt)
        info = rt.rays_info()
        built = info["grid_built"]
        assert built == (1 if name in ("s300", "tri") else 0) and info["grid_in_use"] == built and info["source"] == 1
        assert not info["origin_lo"].any() and not info["origin_hi"].any()
        previous = first
        for step, (pose, route) in enumerate((("pan", "device"), ("moved", "host"), ("camera", None), ("far", "host"), ("pan", "host"), ("far", "device"),
                                              ("moved", "device"))):
            where = f"{name} {kernel} step {step} ({pose}) after {history}"
            if pose == "camera":
                rt.set_camera(*cam)
                history.append("set_camera")
                got = snapshot(rt)
                assert_same_snapshot(got, first, where)
                info = rt.rays_info()
                assert (info["source"], info["grid_in_use"], rt.stats().pinhole) == (1, built, 1), where
                previous = got
                continue
            origin = tri_moved_origin(info["box_lo"]) if (name == "tri" and pose == "moved") else None
            rays = pose_rays(name, W, H, pose, origin)
            history.append(f"set_rays({pose}, {route})")
            if name == "tri" and pose == "far":   # a mesh is traced by the grid only: refused, nothing changes
                with pytest.raises(RTError) as refused:
                    rt.set_rays(rays if route == "host" else device_tensor(rays))
                assert refused.value.code == INVALID_ARGUMENT, where
                history[-1] += " refused"
                assert_same_snapshot(snapshot(rt), previous, where)
                continue
            rt.set_rays(rays if route == "host" else device_tensor(rays))
            got = snapshot(rt)
            st = rt.stats()
            assert (st.pinhole, st.width, st.height, int(st.local_rays)) == (0, 0, 0, n), where
            info = rt.rays_info()
            assert (info["source"], info["dir_w_zero"], info["directions_in_domain"], info["starts_ok"], info["literal"]) == (2, 1, 1, 1, 0), where
            assert np.array_equal(info["origin_lo"], rays["start"][0, :3]) and np.array_equal(info["origin_hi"], rays["start"][0, :3]), where
            if name == "tri":
                o = rays["start"][0, :3].astype(np.float64)
                assert (o >= info["box_lo"]).all() and (o <= info["box_hi"]).all(), where
            assert info["grid_in_use"] == (built if pose != "far" else 0), f"{where}: grid_in_use {info['grid_in_use']}"
            if name == "s300":
                assert got["wavefront"] == (0 if pose == "far" else 1), where   # 96..511 objects: the large-scene path only with the grid
            want = oracle(rays)
            sees_the_scene(want, n, kernel, where)
            fresh = fresh_snapshot(name, kernel, rays=rays)
            check_against_oracle(name, kernel, fresh, want, f"FRESH context, {where}")
            assert_same_snapshot(got, fresh, where)
            check_against_oracle(name, kernel, got, want, where)
            previous = got


# ---- 3. the verdict's routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("direction.w = 1", "direction 0"))
def test_verdict_routes(monkeypatch, kind):
    clean_env(monkeypatch)
    name, kernel, (W, H) = "s300", "shade_and_reflect", (96, 96)
    objs, lights = scene(name)
    rays = pose_rays(name, W, H, "pan")
    if kind == "direction.w = 1":
        rays["direction"][W * H // 3, 3] = 1.0
    else:
        rays["direction"][W * H // 3] = 0.0
    fresh = fresh_snapshot(name, kernel, rays=rays)
    cam = (W, H, camera_z_for(name, W, H))
    for route in ("host", "device"):
        with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
            rt.Render()
            rt.set_rays(rays if route == "host" else device_tensor(rays))
            got = snapshot(rt)
            info = rt.rays_info()
            assert_same_snapshot(got, fresh, f"{kind}, {route}")
            assert got["wavefront"] == fresh["wavefront"] == 0
            if kind == "direction.w = 1":
                assert (info["dir_w_zero"], info["grid_built"], info["grid_in_use"], info["literal"]) == (0, 1, 0, 0)
            else:
                assert (info["directions_in_domain"], info["literal"], info["grid_in_use"]) == (0, 1, 0)
                assert got["traced"] == got["rays_ref"], "the literal loops trace every reference ray"
            rt.set_rays(pose_rays(name, W, H, "pan"))   # and back: the grid, the default path
            back = snapshot(rt)
            assert back["wavefront"] == 1 and back["traced"] < back["rays_ref"] and rt.rays_info()["grid_in_use"] == 1


# ---- 4. partitions -------------------------------------------------------------------------------------------------------
def test_partitions_with_buffer_rays(monkeypatch):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    name, kernel, (W, H) = "s300", "shade_and_reflect", (96, 96)
    n = W * H
    objs, lights = scene(name)
    cam = (W, H, camera_z_for(name, W, H))
    rays = pose_rays(name, W, H, "pan")
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        rt.Render()
        rt.set_rays(device_tensor(rays))
        base = snapshot(rt)
        assert_same_snapshot(base, fresh_snapshot(name, kernel, rays=rays), "unsharded")
        tr, world = 16 * W, 3
        pieces, ts, idxs, refs = [], [], [], 0
        for rank in range(world):
            rt.set_shard(tr, rank, world)
            assert rt.local_rays == sharding.local_rays(n, tr, rank, world)
            pieces.append(rt.Render())
            t, idx = rt.render_aux()
            ts.append(t)
            idxs.append(idx)
            refs += int(rt.count_rays().rays_reference)
        assert same_bits(stitched(pieces, tr, n), base["frame"]), "stitched shards differ from the unsharded frame"
        assert same_bits(stitched(ts, tr, n), base["t"]) and np.array_equal(stitched(idxs, tr, n), base["idx"])
        assert refs == base["rays_ref"]
        rt.set_shard(0, 0, 1)
        for fmt in ("rgba8", "rgb8"):
            assert np.array_equal(rt.render_packed(fmt), packed_of(base["frame"], fmt)), fmt
        monkeypatch.setenv("RT_RENDER_PASSES", "2")
        assert same_bits(rt.Render(), base["frame"]), "two passes differ from one"
        assert np.array_equal(rt.render_packed("rgba8"), packed_of(base["frame"], "rgba8"))
        monkeypatch.delenv("RT_RENDER_PASSES")
    # a factor above 1 needs a pinhole grid: refused, and the frame after the refusal is unchanged
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        rt.set_supersampling(2)
        want = rt.Render()
        assert want.shape == (n // 4, 4)
        for r in (rays, device_tensor(rays)):
            with pytest.raises(RTError) as refused:
                rt.set_rays(r)
            assert refused.value.code == INVALID_ARGUMENT
        assert rt.rays_info()["source"] == 1 and rt.supersampling == 2
        assert same_bits(rt.Render(), want)
        rt.set_supersampling(1)
        rt.set_rays(rays)
        assert same_bits(rt.Render(), base["frame"])
        with pytest.raises(RTError):
            rt.set_supersampling(2)   # the existing rule: no pinhole camera


# ---- 5. ownership and streams --------------------------------------------------------------------------------------------
def test_the_context_owns_the_rays_after_the_call(monkeypatch):
    clean_env(monkeypatch)
    name, kernel, (W, H) = "s300", "shade_and_reflect", (96, 96)
    objs, lights = scene(name)
    rays = pose_rays(name, W, H, "moved")
    want = fresh_snapshot(name, kernel, rays=rays)
    side = torch.cuda.Stream()
    host = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).pin_memory()
    with hip(objs, lights, None, DEPTH, camera=(W, H, camera_z_for(name, W, H)), kernel=kernel) as rt:
        rt.Render()
        with torch.cuda.stream(side):
            # produced on the side stream just before the call: the scan and the copy must run behind it
            buf = torch.zeros((W * H, 8), dtype=torch.float32, device="cuda")
            buf.copy_(host, non_blocking=True)
            buf.mul_(1.0)
            rt.set_rays(buf)
            buf.fill_(float("nan"))   # the caller's buffer is the caller's again
        side.synchronize()
        assert_same_snapshot(snapshot(rt), want, "after the caller overwrote its tensor")
        info = rt.rays_info()
        assert (info["starts_ok"], info["directions_in_domain"], info["grid_in_use"]) == (1, 1, 1)


# ---- 6. a seeded walk ----------------------------------------------------------------------------------------------------
def test_seeded_walk_over_the_three_setters(monkeypatch):
    clean_env(monkeypatch)
    name, kernel = "s300", "shade_and_reflect"
    objs, lights = scene(name)
    rng = np.random.default_rng(41)
    n = 9216
    seen = {}

    def fresh(key, **kw):
        if key not in seen:
            seen[key] = fresh_snapshot(name, kernel, **kw)
        return seen[key]
    W, H = FACTORS_9216[0]
    state = dict(cam=(W, H, camera_z_for(name, W, H)), rays=None, shard=None)
    history, kinds, grids = [f"create {state['cam']}"], set(), set()
    with hip(objs, lights, None, DEPTH, camera=state["cam"], kernel=kernel) as rt:
        rt.Render()
        for step in range(20):
            kind = ("rays", "camera", "shard", "rays")[step % 4] if step < 8 else ("rays", "camera", "shard")[int(rng.integers(0, 3))]
            if kind == "camera":
                W, H = FACTORS_9216[int(rng.integers(0, len(FACTORS_9216)))]
                state.update(cam=(W, H, camera_z_for(name, W, H)), rays=None)
                rt.set_camera(*state["cam"])
                history.append(f"set_camera{state['cam']}")
            elif kind == "rays":
                W, H = FACTORS_9216[int(rng.integers(0, 4))]
                pose = list(POSES)[int(rng.integers(0, 3))]
                pose = {0: "far", 3: "pan"}.get(step, pose)   # both sides of the grid's box, whatever the draws
                route = ("host", "device")[int(rng.integers(0, 2))]
                state.update(rays=(pose, W, H), cam=None)
                rays = pose_rays(name, W, H, pose)
                rt.set_rays(rays if route == "host" else device_tensor(rays))
                history.append(f"set_rays({pose} {W}x{H}, {route})")
                grids.add(rt.rays_info()["grid_in_use"])
            else:
                tile = int(rng.choice([16 * 96, 50, 4 * 128]))
                world = int(rng.choice([1, 2, 3]))
                state["shard"] = (tile, int(rng.integers(0, world)), world) if world > 1 else None
                rt.set_shard(*(state["shard"] or (0, 0, 1)))
                history.append(f"set_shard{state['shard']}")
            kinds.add(kind)
            where = f"step {step} after {history}"
            if state["rays"]:
                pose, W, H = state["rays"]
                want = fresh(("rays", pose, W, H, state["shard"]), rays=pose_rays(name, W, H, pose), shard=state["shard"])
            else:
                want = fresh(("cam", state["cam"], state["shard"]), cam=state["cam"], shard=state["shard"])
            expect_local = sharding.local_rays(n, *state["shard"]) if state["shard"] else n
            assert rt.local_rays == expect_local, where
            assert_same_snapshot(snapshot(rt), want, where)
    assert kinds == {"rays", "camera", "shard"} and grids == {0, 1}
