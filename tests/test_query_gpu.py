"""GPU: ray queries (hip_raytracer.h, "ray queries") - rt_query_closest / rt_query_occluded, their device forms, rt_query_primary and
rt_get_query_info - against FRESH RT_KERNEL_HITTEST contexts created with the queried rays (render_aux), bit for bit, and against
rays.query_route for the counters. Scenes: test_set_materials_gpu.py's 200-object cloud (a grid) and its first 40 objects (no grid).

1. launch boundaries: n around a wave and a workgroup; nothing written behind element n - 1;
2. mixed routes in one wave, and the counters per route;
3. every arithmetic mode on both scenes;
4. the live state is what is queried (set_transforms, set_visibility, both orders);
5. a query leaves the frame alone (camera, ray buffer, pose; shard and supersampling; aux renders);
6. pick (camera, pose inside and outside the box, ray buffer, a sharded context; no rays yet: refused);
7. the device form behind a torch kernel on another stream;
8. refusals and n == 0 change nothing; a triangle context is refused;
9. MultiHIPRaytracer through shard 0;
10. a context that is literal for a degenerate instance, or by the caller's flag, answers by the ordered loop alone;
11. rays as an (n, 8) float32 array are the same rays."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import R, rotation, same_floats
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from test_frame_shapes_cpu import camera_z_for, scene
from test_primary_depth_order_gpu import bits, hip
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, lights, small, snapshot
from test_set_transforms_gpu import apply, three_moves
from test_set_visibility_gpu import random_mask

pytestmark = pytest.mark.gpu
F = np.float32
MAX_FLOAT = F(3.402823466e+38)
MODES = {"default": {}, "unfused": dict(fused=False), "device_opencl": dict(device_opencl=True)}


def predicate(t):
    with np.errstate(invalid="ignore"):
        return (~((t >= F(1.0)) | (t < F(0.0)))).astype(np.uint8)


def fresh_aux(objs, rays, **mode):
    """(t, index) of a fresh hittest context created with these rays: the definition of a closest-hit query."""
    with hip(objs, lights(), rays, 0, kernel="hittest", raygen=False, **mode) as rt:
        return rt.render_aux()


def assert_query(got, want, label):
    (t, index), (wt, wi) = got, want
    assert t.shape == wt.shape and index.shape == wi.shape, label
    assert np.array_equal(bits(t), bits(wt)), f"{label}: t differs on {int((bits(t) != bits(wt)).sum())} rays"
    assert np.array_equal(index, wi), f"{label}: index differs on {int((index != wi).sum())} rays"


@functools.lru_cache(maxsize=None)
def cloud_box():
    """box_lo, box_hi (float64) of the 200-object context created with the camera: the box its grid's radii were derived for."""
    with hip(cloud(), lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        info = rt.rays_info()
    assert info["grid_built"] == 1
    return info["box_lo"].copy(), info["box_hi"].copy()


def centres(objs):
    return objs["mv"].reshape(len(objs), 16)[:, 12:15].astype(np.float64)


def in_box_rays(n, seed, objs=None):
    """n rays with origins uniform in the cloud's box shrunk by 1 %: the even ones aimed at randomly chosen objects' centres (the
    direction is the whole way there, so the segment ends inside the object), the odd ones with random directions of random length."""
    objs = cloud() if objs is None else objs
    lo, hi = cloud_box()
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.99
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    start = mid + rng.uniform(-1.0, 1.0, size=(n, 3)) * half
    rays["start"][:, :3] = start.astype(F)
    rays["start"][:, 3] = 1.0
    aim = centres(objs)[rng.integers(0, len(objs), size=n)] - rays["start"][:, :3].astype(np.float64)
    wander = rng.normal(size=(n, 3)) * rng.uniform(0.1, 30.0, size=(n, 1))
    rays["direction"][:, :3] = np.where((np.arange(n) % 2 == 0)[:, None], aim, wander).astype(F)
    return rays


def out_of_domain_rays(n, seed):
    """n rays the grid does not serve, the eight kinds in turn: an origin outside the box, dd = 0, dd = 1e-31, dd = 1e31, a NaN start
    with a finite direction, an inf component, start.w = 2, direction.w = 1."""
    lo, hi = cloud_box()
    rays = in_box_rays(n, seed)
    c = centres(cloud()).mean(axis=0)
    for k in range(n):
        kind = k % 8
        if kind == 0:   # from outside the box, towards the cloud
            side = np.array([hi[0] + 3.0 + k % 5, lo[1] - 2.0, hi[2] + 4.0])
            rays["start"][k, :3] = side.astype(F)
            rays["direction"][k, :3] = (c - side).astype(F)
        elif kind == 1:
            rays["direction"][k, :3] = 0.0
        elif kind == 2:
            d = rays["direction"][k, :3].astype(np.float64)
            rays["direction"][k, :3] = (d / np.linalg.norm(d) * np.sqrt(1.0e-31)).astype(F)
        elif kind == 3:
            d = rays["direction"][k, :3].astype(np.float64)
            rays["direction"][k, :3] = (d / np.linalg.norm(d) * np.sqrt(1.0e31)).astype(F)
        elif kind == 4:
            rays["start"][k, k % 3] = np.nan
        elif kind == 5:
            if k % 16 < 8:
                rays["direction"][k, k % 3] = np.inf
            else:
                rays["start"][k, (k + 1) % 3] = -np.inf
        elif kind == 6:
            rays["start"][k, 3] = 2.0
        else:
            rays["direction"][k, 3] = 1.0
    return rays


def mixed_rays(n, seed):
    """Every fourth ray out of the domain, the others in the box: every wave of 64 holds both routes."""
    rays = in_box_rays(n, seed)
    k = np.arange(n) % 4 == 3
    rays[k] = out_of_domain_rays(n, seed + 1)[:int(k.sum())]
    return rays


def route_counts(rays, grid=True):
    lo, hi = cloud_box() if grid else (None, None)
    on = RY.query_route(rays, lo, hi)
    return int(on.sum()), int((~on).sum())


# ---- 1. launch boundaries ------------------------------------------------------------------------------------------------------
def test_launch_boundaries():
    import torch
    objs = cloud()
    all_rays = mixed_rays(1000, seed=5)
    assert route_counts(all_rays[:1]) == (1, 0)
    guard_f, guard_i, guard_b = F(-7.25), np.int32(-77), np.uint8(0xa5)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            rays = all_rays[:n]
            want = fresh_aux(objs, rays)
            got = rt.query_closest(rays)
            assert_query(got, want, f"n = {n}")
            info = rt.query_info()
            assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (n,) + route_counts(rays), n
            assert np.array_equal(rt.query_occluded(rays), predicate(want[0])), n
            assert rt.query_info()["n_rays"] == n
            # the device forms into buffers of n + 1 elements: the guard behind element n - 1 stays
            d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
            d_t = torch.full((n + 1,), float(guard_f), dtype=torch.float32, device="cuda")
            d_i = torch.full((n + 1,), int(guard_i), dtype=torch.int32, device="cuda")
            d_o = torch.full((n + 1,), int(guard_b), dtype=torch.uint8, device="cuda")
            vp = ctypes.c_void_p
            assert rt._lib.rt_query_closest_device(rt._ctx, vp(d_rays.data_ptr()), n, vp(d_t.data_ptr()), vp(d_i.data_ptr()), None) == 0
            assert rt._lib.rt_query_occluded_device(rt._ctx, vp(d_rays.data_ptr()), n, vp(d_o.data_ptr()), None) == 0
            torch.cuda.synchronize()
            t, i, o = d_t.cpu().numpy(), d_i.cpu().numpy(), d_o.cpu().numpy()
            assert_query((t[:n], i[:n]), want, f"device form, n = {n}")
            assert np.array_equal(o[:n], predicate(want[0])), n
            assert bits(t[n:])[0] == bits(np.array([guard_f]))[0] and i[n] == guard_i and o[n] == guard_b, n
            # one output at a time
            d_t.fill_(float(guard_f))
            assert rt._lib.rt_query_closest_device(rt._ctx, vp(d_rays.data_ptr()), n, vp(d_t.data_ptr()), None, None) == 0
            d_i.fill_(int(guard_i))
            assert rt._lib.rt_query_closest_device(rt._ctx, vp(d_rays.data_ptr()), n, None, vp(d_i.data_ptr()), None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(bits(d_t.cpu().numpy()[:n]), bits(want[0])) and np.array_equal(d_i.cpu().numpy()[:n], want[1]), n


# ---- 2. mixed routes in one wave -----------------------------------------------------------------------------------------------
def test_mixed_routes_in_one_wave():
    objs = cloud()
    n = 1024
    rays = mixed_rays(n, seed=14)
    lo, hi = cloud_box()
    on = RY.query_route(rays, lo, hi)
    per_wave = on.reshape(-1, 64).sum(axis=1)
    assert (per_wave > 0).all() and (per_wave < 64).all()             # both routes in every wave
    assert np.array_equal(on, np.arange(n) % 4 != 3)                  # the in-box rays are the grid's, the eight other kinds are not
    # conditions on the inputs, on the CPU backend alone: agreement is not agreement on misses
    ct, ci = CPURaytracer(objs, lights(), rays[:1], 0, kernel="hittest").query_closest(rays)
    with np.errstate(invalid="ignore"):
        hit = ct[on] < MAX_FLOAT
    assert hit.mean() >= 0.25 and (~hit).mean() >= 0.25, hit.mean()
    assert np.isnan(ct[~on]).any() and (ci[~on] >= 0).any()
    want = fresh_aux(objs, rays)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        got = rt.query_closest(rays)
        info = rt.query_info()
        assert_query(got, want, "mixed routes")
        assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (n, int(on.sum()), int((~on).sum()))
        assert info["n_grid"] > 0 and info["n_brute"] > 0
        assert info["object_tests"] >= info["n_brute"] * 2 * ((N + 1) // 2) and info["device_ms"] > 0.0
        occluded = rt.query_occluded(rays)
        info = rt.query_info()
        assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (n, int(on.sum()), int((~on).sum()))
        assert np.array_equal(occluded, predicate(want[0]))
        assert 0.1 < occluded[on].mean() < 0.9                        # segments that end inside an object, and segments that reach nothing
    # ... and the CPU backend's query, the definition without a GPU (same_floats: a NaN's bits and a zero's sign are the hardware's)
    assert same_floats(got[0], ct) and np.array_equal(got[1], ci)


# ---- 3. every arithmetic mode, both scenes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_arithmetic_mode(mode, size):
    objs = cloud() if size == "large" else small()
    rays = mixed_rays(1000, seed=21)
    want = fresh_aux(objs, rays, **MODES[mode])
    for kernel in ("shade_and_reflect", "hittest"):   # a context of any rt_kernel
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel=kernel, **MODES[mode]) as rt:
            assert rt.rays_info()["grid_built"] == (1 if size == "large" else 0)
            got = rt.query_closest(rays)
            info = rt.query_info()
            assert_query(got, want, f"{mode} {size} {kernel}")
            assert (info["n_grid"], info["n_brute"]) == route_counts(rays, grid=size == "large")
            if size == "small":
                assert info["n_grid"] == 0 and info["n_brute"] == len(rays)
            assert np.array_equal(rt.query_occluded(rays), predicate(want[0])), (mode, size, kernel)
    assert (want[1] >= 0).mean() > 0.1


# ---- 4. the live state is what is queried --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_live_state_is_what_is_queried(size):
    objs = cloud() if size == "large" else small()
    n_objs = len(objs)
    moves = three_moves(objs)
    a = moves[0][0]
    rays = mixed_rays(768, seed=31)
    rays["start"][0] = (-5.0, 1.0, -30.0, 1.0)     # along x through FRONT[0] = (-2, 1, -30), in front of the cloud: nothing there until object a arrives
    rays["direction"][0] = (1.0, 0.0, 0.0, 0.0)
    mask = random_mask(n_objs, seed=33)
    mask[a] = 1
    hidden = np.nonzero(mask == 0)[0]
    moved, masked, both = apply(objs, moves), R.with_visibility(objs, mask), R.with_visibility(apply(objs, moves), mask)
    want = {"untouched": fresh_aux(objs, rays), "moved": fresh_aux(moved, rays), "masked": fresh_aux(masked, rays), "both": fresh_aux(both, rays)}
    assert want["untouched"][0][0] == MAX_FLOAT and want["untouched"][1][0] == -1
    assert want["moved"][1][0] == a and want["both"][1][0] == a
    for x in ("moved", "masked", "both"):
        assert not np.array_equal(want[x][1], want["untouched"][1]), x

    def move(rt):
        for i, t in moves:
            rt.set_transforms(t, i)

    for order in ("transforms first", "visibility first"):
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
            assert_query(rt.query_closest(rays), want["untouched"], f"{size} {order}: untouched")
            if order == "transforms first":
                move(rt)
                assert_query(rt.query_closest(rays), want["moved"], f"{size} {order}: moved")
                rt.set_visibility(mask)
            else:
                rt.set_visibility(mask)
                assert_query(rt.query_closest(rays), want["masked"], f"{size} {order}: masked")
                move(rt)
            got = rt.query_closest(rays)
            assert_query(got, want["both"], f"{size} {order}: both")
            assert not np.isin(got[1][got[1] >= 0], hidden).any()
            assert np.array_equal(rt.query_occluded(rays), predicate(want["both"][0]))
            if size == "large":
                assert rt.geometry_info()["n_dynamic"] == 3 and rt.query_info()["n_grid"] > 0
            rt.set_visibility(np.ones(n_objs, dtype=np.uint8))
            assert_query(rt.query_closest(rays), want["moved"], f"{size} {order}: shown again")


# ---- 5. a query leaves the frame alone -----------------------------------------------------------------------------------------
def test_a_query_leaves_the_frame_alone():
    objs = cloud()
    rays = mixed_rays(300, seed=41)
    turned = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    M, inside, outside = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0), (1.0, 0.5, 60.0)
    states = [("camera", lambda c: None), ("ray buffer", lambda c: c.set_rays(turned)), ("pose inside the box", lambda c: c.set_pose(W, H, Z, M, inside)),
              ("pose outside the box", lambda c: c.set_pose(W, H, Z, M, outside)), ("camera again", lambda c: c.set_camera(W, H, Z)),
              ("shard", lambda c: c.set_shard(8 * W, 1, 2)), ("shard and supersampling", lambda c: c.set_supersampling(2))]
    want = fresh_aux(objs, rays)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for label, act in states:
            act(rt)
            before, info = snapshot(rt), rt.rays_info()
            assert_query(rt.query_closest(rays), want, label)
            rt.query_occluded(rays)
            rt.pick(np.arange(0, W * H, 97))
            after = snapshot(rt)
            assert_same(after, before, f"{label}: the frame after the queries")
            now = rt.rays_info()
            assert all(np.array_equal(np.asarray(info[k]), np.asarray(now[k])) for k in info), label
        assert before["hits"] > 0
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel="hittest") as rt:   # aux renders around a query
        t0, i0 = rt.render_aux()
        rt.query_closest(rays)
        t1, i1 = rt.render_aux()
        rt.query_occluded(rays)
        t2, i2 = rt.render_aux()
        assert (i0 >= 0).any()
        assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(i0, i1) and np.array_equal(bits(t0), bits(t2)) and np.array_equal(i0, i2)


# ---- 6. pick -------------------------------------------------------------------------------------------------------------------
def work_items(seed=51):
    rng = np.random.default_rng(seed)
    fixed = [0, W * H - 1, W - 1, W, 2 * W - 1, (H - 1) * W, H // 2 * W + W // 2]
    return np.concatenate([fixed, rng.integers(0, W * H, size=50 - len(fixed))]).astype(np.uint64)


def test_pick():
    objs = cloud()
    items = work_items()
    assert len(items) == 50
    M, inside, outside = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0), (1.0, 0.5, 60.0)
    buffer = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    buffer["direction"][5, 3] = 1.0   # a plain buffer, not a pose's: direction.w != 0 somewhere
    cases = [("camera", lambda c: c.set_camera(W, H, Z), None), ("pose inside the box", lambda c: c.set_pose(W, H, Z, M, inside), RY.posed_rays(W, H, Z, M, inside)),
             ("pose outside the box", lambda c: c.set_pose(W, H, Z, M, outside), RY.posed_rays(W, H, Z, M, outside)),
             ("ray buffer", lambda c: c.set_rays(buffer), buffer)]
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for label, act, rays in cases:
            act(rt)
            kw = dict(camera=(W, H, Z)) if rays is None else dict(raygen=False)
            with hip(objs, lights(), rays, 0, kernel="hittest", **kw) as ref:
                wt, wi = ref.render_aux()
            assert (wi[items.astype(np.int64)] >= 0).any() and (wi[items.astype(np.int64)] < 0).any(), label
            want = (wt[items.astype(np.int64)], wi[items.astype(np.int64)])
            assert_query(rt.pick(items), want, label)
            info = rt.query_info()
            assert info["n_rays"] == 50
            if label == "pose outside the box":
                assert info["n_brute"] == 50   # brute force, like any ray from outside the box
            elif label != "ray buffer":
                assert info["n_grid"] == 50
            rt.set_shard(8 * W, 1, 2)          # frame work-items, regardless of the shard
            assert_query(rt.pick(items), want, f"{label}, rank 1 of 2")
            rt.set_shard(0, 0, 1)
            if label != "ray buffer":
                k = int(items[6])
                t, i = rt.pick(k % W, k // W)
                assert bits(np.array([t], dtype=F))[0] == bits(want[0][6:7])[0] and i == want[1][6], label
        with pytest.raises(ValueError):
            rt.pick(3, 4)                      # a plain ray buffer has no grid: work-items only


def test_pick_without_rays_is_refused():
    from opencl_raytracer_amd.hip_raytracer import RTQueryInfo, load_library
    lib = load_library()
    objs, lts = np.ascontiguousarray(cloud()), np.ascontiguousarray(lights())
    ctx = ctypes.c_void_p()
    vp = ctypes.c_void_p
    assert lib.rt_create(ctypes.byref(ctx), objs.ctypes.data_as(vp), len(objs), lts.ctypes.data_as(vp), len(lts), None, W * H, 0, 0, 0, 0) == 0
    try:
        items = np.arange(4, dtype=np.uint64)
        t, i = np.full(4, 5.0, dtype=F), np.full(4, 9, dtype=np.int32)
        assert lib.rt_query_primary(ctx, items.ctypes.data_as(vp), 4, t.ctypes.data_as(vp), i.ctypes.data_as(vp)) == -5   # RT_ERR_STATE
        assert lib.rt_last_error(ctx)
        assert (t == 5.0).all() and (i == 9).all()
        info = RTQueryInfo()
        assert lib.rt_get_query_info(ctx, ctypes.byref(info)) == -5                                                     # no query yet
        rays = in_box_rays(3, seed=1)
        assert lib.rt_query_closest(ctx, rays.ctypes.data_as(vp), 3, t.ctypes.data_as(vp), i.ctypes.data_as(vp)) == 0   # rays of the caller's own need none
        assert lib.rt_get_query_info(ctx, ctypes.byref(info)) == 0 and info.n_rays == 3
    finally:
        lib.rt_destroy(ctx)


# ---- 7. the device form --------------------------------------------------------------------------------------------------------
def test_device_form_behind_a_torch_kernel_on_another_stream():
    import torch
    objs = cloud()
    rays = mixed_rays(4096, seed=61)
    source = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_rays = torch.full_like(source, float("nan"))   # until the torch kernel has run, every ray is a NaN ray
    work = torch.full((2048, 2048), 1.0 / 2048.0, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as dev, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as host:
        with torch.cuda.stream(side):
            for _ in range(8):                          # the stream is busy for a while ...
                work = work @ work
            torch.mul(source, 1.0, out=d_rays)          # ... then a torch kernel writes the rays ...
            t, index = dev.query_closest(d_rays)        # ... immediately before the queries, which are ordered behind it on that stream
            occluded = dev.query_occluded(d_rays)
        assert t.is_cuda and index.is_cuda and occluded.is_cuda and t.dtype == torch.float32 and index.dtype == torch.int32 and occluded.dtype == torch.uint8
        side.synchronize()
        info = dev.query_info()
        assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (4096,) + route_counts(rays)
        ht, hi = host.query_closest(rays)
        assert_query((t.cpu().numpy(), index.cpu().numpy()), (ht, hi), "device form vs host twin")
        assert np.array_equal(occluded.cpu().numpy(), host.query_occluded(rays))
        assert np.array_equal(occluded.cpu().numpy(), predicate(ht))
        assert torch.equal(d_rays.view(torch.int32), source.view(torch.int32))   # the input is unchanged
        assert (hi >= 0).mean() > 0.2
        # the legacy default stream, and an empty tensor
        t0, i0 = dev.query_closest(source)
        torch.cuda.synchronize()
        assert_query((t0.cpu().numpy(), i0.cpu().numpy()), (ht, hi), "default stream")
        te, ie = dev.query_closest(source[:0])
        assert te.numel() == 0 and ie.numel() == 0 and dev.query_occluded(source[:0]).numel() == 0
        with pytest.raises(ValueError):
            dev.query_closest(torch.ones(12, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            dev.query_closest(torch.ones(16, dtype=torch.float32))
    assert_query((ht, hi), fresh_aux(objs, rays), "host twin vs fresh")


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    objs = cloud()
    rays = mixed_rays(16, seed=71)
    vp = ctypes.c_void_p
    r_ptr = rays.ctypes.data_as(vp)
    t, i, o = np.full(16, 5.0, dtype=F), np.full(16, 9, dtype=np.int32), np.full(16, 3, dtype=np.uint8)
    t_ptr, i_ptr, o_ptr = t.ctypes.data_as(vp), i.ctypes.data_as(vp), o.ctypes.data_as(vp)
    d_rays = torch.from_numpy(np.concatenate([rays.view(np.float32).reshape(-1), np.zeros(8, dtype=F)])).cuda()
    d_t = torch.full((16,), 5.0, dtype=torch.float32, device="cuda")
    d_i = torch.full((16,), 9, dtype=torch.int32, device="cuda")
    d_o = torch.full((16,), 3, dtype=torch.uint8, device="cuda")
    items = np.array([0, 1, W * H], dtype=np.uint64)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_visibility(random_mask(N, seed=72))
        mats, xf, vis = rt.read_materials(), rt.read_transforms(), rt.read_visibility()
        before = snapshot(rt)
        first = rt.query_closest(rays)
        info = rt.query_info()
        lib, ctx = rt._lib, rt._ctx
        refused = [lambda: lib.rt_query_closest(ctx, None, 3, t_ptr, i_ptr), lambda: lib.rt_query_occluded(ctx, None, 3, o_ptr),
                   lambda: lib.rt_query_closest(ctx, r_ptr, 16, None, None), lambda: lib.rt_query_occluded(ctx, r_ptr, 16, None),
                   lambda: lib.rt_query_closest_device(ctx, None, 3, vp(d_t.data_ptr()), vp(d_i.data_ptr()), None),
                   lambda: lib.rt_query_closest_device(ctx, vp(d_rays.data_ptr() + 4), 16, vp(d_t.data_ptr()), vp(d_i.data_ptr()), None),   # misaligned
                   lambda: lib.rt_query_closest_device(ctx, vp(d_rays.data_ptr() + 8), 16, vp(d_t.data_ptr()), vp(d_i.data_ptr()), None),
                   lambda: lib.rt_query_closest_device(ctx, vp(d_rays.data_ptr()), 16, None, None, None),
                   lambda: lib.rt_query_occluded_device(ctx, None, 3, vp(d_o.data_ptr()), None),
                   lambda: lib.rt_query_occluded_device(ctx, vp(d_rays.data_ptr() + 4), 16, vp(d_o.data_ptr()), None),
                   lambda: lib.rt_query_occluded_device(ctx, vp(d_rays.data_ptr()), 16, None, None),
                   lambda: lib.rt_query_primary(ctx, items.ctypes.data_as(vp), 3, t_ptr, i_ptr),                                            # a work-item >= the ray count
                   lambda: lib.rt_query_primary(ctx, None, 3, t_ptr, i_ptr), lambda: lib.rt_query_primary(ctx, items.ctypes.data_as(vp), 2, None, None)]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        # n == 0 is RT_OK and launches nothing
        for call in (lambda: lib.rt_query_closest(ctx, None, 0, t_ptr, i_ptr), lambda: lib.rt_query_closest(ctx, r_ptr, 0, t_ptr, None),
                     lambda: lib.rt_query_occluded(ctx, None, 0, o_ptr), lambda: lib.rt_query_closest_device(ctx, None, 0, vp(d_t.data_ptr()), None, None),
                     lambda: lib.rt_query_occluded_device(ctx, vp(d_rays.data_ptr()), 0, vp(d_o.data_ptr()), None),
                     lambda: lib.rt_query_primary(ctx, None, 0, t_ptr, i_ptr)):
            assert call() == 0
        torch.cuda.synchronize()
        assert (t == 5.0).all() and (i == 9).all() and (o == 3).all()
        assert (d_t.cpu().numpy() == 5.0).all() and (d_i.cpu().numpy() == 9).all() and (d_o.cpu().numpy() == 3).all()
        assert rt.query_info() == info                     # the last query is still the last query
        assert np.array_equal(rt.read_visibility(), vis)
        assert np.array_equal(bits(rt.read_materials().view(np.float32)), bits(mats.view(np.float32)))
        assert rt.read_transforms().tobytes() == xf.tobytes()
        assert_same(snapshot(rt), before, "after the refusals")
        assert_query(rt.query_closest(rays), first, "after the refusals")


def test_a_triangle_context_is_refused():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    assert (objs["type"] == 2).all()
    rays = in_box_rays(8, seed=81)
    vp = ctypes.c_void_p
    t, i, o = np.full(8, 5.0, dtype=F), np.full(8, 9, dtype=np.int32), np.full(8, 3, dtype=np.uint8)
    items = np.arange(8, dtype=np.uint64)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = snapshot(rt)
        lib, ctx = rt._lib, rt._ctx
        assert lib.rt_query_closest(ctx, rays.ctypes.data_as(vp), 8, t.ctypes.data_as(vp), i.ctypes.data_as(vp)) == -5   # RT_ERR_STATE
        assert b"triangle" in lib.rt_last_error(ctx)
        assert lib.rt_query_occluded(ctx, rays.ctypes.data_as(vp), 8, o.ctypes.data_as(vp)) == -5
        assert lib.rt_query_primary(ctx, items.ctypes.data_as(vp), 8, t.ctypes.data_as(vp), i.ctypes.data_as(vp)) == -5
        assert (t == 5.0).all() and (i == 9).all() and (o == 3).all()
        assert_same(snapshot(rt), before, "after the refusals")


# ---- 9. several GPUs -----------------------------------------------------------------------------------------------------------
def test_multi_queries_through_shard_0():
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs = cloud()
    rays = mixed_rays(500, seed=91)
    items = work_items()
    mask = random_mask(N, seed=92)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_visibility(mask)
        want, want_occluded, want_pick = rt.query_closest(rays), rt.query_occluded(rays), rt.pick(items)
    with MultiHIPRaytracer(objs, lights(), None, DEPTH, devices=(0, 0), camera=(W, H, Z)) as m:
        frame = m.Render()
        m.set_visibility(mask)
        assert_query(m.query_closest(rays), want, "multi")
        assert m.query_info()["n_rays"] == 500
        assert np.array_equal(m.query_occluded(rays), want_occluded)
        assert_query(m.pick(items), want_pick, "multi pick")
        m.set_visibility(np.ones(N, dtype=np.uint8))
        assert np.array_equal(bits(m.Render()), bits(frame))
    assert (want[1] >= 0).any() and not np.isin(want[1][want[1] >= 0], np.nonzero(mask == 0)[0]).any()


# ---- 10. literal contexts ------------------------------------------------------------------------------------------------------
def with_a_degenerate_object(objs, where, kind):
    """The cloud with object `where` made degenerate: a singular but finite mvInverse (t = 0 / 0 for EVERY ray: a NaN time that
    overwrites and is overwritten, so the result depends on the order of the loop) or what the inverse of a scale of 0 holds."""
    out = objs.copy()
    inv = out["mvInverse"][where].reshape(4, 4).copy()   # column-major: [c][r]
    if kind == "zero":
        inv[:3, :3] = 0.0
    else:
        inv[2, 2] = np.inf
        inv[3, 2] = np.nan
        out["mv"][where].reshape(4, 4)[2, 2] = 0.0
    out["mvInverse"][where] = inv.reshape(16)
    return out


@pytest.mark.parametrize("kind", ["zero", "inf"])
def test_a_degenerate_instance_sends_every_ray_to_the_ordered_loop(kind):
    base = cloud()
    where = int(np.nonzero(base["type"] == R.SPHERE)[0][60])   # a sphere between objects of lower and of higher index
    assert 20 < where < N - 20
    objs = with_a_degenerate_object(base, where, kind)
    rays = mixed_rays(1024, seed=101)
    want = fresh_aux(objs, rays)
    plain = fresh_aux(base, rays)
    assert not np.array_equal(bits(want[0]), bits(plain[0]))                  # the instance is met: the answers are not the cloud's
    if kind == "zero":
        assert np.isnan(want[0][np.arange(1024) % 4 != 3]).any()             # NaN times on finite rays from inside the box
    for kernel in ("shade_and_reflect", "hittest"):
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel=kernel) as rt:
            info = rt.rays_info()
            assert info["grid_built"] == 1 and info["literal"] == 1           # a grid is built all the same: it must not answer
            assert_query(rt.query_closest(rays), want, f"degenerate {kind} {kernel}")
            q = rt.query_info()
            assert (q["n_rays"], q["n_grid"], q["n_brute"]) == (1024, 0, 1024)
            assert (q["n_grid"], q["n_brute"]) == route_counts(rays, grid=False)
            assert np.array_equal(rt.query_occluded(rays), predicate(want[0]))
            assert rt.query_info()["n_grid"] == 0
            items = work_items()
            with hip(objs, lights(), None, 0, kernel="hittest", camera=(W, H, Z)) as ref:
                wt, wi = ref.render_aux()
            assert_query(rt.pick(items), (wt[items.astype(np.int64)], wi[items.astype(np.int64)]), f"degenerate {kind} {kernel}: pick")
            assert rt.query_info()["n_grid"] == 0
    ct, ci = CPURaytracer(objs, lights(), rays[:1], 0, kernel="hittest").query_closest(rays)
    assert same_floats(want[0], ct) and np.array_equal(want[1], ci)           # the definition without a GPU agrees


def test_a_context_created_literal_answers_by_the_ordered_loop():
    objs = cloud()
    rays = mixed_rays(512, seed=103)
    want = fresh_aux(objs, rays)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), literal=True) as rt:
        assert_query(rt.query_closest(rays), want, "literal=True")
        q = rt.query_info()
        assert (q["n_grid"], q["n_brute"]) == (0, 512)
        assert np.array_equal(rt.query_occluded(rays), predicate(want[0]))
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:               # a FRAME literal for its own rays only: queries keep the grid
        rt.set_camera(W, H, 0.0)                                                 # z = 0: the centre pixel's direction is (0, 0, 0)
        info = rt.rays_info()
        assert info["literal"] == 1 and info["grid_built"] == 1 and info["directions_in_domain"] == 0
        assert_query(rt.query_closest(rays), want, "literal for the frame's rays")
        q = rt.query_info()
        assert (q["n_grid"], q["n_brute"]) == route_counts(rays) and q["n_grid"] > 0


# ---- 11. plain float32 arrays --------------------------------------------------------------------------------------------------
def test_rays_as_an_n_by_8_float32_array():
    import torch
    objs = cloud()
    rays = mixed_rays(300, seed=111)
    plain = rays.view(np.float32).reshape(-1, 8).copy()
    assert plain.shape == (300, 8) and plain.dtype == np.float32
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        want, want_occluded = rt.query_closest(rays), rt.query_occluded(rays)
        info = rt.query_info()
        assert_query(rt.query_closest(plain), want, "(n, 8) float32")
        assert np.array_equal(rt.query_occluded(plain), want_occluded)
        assert rt.query_info()["n_rays"] == 300 and rt.query_info()["n_grid"] == info["n_grid"]
        back = torch.from_numpy(plain).cuda().cpu().numpy()                    # what a torch user holds
        assert_query(rt.query_closest(back), want, "tensor.cpu().numpy()")
        assert_query(rt.query_closest(plain[::-1][::-1]), want, "a view")
        t1, i1 = rt.query_closest(plain[7])                                   # one ray, shape (8,)
        assert t1.shape == (1,) and bits(t1)[0] == bits(want[0])[7] and i1[0] == want[1][7]
        for bad in (plain[:, :7], plain.astype(np.float64), plain.reshape(-1), np.float32(1.0)):   # (flat: the last dimension is 8 n)
            with pytest.raises(ValueError):
                rt.query_closest(bad)
        with pytest.raises(ValueError):
            rt.query_occluded(plain[:, :4])
    assert_query(want, fresh_aux(objs, rays), "vs fresh")
    assert (want[1] >= 0).mean() > 0.2
