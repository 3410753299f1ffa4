"""GPU: hit-record queries (hip_raytracer.h, "hit-record queries") - rt_query_hits_device, rt_query_hits, rt_query_primary_hits -
against FRESH hittest contexts for (t, index), and for the records against the CPU backend's query_hits (the default arithmetic),
hits.hit_records (RT_FLAG_UNFUSED) and bounds derived from the two normalisations (RT_FLAG_DEVICE_OPENCL). Scenes and rays are
test_query_gpu.py's: the 200-object cloud (a grid) and its first 40 objects (no grid).

5. launch boundaries, the guard behind element n - 1, every selection of outputs;
6. both routes in every wave;
7. every arithmetic mode on both scenes, RT_FLAG_FAST_PHONG, the zero box normal per mode;
8. the live state is what is queried, and a query leaves the frame alone;
9. a three-bounce chain with the mask: separate buffers, in place, and from a torch tensor on a side stream;
10. pick_hit; 11. refusals touch nothing; 12. MultiHIPRaytracer through shard 0.
(The numbering goes on from test_query_hits_cpu.py's 1-4; the C++ flavour is test_host_hits_gpu.py's.)"""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import R, rotation, same_floats
from opencl_raytracer_amd import hits as HT
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from opencl_raytracer_amd.hip_raytracer import HIT_FIELDS, RTError, RTHits
from test_frame_shapes_cpu import camera_z_for, scene
from test_primary_depth_order_gpu import bits, hip
from test_query_gpu import MODES, assert_query, cloud_box, fresh_aux, in_box_rays, mixed_rays, route_counts, work_items
from test_query_hits_cpu import tiny_far_box
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, lights, small, snapshot
from test_set_transforms_gpu import three_moves
from test_set_visibility_gpu import random_mask

pytestmark = pytest.mark.gpu
F = np.float32
MAX_FLOAT = F(3.402823466e+38)
U = 2.0 ** -23
RECORDS = ("point", "normal", "reflected")
VP = ctypes.c_void_p


def flat(a):
    """A record array as float32 numbers, one row per ray (RAY_DTYPE: 8 per ray)."""
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) if a.dtype == R.RAY_DTYPE else a).reshape(len(a), -1)


def numpy_of(h):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in h.items()}


def cpu_backend(objs):
    return CPURaytracer(objs, lights(), in_box_rays(1, 1), 0, kernel="hittest")


def same_bits_or_nan(a, b):
    """Bit for bit, but a NaN on both sides counts as equal: a NaN's payload is the hardware's."""
    a, b = flat(a), flat(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_records(got, want, label, keys=RECORDS, same=same_floats):
    for k in keys:
        a, b = flat(got[k]), flat(want[k])
        assert a.shape == b.shape, (label, k, a.shape, b.shape)
        assert same(a, b), f"{label}: {k} differs on {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=1).sum())} rays"


def assert_zero_where_missed(h, label):
    miss = h["index"] < 0
    for k in RECORDS:
        if k in h:
            assert not bits(flat(h[k])[miss]).any(), f"{label}: {k} of a miss is not all-zero bytes"


def assert_exact(a, b, label):
    for k in a:
        assert np.array_equal(bits(flat(a[k])) if k != "index" else a[k], bits(flat(b[k])) if k != "index" else b[k]), f"{label}: {k}"


# ---- 5. launch boundaries ------------------------------------------------------------------------------------------------------
GUARD = {"t": -7.25, "index": -77, "point": -3.5, "normal": 9.75, "reflected": 1.25}


def guarded(n):
    import torch
    shapes = {"t": ((n + 1,), torch.float32), "index": ((n + 1,), torch.int32), "point": ((n + 1, 4), torch.float32),
              "normal": ((n + 1, 4), torch.float32), "reflected": ((n + 1, 8), torch.float32)}
    return {k: torch.full(s, GUARD[k], dtype=d, device="cuda") for k, (s, d) in shapes.items()}


def test_launch_boundaries():
    import torch
    objs = cloud()
    all_rays = mixed_rays(1000, seed=5)
    want_all = cpu_backend(objs).query_hits(all_rays)
    subsets = [c for r in range(1, 6) for c in itertools.combinations(HIT_FIELDS, r)]
    assert len(subsets) == 31
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            rays = all_rays[:n]
            want = {k: v[:n] for k, v in want_all.items()}
            fresh = fresh_aux(objs, rays)
            got = rt.query_hits(rays)
            assert_query((got["t"], got["index"]), fresh, f"n = {n}")
            assert_records(got, want, f"n = {n}")
            assert_zero_where_missed(got, f"n = {n}")
            info = rt.query_info()
            assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (n,) + route_counts(rays), n
            # the device form into buffers of n + 1 elements, for every selection of outputs: the guard element of every output
            # stays, an output that was not asked for is not written at all
            d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
            for chosen in subsets:
                out = guarded(n)
                hits = RTHits(**{k: out[k].data_ptr() for k in chosen})
                assert rt._lib.rt_query_hits_device(rt._ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(hits), None) == 0, (n, chosen)
                torch.cuda.synchronize()
                for k, tensor in out.items():
                    a = tensor.cpu().numpy()
                    if k in chosen:
                        assert np.array_equal(bits(flat(a[:n])) if k != "index" else a[:n], bits(flat(got[k])) if k != "index" else got[k]), (n, chosen, k)
                        assert (a[n:] == GUARD[k]).all(), (n, chosen, k, "guard")
                    else:
                        assert (a == GUARD[k]).all(), (n, chosen, k, "not asked for")
            none = RTHits()
            assert rt._lib.rt_query_hits_device(rt._ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(none), None) == -1
            # the Python front's `want`
            only = rt.query_hits(rays, want=("normal",))
            assert list(only) == ["normal"] and np.array_equal(bits(only["normal"]), bits(got["normal"]))
        with pytest.raises(ValueError):
            rt.query_hits(all_rays, want=())
        with pytest.raises(ValueError):
            rt.query_hits(all_rays, want=("colour",))
    hit = want_all["index"] >= 0
    assert hit.sum() > 300 and (~hit).sum() > 100


# ---- 6. both routes in every wave ----------------------------------------------------------------------------------------------
def test_mixed_routes_in_one_wave():
    objs = cloud()
    n = 1024
    rays = mixed_rays(n, seed=14)
    on = RY.query_route(rays, *cloud_box())
    per_wave = on.reshape(-1, 64).sum(axis=1)
    assert (per_wave > 0).all() and (per_wave < 64).all()
    want = cpu_backend(objs).query_hits(rays)
    assert (want["index"][on] >= 0).sum() >= 100 and (want["index"][~on] >= 0).sum() >= 50    # records on both routes
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        got = rt.query_hits(rays)
        info = rt.query_info()
    assert_query((got["t"], got["index"]), fresh_aux(objs, rays), "mixed routes")
    assert (info["n_rays"], info["n_grid"], info["n_brute"]) == (n, int(on.sum()), int((~on).sum()))
    assert_records({k: v[~on] for k, v in got.items()}, {k: v[~on] for k, v in want.items()}, "brute-force lanes")
    assert_records({k: v[on] for k, v in got.items()}, {k: v[on] for k, v in want.items()}, "grid lanes")
    assert_zero_where_missed(got, "mixed routes")


# ---- 7. arithmetic modes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_arithmetic_mode(mode, size, capsys):
    objs = cloud() if size == "large" else small()
    rays = mixed_rays(1000, seed=21)
    fresh = fresh_aux(objs, rays, **MODES[mode])
    cpu = cpu_backend(objs)
    for kernel in ("shade_and_reflect", "hittest"):
        label = f"{mode} {size} {kernel}"
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel=kernel, **MODES[mode]) as rt:
            got = rt.query_hits(rays)
            info = rt.query_info()
        assert_query((got["t"], got["index"]), fresh, label)
        assert (info["n_grid"], info["n_brute"]) == route_counts(rays, grid=size == "large")
        assert_zero_where_missed(got, label)
        hit = got["index"] >= 0
        assert hit.sum() > 100
        if mode == "default":
            assert_records(got, cpu.query_hits(rays), label, same=same_bits_or_nan)
        elif mode == "unfused":
            assert_records(got, HT.hit_records(objs, rays, got["t"], got["index"]), label)
        else:
            # the record stage of the default arithmetic at the GPU's own (t, index): row4 and fma_ are the same under kFused and
            # kDeviceCL, so the point is the same number; the two normalisations are the device's (each within about 3 units of
            # 2^-23 of the exact normalisation of the same vector; r = d - 2 (d . n) n roughly quadruples the normal's error)
            stage = cpu.hit_records(rays, got["t"], got["index"])
            assert_records(got, stage, label, keys=("point",), same=same_bits_or_nan)
            fin = hit & np.isfinite(flat(stage["reflected"])).all(axis=1) & np.isfinite(stage["normal"]).all(axis=1)
            assert fin.sum() > 100 and np.isfinite(flat(got["reflected"])[fin]).all()
            dn = np.abs(got["normal"][fin].astype(np.float64) - stage["normal"][fin]).max(axis=1)
            d_len = np.linalg.norm(rays["direction"][fin, :3].astype(np.float64), axis=1)
            dr = np.abs(got["reflected"]["direction"][fin].astype(np.float64) - stage["reflected"]["direction"][fin]).max(axis=1) / d_len
            p_inf = np.maximum(1.0, np.abs(got["point"][fin, :3].astype(np.float64)).max(axis=1))
            ds = np.abs(got["reflected"]["start"][fin].astype(np.float64) - stage["reflected"]["start"][fin]).max(axis=1)
            start_bound = 4 * U * p_inf + 0.001 * 128 * U
            with capsys.disabled():
                print(f"\n[device_opencl records, {size} {kernel}: {int(fin.sum())} hits] normal {dn.max() / U:.2f} x 2^-23 (bound 16); reflected "
                      f"direction {dr.max() / U:.2f} x 2^-23 |d| (bound 128); reflected start {(ds / start_bound).max():.3f} of its bound")
            assert dn.max() <= 16 * U and dr.max() <= 128 * U and (ds <= start_bound).all()


def test_fast_phong_plays_no_part():
    rays = mixed_rays(1000, seed=21)
    for objs in (cloud(), small()):
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as plain, hip(objs, lights(), None, DEPTH, camera=(W, H, Z), fast_phong=True) as fast:
            a, b = plain.query_hits(rays), fast.query_hits(rays)
        assert_exact(a, b, "fast_phong")
        assert (a["index"] >= 0).sum() > 100


def test_the_zero_box_normal_follows_its_mode():
    objs, rays = tiny_far_box()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        d = rt.query_hits(rays)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), fused=False) as rt:
        u = rt.query_hits(rays)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), device_opencl=True) as rt:
        c = rt.query_hits(rays)
    cpu = CPURaytracer(objs, lights(), rays[:1], 0, kernel="hittest")
    assert_records(d, cpu.query_hits(rays), "default", same=same_bits_or_nan)
    assert_records(u, HT.hit_records(objs, rays, u["t"], u["index"]), "unfused")
    for h in (d, u):   # default and unfused: a NaN normal and a NaN reflected ray, on at least 16 hits; finite ones on at least 16
        hit = h["index"] >= 0
        nan_normal = hit & np.isnan(h["normal"][:, :3]).all(axis=1)
        assert nan_normal.sum() >= 16 and (hit & np.isfinite(h["normal"]).all(axis=1)).sum() >= 16
        assert np.isnan(flat(h["reflected"])[nan_normal][:, [0, 1, 2, 4, 5, 6]]).all()
    # device arithmetic: normalize(0) = 0. The object-space point is the default arithmetic's at the same t, so the zero normals are
    # where the default record stage AT THE DEVICE'S t has its NaN normals, and - on the rays whose t has the same bits in both
    # modes - where the default-mode query has them
    hit = c["index"] >= 0
    assert hit.sum() >= 500 and np.isfinite(flat(c["reflected"])).all() and np.isfinite(c["normal"]).all()
    zero = hit & (c["normal"] == 0).all(axis=1)
    stage = cpu.hit_records(rays, c["t"], c["index"])
    assert np.array_equal(zero, np.isnan(stage["normal"][:, :3]).all(axis=1))
    same_t = bits(c["t"]) == bits(d["t"])
    assert same_t.sum() >= 256
    assert np.array_equal(zero[same_t], np.isnan(d["normal"][:, :3]).all(axis=1)[same_t])
    assert zero.sum() >= 16 and (zero & same_t).sum() >= 16
    # ... and the reflection goes on along d, from 0.001 further along it
    assert same_floats(c["reflected"]["direction"][zero], rays["direction"][zero])
    step = np.linalg.norm(c["reflected"]["start"][zero, :3].astype(np.float64) - c["point"][zero, :3], axis=1)
    assert (np.abs(step - 0.001) <= 4 * U * 1000.0).all()


# ---- 8. live state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_live_state_is_what_is_queried(size):
    objs = cloud() if size == "large" else small()
    moves = three_moves(objs)
    rays = mixed_rays(768, seed=31)
    rays["start"][0] = (-5.0, 1.0, -30.0, 1.0)     # along x through the place the first moved object arrives at
    rays["direction"][0] = (1.0, 0.0, 0.0, 0.0)
    mask = random_mask(len(objs), seed=33)
    mask[moves[0][0]] = 1
    hidden = np.nonzero(mask == 0)[0]
    cpu = cpu_backend(objs)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        untouched = rt.query_hits(rays)
        assert_records(untouched, cpu.query_hits(rays), f"{size}: untouched", keys=HIT_FIELDS)
        assert_same(snapshot(rt), before, "a render before and after a query")
        assert untouched["index"][0] == -1
        for i, t in moves:
            rt.set_transforms(t, i)
            cpu.set_transforms(t, i)
        moved = rt.query_hits(rays)
        assert_records(moved, cpu.query_hits(rays), f"{size}: moved", keys=HIT_FIELDS)
        assert moved["index"][0] == moves[0][0] and np.isfinite(moved["normal"][0]).all()
        frame_moved = snapshot(rt)
        rt.set_visibility(mask)
        cpu.set_visibility(mask)
        both = rt.query_hits(rays)
        assert_records(both, cpu.query_hits(rays), f"{size}: moved and masked", keys=HIT_FIELDS)
        assert not np.isin(both["index"][both["index"] >= 0], hidden).any()
        assert not np.array_equal(both["index"], moved["index"])
        assert_zero_where_missed(both, size)
        rt.set_visibility(np.ones(len(objs), dtype=np.uint8))      # hide, then show: the moved scene again
        cpu.set_visibility(np.ones(len(objs), dtype=np.uint8))
        again = rt.query_hits(rays)
        assert_exact(again, moved, f"{size}: shown again")
        assert_records(again, cpu.query_hits(rays), f"{size}: shown again", keys=HIT_FIELDS)
        assert_same(snapshot(rt), frame_moved, "the frame after the queries")


# ---- 9. chain and mask ---------------------------------------------------------------------------------------------------------
def test_a_three_bounce_chain_with_the_mask():
    import torch
    objs = cloud()
    n = 1000
    rays = mixed_rays(n, seed=91)
    lo, hi = cloud_box()
    want = HT.chain(cpu_backend(objs).query_hits, rays, 3)
    hits_per_bounce = [int((w["index"] >= 0).sum()) for w in want]
    assert hits_per_bounce[0] > 300 and hits_per_bounce[1] > 50 and hits_per_bounce[2] > 10 and hits_per_bounce[0] > hits_per_bounce[1] > hits_per_bounce[2]
    source = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        # (a) separate buffers, with the counters of every bounce
        infos = []

        def query(r, m):
            res = rt.query_hits(r, m)
            infos.append(rt.query_info())
            return res
        separate = [numpy_of(h) for h in HT.chain(query, source, 3)]
        # (b) in place: reflected == rays and index == mask
        buf, idx = source.clone(), torch.zeros(n, dtype=torch.int32, device="cuda")
        in_place = []
        for _ in range(3):
            res = rt.query_hits(buf, idx, out={"reflected": buf, "index": idx})
            assert res["reflected"] is buf and res["index"] is idx
            in_place.append(numpy_of({k: v.clone() for k, v in res.items()}))
        # (c) from a torch tensor on a side stream, behind the torch kernel that makes the rays
        d_rays = torch.full_like(source, float("nan"))
        work = torch.full((1024, 1024), 1.0 / 1024.0, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(4):
                work = work @ work
            torch.mul(source, 1.0, out=d_rays)
            streamed = HT.chain(rt.query_hits, d_rays, 3)
        side.synchronize()
        streamed = [numpy_of(h) for h in streamed]
        # the host twin follows the same chain
        twin = HT.chain(rt.query_hits, rays, 3)
    for k in range(3):
        label = f"bounce {k + 1}"
        assert_exact(in_place[k], separate[k], f"{label}: in place")
        assert_exact(streamed[k], separate[k], f"{label}: side stream")
        assert_exact(twin[k], separate[k], f"{label}: host twin")
        assert_records(separate[k], want[k], label, keys=HIT_FIELDS, same=same_bits_or_nan)
        assert_zero_where_missed(separate[k], label)
        traced = np.ones(n, dtype=bool) if k == 0 else separate[k - 1]["index"] >= 0
        assert (separate[k]["index"][~traced] == -1).all() and (separate[k]["t"][~traced] == MAX_FLOAT).all()   # masked rays stay zero records
        assert infos[k]["n_rays"] == int(traced.sum()) == (n if k == 0 else hits_per_bounce[k - 1]), label
        bounce_rays = rays if k == 0 else R.rays_of(separate[k - 1]["reflected"])
        off_grid = ~RY.query_route(bounce_rays[traced], lo, hi)
        assert infos[k]["n_brute"] == int(off_grid.sum()) and infos[k]["n_grid"] == int((~off_grid).sum()), label   # no miss was traced by brute force
    assert infos[1]["n_grid"] > 0


# ---- 10. pick_hit --------------------------------------------------------------------------------------------------------------
def camera_rays():
    """The in-kernel pinhole grid of rt_set_camera(W, H, Z), ray by ray."""
    rays = np.zeros(W * H, dtype=R.RAY_DTYPE)
    col, row = np.tile(np.arange(W), H).astype(F), np.repeat(np.arange(H), W).astype(F)
    rays["start"][:, 3] = 1.0
    rays["direction"][:, 0] = col - F(W) / F(2.0)
    rays["direction"][:, 1] = (F(H) - row) - F(H) / F(2.0)
    rays["direction"][:, 2] = F(Z)
    return rays


def test_pick_hit():
    objs = cloud()
    items = work_items()
    M, inside = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0)
    buffer = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    buffer["direction"][5, 3] = 1.0   # a plain buffer, not a pose's
    cases = [("camera", lambda c: c.set_camera(W, H, Z), camera_rays()), ("pose inside the box", lambda c: c.set_pose(W, H, Z, M, inside), RY.posed_rays(W, H, Z, M, inside)),
             ("ray buffer", lambda c: c.set_rays(buffer), buffer)]
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for label, act, rays in cases:
            act(rt)
            want = rt.query_hits(rays[items.astype(np.int64)])
            assert (want["index"] >= 0).any() and (want["index"] < 0).any(), label
            got = rt.pick_hit(items)
            assert_exact(got, want, label)
            assert rt.query_info()["n_rays"] == len(items)
            assert_exact(rt.pick_hit(items, want=("point",)), {"point": want["point"]}, label)
            if label != "ray buffer":
                k = int(np.nonzero(want["index"] >= 0)[0][0])
                one = rt.pick_hit(int(items[k]) % W, int(items[k]) // W)
                assert isinstance(one["t"], float) and one["index"] == want["index"][k] and F(one["t"]) == want["t"][k]
                assert np.array_equal(bits(one["point"]), bits(want["point"][k])) and np.array_equal(bits(one["normal"]), bits(want["normal"][k]))
                assert one["reflected"].tobytes() == want["reflected"][k].tobytes()
        with pytest.raises(ValueError):
            rt.pick_hit(3, 4)                  # a plain ray buffer has no grid: work-items only


def test_pick_hit_without_rays_is_refused():
    from opencl_raytracer_amd.hip_raytracer import load_library
    lib = load_library()
    objs, lts = np.ascontiguousarray(cloud()), np.ascontiguousarray(lights())
    ctx = VP()
    assert lib.rt_create(ctypes.byref(ctx), objs.ctypes.data_as(VP), len(objs), lts.ctypes.data_as(VP), len(lts), None, W * H, 0, 0, 0, 0) == 0
    try:
        items = np.arange(4, dtype=np.uint64)
        point = np.full((4, 4), 5.0, dtype=F)
        hits = RTHits(point=point.ctypes.data)
        assert lib.rt_query_primary_hits(ctx, items.ctypes.data_as(VP), 4, ctypes.byref(hits)) == -5   # RT_ERR_STATE
        assert lib.rt_last_error(ctx) and (point == 5.0).all()
        rays = in_box_rays(3, seed=1)
        assert lib.rt_query_hits(ctx, rays.ctypes.data_as(VP), 3, None, ctypes.byref(hits)) == 0         # rays of the caller's own need none
        assert not (point[:3] == 5.0).all() and (point[3] == 5.0).all()
    finally:
        lib.rt_destroy(ctx)


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    import torch
    objs = cloud()
    n = 16
    rays = mixed_rays(n, seed=71)
    d_rays = torch.from_numpy(np.concatenate([rays.view(np.float32).reshape(-1), np.zeros(8, dtype=F)])).cuda()
    out = guarded(n + 1)
    host = {"t": np.full(n, 5.0, dtype=F), "index": np.full(n, 9, dtype=np.int32), "point": np.full((n, 4), 5.0, dtype=F)}
    h_hits = RTHits(**{k: v.ctypes.data for k, v in host.items()})
    items = np.array([0, 1, W * H], dtype=np.uint64)
    r_ptr = rays.ctypes.data_as(VP)

    def dev(rays_at=0, mask_at=None, **offsets):
        hits = RTHits(**{k: out[k].data_ptr() + offsets.get(k, 0) for k in HIT_FIELDS})
        mask = None if mask_at is None else VP(out["index"].data_ptr() + mask_at)
        return lambda: rt._lib.rt_query_hits_device(rt._ctx, VP(d_rays.data_ptr() + rays_at), n, mask, ctypes.byref(hits), None)

    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        first = rt.query_hits(rays)
        info = rt.query_info()
        lib, ctx = rt._lib, rt._ctx
        refused = [dev(point=4), dev(point=8), dev(normal=4), dev(reflected=16 + 4), dev(reflected=8), dev(rays_at=4), dev(rays_at=8), dev(t=2), dev(index=1),
                   dev(mask_at=2),
                   lambda: lib.rt_query_hits_device(ctx, None, 3, None, ctypes.byref(RTHits(t=out["t"].data_ptr())), None),      # NULL rays, n != 0
                   lambda: lib.rt_query_hits_device(ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(RTHits()), None),         # all outputs NULL
                   lambda: lib.rt_query_hits_device(ctx, VP(d_rays.data_ptr()), n, None, None, None),                            # no struct
                   lambda: lib.rt_query_hits(ctx, None, 3, None, ctypes.byref(h_hits)), lambda: lib.rt_query_hits(ctx, r_ptr, n, None, ctypes.byref(RTHits())),
                   lambda: lib.rt_query_hits(ctx, r_ptr, n, None, None),
                   lambda: lib.rt_query_primary_hits(ctx, items.ctypes.data_as(VP), 3, ctypes.byref(h_hits)),                    # a work-item >= the ray count
                   lambda: lib.rt_query_primary_hits(ctx, None, 3, ctypes.byref(h_hits)),
                   lambda: lib.rt_query_primary_hits(ctx, items.ctypes.data_as(VP), 2, ctypes.byref(RTHits()))]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        # n == 0 is RT_OK and launches nothing
        for call in (lambda: lib.rt_query_hits(ctx, None, 0, None, ctypes.byref(h_hits)),
                     lambda: lib.rt_query_hits_device(ctx, None, 0, None, ctypes.byref(RTHits(t=out["t"].data_ptr())), None),
                     lambda: lib.rt_query_primary_hits(ctx, None, 0, ctypes.byref(h_hits))):
            assert call() == 0
        torch.cuda.synchronize()
        for k, tensor in out.items():
            assert (tensor.cpu().numpy() == GUARD[k]).all(), k
        assert (host["t"] == 5.0).all() and (host["index"] == 9).all() and (host["point"] == 5.0).all()
        assert rt.query_info() == info                     # the last query is still the last query
        assert_same(snapshot(rt), before, "the frame after the refusals")
        assert_exact(rt.query_hits(rays), first, "after the refusals")


def test_a_triangle_context_is_refused():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    rays = in_box_rays(8, seed=81)
    point = np.full((8, 4), 5.0, dtype=F)
    hits = RTHits(point=point.ctypes.data)
    items = np.arange(8, dtype=np.uint64)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = snapshot(rt)
        lib, ctx = rt._lib, rt._ctx
        assert lib.rt_query_hits(ctx, rays.ctypes.data_as(VP), 8, None, ctypes.byref(hits)) == -5   # RT_ERR_STATE
        assert b"triangle" in lib.rt_last_error(ctx)
        assert lib.rt_query_primary_hits(ctx, items.ctypes.data_as(VP), 8, ctypes.byref(hits)) == -5
        with pytest.raises(RTError):
            rt.query_hits(rays)
        assert (point == 5.0).all()
        assert_same(snapshot(rt), before, "after the refusals")


# ---- 12. several GPUs ----------------------------------------------------------------------------------------------------------
def test_multi_queries_through_shard_0():
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs = cloud()
    rays = mixed_rays(500, seed=92)
    items = work_items()
    mask = random_mask(N, seed=93)
    ray_mask = np.where(np.arange(500) % 5 == 0, -1, 0).astype(np.int32)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_visibility(mask)
        want, want_masked, want_pick = rt.query_hits(rays), rt.query_hits(rays, ray_mask), rt.pick_hit(items)
    with MultiHIPRaytracer(objs, lights(), None, DEPTH, devices=(0, 0), camera=(W, H, Z)) as m:
        frame = m.Render()
        m.set_visibility(mask)
        assert_exact(m.query_hits(rays), want, "multi")
        assert m.query_info()["n_rays"] == 500
        assert_exact(m.query_hits(rays, ray_mask), want_masked, "multi, masked")
        assert m.query_info()["n_rays"] == 400
        assert_exact(m.pick_hit(items), want_pick, "multi pick_hit")
        m.set_visibility(np.ones(N, dtype=np.uint8))
        assert np.array_equal(bits(m.Render()), bits(frame))
    assert (want["index"] >= 0).any() and (want_masked["index"][ray_mask < 0] == -1).all()
    assert not np.isin(want["index"][want["index"] >= 0], np.nonzero(mask == 0)[0]).any()
