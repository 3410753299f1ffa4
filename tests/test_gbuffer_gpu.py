"""GPU: G-buffer frames (hip_raytracer.h, "G-buffer frames") - rt_render_gbuffer_device, rt_render_gbuffer, rt_get_gbuffer_info.

1. record agreement: render_gbuffer() against pick_hit over all work-items, bit for bit, in every arithmetic mode on the grid scene and
   the no-grid scene; albedo against read_materials;
2. launch boundaries: ray-buffer contexts of 1 .. 1000 mixed rays (the literal and brute-force frame routes), the guard element, all 31
   selections of outputs;
3. frame shapes: a width that is no multiple of 8, row tiles and tiles that are no whole rows, a ragged last tile, world = 3;
4. poses inside and one box diagonal outside the grid's box (the screen-tile route, tiles_info().source == 3);
5. live state: set_transforms, set_visibility, set_materials; 6. the frame is untouched (aux pair, stats, timing, supersampling);
7. triangles; 8. a hittest context, a side stream, refusals, an empty shard.
Scenes and helpers are test_query_hits_gpu.py's: 64 x 48 frames of the 200-object cloud (a grid) and its first 40 objects."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import R, camera
from opencl_raytracer_amd import hits as HT
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.tessellate import TRIANGLE
from opencl_raytracer_amd.hip_raytracer import GBUFFER_FIELDS, RTError, RTGBuffer
from test_frame_shapes_cpu import camera_z_for, pinhole_rays, scene
from test_primary_depth_order_gpu import bits, hip
from test_query_gpu import MODES, assert_query, cloud_box, fresh_aux, mixed_rays
from test_query_hits_gpu import same_bits_or_nan
from test_set_materials_cpu import new_materials
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, lights, small, snapshot
from test_set_transforms_gpu import three_moves
from test_set_visibility_gpu import random_mask

pytestmark = pytest.mark.gpu
F = np.float32
MAX_FLOAT = F(3.402823466e+38)
VP = ctypes.c_void_p
RECORDS = ("point", "normal")


def assert_gbuffer(got, want, label, keys=("t", "index", "point", "normal")):
    for k in keys:
        assert got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        ok = np.array_equal(got[k], want[k]) if k == "index" else same_bits_or_nan(got[k], want[k])
        assert ok, f"{label}: {k} differs"


def assert_albedo(rt, g, label):
    mats = rt.read_materials()
    hit = g["index"] >= 0
    want = np.zeros((len(hit), 4), dtype=F)
    want[hit, :3] = mats["diffuse"][g["index"][hit]][:, :3]
    want[hit, 3] = 1.0
    assert same_bits_or_nan(g["albedo"], want), f"{label}: albedo"
    assert not bits(g["albedo"][~hit]).any(), f"{label}: albedo of a miss is not zero bytes"


def assert_zero_where_missed(g, label):
    miss = g["index"] < 0
    for k in ("point", "normal", "albedo"):
        if k in g:
            assert not bits(g[k][miss]).any(), f"{label}: {k} of a miss is not all-zero bytes"


def global_items(n_rays, tile_rays, rank, world, n_local):
    """global_ray_of's mapping on the local pixel index (rt_wavefront.hip); entries >= n_rays are padding."""
    i = np.arange(n_local, dtype=np.int64)
    if world <= 1:
        return i
    run = i // tile_rays
    return (run * world + rank) * tile_rays + (i - run * tile_rays)


# ---- 1. record agreement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
@pytest.mark.parametrize("mode", list(MODES))
def test_records_equal_the_primary_hit_queries(mode, size):
    objs = cloud() if size == "large" else small()
    items = np.arange(W * H, dtype=np.uint64)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), **MODES[mode]) as rt:
        g = rt.render_gbuffer()
        info = rt.gbuffer_info()
        want = rt.pick_hit(items)
        assert_gbuffer(g, want, f"{mode} {size}")
        assert_albedo(rt, g, f"{mode} {size}")
        rays = pinhole_rays(W, H, Z)
        assert_gbuffer(g, rt.query_hits(rays), f"{mode} {size}: query_hits")
        rt.Render()
        assert info["wavefront"] == int(rt.stats().wavefront)       # the pass takes the frame's route
    assert_zero_where_missed(g, f"{mode} {size}")
    hit = g["index"] >= 0
    assert hit.sum() > 300 and (~hit).sum() > 300
    assert (info["n_items"], info["hits"]) == (W * H, int(hit.sum())) and info["trace_ms"] > 0 and info["records_ms"] > 0
    assert_query((g["t"], g["index"]), fresh_aux(objs, rays, **MODES[mode]), f"{mode} {size}: fresh hittest context")


# ---- 2. launch boundaries --------------------------------------------------------------------------------------------------------
GUARD = {"t": -7.25, "index": -77, "point": -3.5, "normal": 9.75, "albedo": 1.25}


def guarded(n):
    import torch
    shapes = {"t": ((n + 1,), torch.float32), "index": ((n + 1,), torch.int32), "point": ((n + 1, 4), torch.float32),
              "normal": ((n + 1, 4), torch.float32), "albedo": ((n + 1, 4), torch.float32)}
    return {k: torch.full(s, GUARD[k], dtype=d, device="cuda") for k, (s, d) in shapes.items()}


def test_launch_boundaries():
    import torch
    objs = cloud()
    all_rays = mixed_rays(1000, seed=5)
    subsets = [c for r in range(1, 6) for c in itertools.combinations(GBUFFER_FIELDS, r)]
    assert len(subsets) == 31
    hits_seen = 0
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        rays = all_rays[:n]
        with hip(objs, lights(), rays, DEPTH, raygen=False) as rt:
            g = rt.render_gbuffer()
            assert_gbuffer(g, rt.query_hits(rays), f"n = {n}")
            assert_gbuffer(g, rt.pick_hit(np.arange(n, dtype=np.uint64)), f"n = {n}: pick_hit")
            assert_albedo(rt, g, f"n = {n}")
            assert_zero_where_missed(g, f"n = {n}")
            assert rt.gbuffer_info()["n_items"] == n and rt.gbuffer_info()["hits"] == int((g["index"] >= 0).sum())
            hits_seen += int((g["index"] >= 0).sum())
            # the device form into buffers of n + 1 elements: the guard element stays; every selection of outputs on one size
            for chosen in (subsets if n == 257 else [GBUFFER_FIELDS]):
                out = guarded(n)
                gb = RTGBuffer(**{k: out[k].data_ptr() for k in chosen})
                assert rt._lib.rt_render_gbuffer_device(rt._ctx, ctypes.byref(gb), None) == 0, (n, chosen)
                torch.cuda.synchronize()
                for k, tensor in out.items():
                    a = tensor.cpu().numpy()
                    if k in chosen:
                        assert np.array_equal(a[:n], g[k]) if k == "index" else same_bits_or_nan(a[:n], g[k]), (n, chosen, k)
                        assert (a[n:] == GUARD[k]).all(), (n, chosen, k, "guard")
                    else:
                        assert (a == GUARD[k]).all(), (n, chosen, k, "not asked for")
            only = rt.render_gbuffer(want=("normal",))
            assert list(only) == ["normal"] and same_bits_or_nan(only["normal"], g["normal"])
        assert_query((g["t"], g["index"]), fresh_aux(objs, rays), f"n = {n}: fresh hittest context")
    assert hits_seen > 500


# ---- 3. frame shapes --------------------------------------------------------------------------------------------------------------
def test_a_width_that_is_no_multiple_of_8():
    objs = cloud()
    w, h = 60, 44
    with hip(objs, lights(), None, DEPTH, camera=(w, h, Z)) as rt:
        g = rt.render_gbuffer()
        assert_gbuffer(g, rt.pick_hit(np.arange(w * h, dtype=np.uint64)), "60 x 44")
        assert_albedo(rt, g, "60 x 44")
    assert (g["index"] >= 0).sum() > 300


@pytest.mark.parametrize("tile_rays", [8 * W, 100], ids=["row tiles", "tiles of 100 rays"])
def test_every_rank_of_three_delivers_its_part_of_the_unsharded_pass(tile_rays):
    objs = cloud()
    n = W * H
    padding_seen = 0
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        whole = rt.render_gbuffer()
        for rank in range(3):
            rt.set_shard(tile_rays, rank, 3)
            part = rt.render_gbuffer()
            g = global_items(n, tile_rays, rank, 3, rt.local_rays)
            real = g < n
            assert len(part["t"]) == rt.local_rays and real.sum() > 0
            for k in GBUFFER_FIELDS:
                a, b = part[k][real], whole[k][g[real]]
                assert np.array_equal(a, b) if k == "index" else same_bits_or_nan(a, b), (rank, k)
            # a ragged last tile: its padding reads as a miss
            pad = ~real
            padding_seen += int(pad.sum())
            assert (part["t"][pad] == MAX_FLOAT).all() and (part["index"][pad] == -1).all()
            for k in ("point", "normal", "albedo"):
                assert not bits(part[k][pad]).any(), (rank, k)
            assert rt.gbuffer_info()["n_items"] == rt.local_rays
        rt.set_shard(n, 0, 1)
        assert_gbuffer(rt.render_gbuffer(), whole, "unsharded again", keys=GBUFFER_FIELDS)
    assert (padding_seen > 0) == (n % tile_rays != 0)


# ---- 4. poses ---------------------------------------------------------------------------------------------------------------------
def test_a_pose_inside_and_a_pose_outside_the_box():
    """The frame is 128 x 64 - sixteen screen tiles, the smallest frame of a scene of fewer than 512 objects whose pose outside the box is
    served by its tiles (rt_camera_tiles.cpp) - and the query it is compared with takes brute force out there, so it gets 64 x 16 of the
    frame's rays, spread over the whole frame."""
    import torch
    objs = cloud()
    lo, hi = cloud_box()
    centre, diag = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
    pw, ph = 128, 64
    inside = (centre + np.array([0.3, -0.2, 2.0])).astype(F)
    outside = centre + np.array([0.0, 0.05, 0.04]) * diag
    outside[0] = hi[0] + diag                                 # one box diagonal outside the x.hi face
    outside = outside.astype(F)
    z_out = float(F(-0.5 * pw * np.linalg.norm(outside - centre) / (0.5 * diag)))
    poses = [("inside", -80.0, camera.look_at(inside, centre + np.array([0.0, 0.0, -3.0])), inside),
             ("outside", z_out, camera.look_at(outside, centre), outside)]
    picked = np.sort(np.random.default_rng(3).choice(pw * ph, size=64 * 16, replace=False))
    with hip(objs, lights(), None, DEPTH, camera=(pw, ph, Z)) as rt:
        for label, z, M, o in poses:
            rt.set_pose(pw, ph, z, M, o)
            g = rt.render_gbuffer()
            if label == "outside":
                ti, ri = rt.tiles_info(), rt.rays_info()
                assert ti["source"] == 3 and ri["primary_outside_box"] == 1, (ti, {k: v for k, v in ri.items() if not hasattr(v, "shape")})
            rays = rt.generate_rays(pw, ph, z, M, o)[torch.from_numpy(picked).cuda()].contiguous()
            want = {k: v.cpu().numpy() for k, v in rt.query_hits(rays, want=("t", "index", "point", "normal")).items()}
            assert_gbuffer({k: v[picked] for k, v in g.items()}, want, label)
            assert_albedo(rt, g, label)
            assert (g["index"] >= 0).sum() > 400 and (g["index"] < 0).sum() > 100, label
            if label == "outside":
                assert rt.query_info()["n_brute"] == len(picked)      # the query took brute force; the pass its screen tiles


# ---- 5. live state ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_pass_follows_the_setters(size):
    objs = cloud() if size == "large" else small()
    moves = three_moves(objs)
    mask = random_mask(len(objs), seed=33)
    mask[moves[0][0]] = 1
    hidden = np.nonzero(mask == 0)[0]
    items = np.arange(W * H, dtype=np.uint64)
    rays = pinhole_rays(W, H, Z)
    now = objs.copy()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        first = rt.render_gbuffer()
        for i, t in moves:
            rt.set_transforms(t, i)
            now = R.with_transforms(now, t, i)
        moved = rt.render_gbuffer()
        assert_gbuffer(moved, rt.pick_hit(items), f"{size}: moved")
        assert_query((moved["t"], moved["index"]), fresh_aux(now, rays), f"{size}: moved, fresh hittest context")
        assert (moved["index"] == moves[0][0]).any() and not np.array_equal(moved["index"], first["index"])
        rt.set_visibility(mask)
        now = R.with_visibility(now, mask)
        masked = rt.render_gbuffer()
        assert_gbuffer(masked, rt.pick_hit(items), f"{size}: moved and masked")
        assert_query((masked["t"], masked["index"]), fresh_aux(now, rays), f"{size}: masked, fresh hittest context")
        assert not np.isin(masked["index"][masked["index"] >= 0], hidden).any()
        assert not np.array_equal(masked["index"], moved["index"])
        mats = new_materials(len(objs), seed=35)
        rt.set_materials(mats)
        coloured = rt.render_gbuffer()
        assert_gbuffer(coloured, masked, f"{size}: new materials move nothing")
        assert_albedo(rt, coloured, f"{size}: new materials")
        hit = coloured["index"] >= 0
        assert same_bits_or_nan(coloured["albedo"][hit, :3], mats["diffuse"][coloured["index"][hit]][:, :3])
        assert not same_bits_or_nan(coloured["albedo"], masked["albedo"])
        assert_zero_where_missed(coloured, size)


# ---- 6. the frame is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_frame_is_untouched(size):
    import torch
    objs = cloud() if size == "large" else small()
    n = W * H
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        aux = rt.render_aux()
        g = rt.render_gbuffer()
        assert_same(snapshot(rt), before, "a render before and after a pass")
        # a pending aux pair still receives the NEXT render's values
        d_t = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        d_i = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        assert rt._lib.rt_set_aux_device(rt._ctx, VP(d_t.data_ptr()), VP(d_i.data_ptr())) == 0
        again = rt.render_gbuffer()
        torch.cuda.synchronize()
        assert (d_t.cpu().numpy() == -1.0).all() and (d_i.cpu().numpy() == -5).all()       # the pass did not consume the pair
        rt.render_device(frame.data_ptr())
        torch.cuda.synchronize()
        assert_query((d_t.cpu().numpy(), d_i.cpu().numpy()), aux, "the aux pair after the pass")
        assert np.array_equal(bits(frame.cpu().numpy()), bits(before["frame"]))
        assert_gbuffer(again, g, "a second pass", keys=GBUFFER_FIELDS)
        # stats and the timing summary keep describing renders
        rt.timing_reset()
        rt.Render()
        st, summary = rt.stats(), rt.timing_summary()
        rt.render_gbuffer()
        st2, summary2 = rt.stats(), rt.timing_summary()
        for field, _ in st._fields_:
            assert getattr(st, field) == getattr(st2, field), field
        assert summary == summary2 and summary[1] == 1


def test_supersampling_delivers_samples_and_leaves_the_pixels():
    objs = cloud()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), supersample=2) as rt:
        assert rt.local_rays == 4 * W * H and rt.local_pixels == W * H
        before = rt.Render()
        g = rt.render_gbuffer()
        assert all(len(g[k]) == 4 * W * H for k in GBUFFER_FIELDS)
        want = rt.pick_hit(np.arange(4 * W * H, dtype=np.uint64))
        assert_gbuffer(g, want, "samples")
        assert_albedo(rt, g, "samples")
        after = rt.Render()
        assert after.shape == before.shape and len(after) == W * H and np.array_equal(bits(after), bits(before))
    assert (g["index"] >= 0).sum() > 1200


# ---- 7. triangles -----------------------------------------------------------------------------------------------------------------
def test_triangles(restatement):
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    rays = pinhole_rays(W, H, z)
    oracle = restatement[True].render("hittest", objs, lts, rays, 0)
    with hip(objs, lts, rays, 0, kernel="hittest", raygen=False) as fresh:
        fresh_pair = fresh.render_aux()
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        d = rt.render_gbuffer()
        assert_albedo(rt, d, "tri")
        with pytest.raises(RTError):
            rt.query_hits(rays)                              # the queries' refusal stays
    with hip(objs, lts, None, DEPTH, camera=(W, H, z), fused=False) as rt:
        u = rt.render_gbuffer()
    with hip(objs, lts, rays, 0, kernel="hittest", raygen=False, fused=False) as fresh:
        fresh_unfused = fresh.render_aux()
    assert_query((d["t"], d["index"]), fresh_pair, "tri: fresh hittest context")
    assert_query((u["t"], u["index"]), fresh_unfused, "tri, unfused: fresh hittest context")
    assert np.array_equal(d["index"], oracle["hit_index"]) and np.array_equal(bits(d["t"]), bits(oracle["hit_t"].astype(F)))
    hit = d["index"] >= 0
    assert hit.sum() > 300 and (objs["type"][d["index"][hit]] == TRIANGLE).all()
    want_u = HT.hit_records(objs, rays, u["t"], u["index"])
    assert_gbuffer(u, want_u, "tri, unfused", keys=RECORDS)
    want_d = HT.hit_records(objs, rays, d["t"], d["index"], fused=True)
    assert_gbuffer(d, want_d, "tri, default: the single-rounded point", keys=("point",))
    assert_gbuffer(d, HT.hit_records(objs, rays, d["t"], d["index"]), "tri, default: the normal contracts nothing", keys=("normal",))
    assert_zero_where_missed(d, "tri")
    assert_zero_where_missed(u, "tri, unfused")


# ---- 8. contexts and streams ------------------------------------------------------------------------------------------------------
def test_a_hittest_context():
    objs = cloud()
    with hip(objs, lights(), None, 0, camera=(W, H, Z), kernel="hittest") as rt:
        aux = rt.render_aux()
        frame = rt.Render()
        g = rt.render_gbuffer()
        assert_query((g["t"], g["index"]), aux, "hittest: render_aux plus records")
        assert_gbuffer(g, rt.pick_hit(np.arange(W * H, dtype=np.uint64)), "hittest")
        assert_albedo(rt, g, "hittest")
        assert np.array_equal(bits(rt.Render()), bits(frame))


def test_torch_out_on_a_side_stream_behind_a_torch_kernel():
    import torch
    objs = cloud()
    n = W * H
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        want = rt.render_gbuffer()
        work = torch.full((1024, 1024), 1.0 / 1024.0, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(4):
                work = work @ work
            out = {"t": torch.empty(n, dtype=torch.float32, device="cuda"), "index": torch.empty(n, dtype=torch.int32, device="cuda"),
                   "point": torch.empty((n, 4), dtype=torch.float32, device="cuda"), "normal": torch.empty((n, 4), dtype=torch.float32, device="cuda"),
                   "albedo": torch.empty((n, 4), dtype=torch.float32, device="cuda")}
            res = rt.render_gbuffer(out=out)
            assert all(res[k] is out[k] for k in GBUFFER_FIELDS)
            only = rt.render_gbuffer(want=("normal",), out={"normal": torch.empty((n, 4), dtype=torch.float32, device="cuda")})
        side.synchronize()
        assert_gbuffer({k: v.cpu().numpy() for k, v in res.items()}, want, "side stream", keys=GBUFFER_FIELDS)
        assert same_bits_or_nan(only["normal"].cpu().numpy(), want["normal"])
        with pytest.raises(ValueError):
            rt.render_gbuffer(out={"t": torch.empty(n - 1, dtype=torch.float32, device="cuda")}, want=("t",))
        with pytest.raises(ValueError):
            rt.render_gbuffer(want=("colour",))


def test_refusals_touch_nothing_and_an_empty_shard_is_ok():
    import torch
    from opencl_raytracer_amd.hip_raytracer import RTGBufferInfo, load_library
    objs = cloud()
    n = W * H
    out = guarded(n)
    host_t = np.full(n, 5.0, dtype=F)

    def dev(**offsets):
        gb = RTGBuffer(**{k: out[k].data_ptr() + offsets.get(k, 0) for k in GBUFFER_FIELDS})
        return lambda: rt._lib.rt_render_gbuffer_device(rt._ctx, ctypes.byref(gb), None)

    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        lib, ctx = rt._lib, rt._ctx
        info = RTGBufferInfo()
        assert lib.rt_get_gbuffer_info(ctx, ctypes.byref(info)) == -5            # RT_ERR_STATE before the first pass
        before = snapshot(rt)
        first = rt.render_gbuffer()
        said = rt.gbuffer_info()
        refused = [dev(point=4), dev(point=8), dev(normal=4), dev(albedo=8), dev(t=2), dev(index=1),
                   lambda: lib.rt_render_gbuffer_device(ctx, ctypes.byref(RTGBuffer()), None),
                   lambda: lib.rt_render_gbuffer_device(ctx, None, None),
                   lambda: lib.rt_render_gbuffer(ctx, ctypes.byref(RTGBuffer())),
                   lambda: lib.rt_render_gbuffer(ctx, None)]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        torch.cuda.synchronize()
        for k, tensor in out.items():
            assert (tensor.cpu().numpy() == GUARD[k]).all(), k
        counts = rt.gbuffer_info()
        assert (counts["n_items"], counts["hits"]) == (said["n_items"], said["hits"])     # the last pass is still the last pass
        # an empty shard: RT_OK, nothing launched, nothing written
        rt.set_shard(n, 1, 2)                               # one tile: rank 1 of 2 owns nothing
        assert rt.local_rays == 0
        assert lib.rt_render_gbuffer_device(ctx, ctypes.byref(RTGBuffer(t=out["t"].data_ptr())), None) == 0
        assert lib.rt_render_gbuffer(ctx, ctypes.byref(RTGBuffer(t=host_t.ctypes.data))) == 0
        assert all(len(v) == 0 for v in rt.render_gbuffer().values())
        torch.cuda.synchronize()
        assert (out["t"].cpu().numpy() == GUARD["t"]).all() and (host_t == 5.0).all()
        rt.set_shard(n, 0, 1)
        assert_same(snapshot(rt), before, "the frame after the refusals")
        assert_gbuffer(rt.render_gbuffer(), first, "after the refusals", keys=GBUFFER_FIELDS)
    # no rays yet: RT_ERR_STATE, nothing touched
    lib = load_library()
    o, lts = np.ascontiguousarray(objs), np.ascontiguousarray(lights())
    ctx = VP()
    assert lib.rt_create(ctypes.byref(ctx), o.ctypes.data_as(VP), len(o), lts.ctypes.data_as(VP), len(lts), None, n, 0, 0, 0, 0) == 0
    try:
        assert lib.rt_render_gbuffer(ctx, ctypes.byref(RTGBuffer(t=host_t.ctypes.data))) == -5
        assert lib.rt_last_error(ctx) and (host_t == 5.0).all()
    finally:
        lib.rt_destroy(ctx)
