"""GPU: ambient-occlusion frames (hip_raytracer.h, "ambient-occlusion frames") - rt_ao_device, rt_ao, rt_render_ao_device, rt_render_ao,
rt_get_ao_info.

1. the contract: render_ao's counts equal K - sum query_occluded(ao.rays(render_gbuffer())) on the same context and ao has the bits of
   count / K, for every K, in every arithmetic mode, on the grid scene and the no-grid scene; in the default arithmetic also
   CPURaytracer.render_ao; ao_info against the definition's live items and rays.query_route;
2. launch boundaries of the pass alone: 1 .. 1000 items x K = 1, 8, 64 from hit records with misses and non-finite entries, the guard
   element, every selection of outputs, index = None;
3. shapes: world = 3 with tiles that are no whole rows and a ragged last tile; supersampling 2;
4. live state; 5. the frame is untouched; 6. torch outputs on a side stream; 7. a hittest context, refusals, triangles, an empty shard.
(The file's name sorts behind test_bench_launcher.py, whose launcher test needs a process that has not initialised the GPU yet.)
Scenes are test_set_materials_gpu.py's: 64 x 48 frames of the 200-object cloud (a grid) and its first 40 objects (none)."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import R
from opencl_raytracer_amd import ao as AO
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from opencl_raytracer_amd.hip_raytracer import AO_FIELDS, RTAO, RTAOInfo, RTAOParams, RTError
from test_frame_shapes_cpu import camera_z_for, pinhole_rays, scene
from test_gbuffer_gpu import global_items
from test_primary_depth_order_gpu import bits, hip
from test_query_gpu import MODES, assert_query, mixed_rays
from test_set_materials_cpu import new_materials
from test_set_materials_gpu import DEPTH, H, W, Z, assert_same, cloud, lights, small, snapshot
from test_set_transforms_gpu import three_moves
from test_set_visibility_gpu import random_mask

pytestmark = pytest.mark.gpu
F = np.float32
VP = ctypes.c_void_p
BIAS = 1e-3
KS = (1, 2, 4, 8, 16, 32, 64)
BOTH = ("unoccluded", "ao")


def table(K, radius=None, n_sets=16):
    """radius 1 and 4 in turn: short rays that mostly end free, long ones that mostly do not"""
    return AO.directions(K, n_sets, radius or (1.0 if K in (1, 4, 16, 64) else 4.0), seed=100 + K)


def defined(rt, g, dirs, K, bias=BIAS, items=None, index=True):
    """(unoccluded, ao, live, rays) of the definition on this context: ao.rays -> query_occluded -> ao.reduce"""
    rays, live = AO.rays(g["point"], g["normal"], g["index"] if index else None, dirs, K, bias, items)
    unoccluded, ao = AO.reduce(rt.query_occluded(rays), live, K)
    return unoccluded, ao, live, rays


def assert_ao(got, unoccluded, ao, label):
    assert got["unoccluded"].dtype == np.uint8 and got["ao"].dtype == F, label
    bad = int((got["unoccluded"] != unoccluded).sum())
    assert got["unoccluded"].shape == unoccluded.shape and bad == 0, f"{label}: {bad} counts differ"
    assert np.array_equal(bits(got["ao"]), bits(ao)), f"{label}: ao"


# ---- 1. the contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
@pytest.mark.parametrize("mode", list(MODES))
def test_counts_equal_the_occlusion_queries_of_the_definitions_rays(mode, size):
    objs = cloud() if size == "large" else small()
    cpu = CPURaytracer(objs, lights(), pinhole_rays(W, H, Z), 0, kernel="hittest") if mode == "default" else None
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), **MODES[mode]) as rt:
        g = rt.render_gbuffer()
        info = rt.rays_info()
        box = (info["box_lo"], info["box_hi"]) if info["grid_built"] else (None, None)
        assert bool(info["grid_built"]) == (size == "large")
        for K in KS:
            label = f"{mode} {size} K = {K}"
            dirs = table(K)
            got = rt.render_ao(dirs, K, BIAS, want=BOTH)
            said = rt.ao_info()
            unoccluded, ao, live, rays = defined(rt, g, dirs, K)
            assert_ao(got, unoccluded, ao, label)
            assert np.array_equal(bits(got["ao"]), bits(got["unoccluded"].astype(F) / F(K))), label
            traced = R.rays_of(rays)[np.repeat(live, K)]
            on_grid = int(RY.query_route(traced, *box).sum())
            assert (said["n_items"], said["n_live"], said["n_rays"]) == (W * H, int(live.sum()), K * int(live.sum())), (label, said)
            assert (said["n_grid"], said["n_brute"]) == (on_grid, len(traced) - on_grid), (label, said)
            assert said["ao_ms"] > 0 and said["gbuffer_ms"] > 0 and said["object_tests"] > 0, (label, said)
            assert (got["unoccluded"][~live] == K).all() and (got["ao"][~live] == 1.0).all(), label
            seen = set(got["unoccluded"][live].tolist())
            assert len(seen) >= min(K + 1, 5) and max(seen) == K, (label, sorted(seen))          # a test with signal
            if cpu is not None:
                want = cpu.render_ao(dirs, K, BIAS)
                assert_ao(got, want["unoccluded"], want["ao"], f"{label}: CPURaytracer")
            if size == "large":
                assert said["n_grid"] > 0.9 * said["n_rays"], (label, said)
        assert int(live.sum()) == (2528 if size == "large" else 1208)
        only = rt.render_ao(table(8), 8, BIAS)
        assert list(only) == ["ao"]


# ---- 2. launch boundaries of the pass alone ----------------------------------------------------------------------------------------
GUARD = {"unoccluded": 200, "ao": -7.25}


def guarded(n):
    import torch
    return {"unoccluded": torch.full((n + 1,), GUARD["unoccluded"], dtype=torch.uint8, device="cuda"),
            "ao": torch.full((n + 1,), GUARD["ao"], dtype=torch.float32, device="cuda")}


def test_launch_boundaries_of_the_pass_alone():
    import torch
    objs = cloud()
    all_rays = mixed_rays(1000, seed=5)
    selections = [c for r in (1, 2) for c in itertools.combinations(AO_FIELDS, r)]
    assert len(selections) == 3
    dead_seen = live_seen = 0
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        hits = rt.query_hits(all_rays)
        hits["point"][7, 1] = np.inf               # non-finite records among them: dead whatever the index says
        hits["normal"][11, 2] = np.nan
        assert (hits["index"] < 0).sum() > 100 and (hits["index"] >= 0).sum() > 100
        d_point, d_normal = torch.from_numpy(hits["point"]).cuda(), torch.from_numpy(hits["normal"]).cuda()
        d_index = torch.from_numpy(hits["index"]).cuda()
        for n, K in itertools.product((1, 63, 64, 65, 255, 256, 257, 1000), (1, 8, 64)):
            g = {k: hits[k][:n] for k in ("point", "normal", "index")}
            dirs = table(K, n_sets=5)
            d_dirs = torch.from_numpy(dirs).cuda()
            params = RTAOParams(K, 5, BIAS, 0, d_dirs.data_ptr())
            for with_index in (True, False):
                unoccluded, ao, live, _ = defined(rt, g, dirs, K, index=with_index)
                want = {"unoccluded": unoccluded, "ao": ao}
                dead_seen += int((~live).sum())
                live_seen += int(live.sum())
                host = rt.ao_pass(g["point"], g["normal"], g["index"] if with_index else None, dirs, K, BIAS, want=BOTH)
                assert_ao(host, unoccluded, ao, f"n = {n}, K = {K}, index {with_index}: host twin")
                said = rt.ao_info()
                assert (said["n_items"], said["n_live"], said["n_rays"], said["gbuffer_ms"]) == (n, int(live.sum()), K * int(live.sum()), 0.0)
                assert said["n_grid"] + said["n_brute"] == said["n_rays"]
                # the device form into buffers of n + 1 elements: the guard element stays; every selection of the outputs
                for chosen in (selections if with_index else [BOTH]):
                    out = guarded(n)
                    o = RTAO(**{k: out[k].data_ptr() for k in chosen})
                    rc = rt._lib.rt_ao_device(rt._ctx, VP(d_point.data_ptr()), VP(d_normal.data_ptr()), VP(d_index.data_ptr()) if with_index else None,
                                              n, ctypes.byref(params), ctypes.byref(o), None)
                    assert rc == 0, (n, K, chosen, rt._lib.rt_last_error(rt._ctx))
                    torch.cuda.synchronize()
                    for k, tensor in out.items():
                        a = tensor.cpu().numpy()
                        if k in chosen:
                            assert np.array_equal(bits(a[:n]), bits(want[k])), (n, K, chosen, k)
                            assert (a[n:] == F(GUARD[k])).all(), (n, K, chosen, k, "guard")
                        else:
                            assert (a == F(GUARD[k])).all(), (n, K, chosen, k, "not asked for")
    assert dead_seen > 1000 and live_seen > 1000


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------------
def test_every_rank_of_three_delivers_its_part_of_the_unsharded_frame():
    objs = cloud()
    n, tile_rays, K = W * H, 100, 8             # tiles that are no whole rows; 3072 = 30 * 100 + 72: a ragged last tile
    dirs = table(K, n_sets=64)
    padding_seen = 0
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        whole = rt.render_ao(dirs, K, BIAS, want=BOTH)
        assert len(set(AO.item_sets(np.arange(n), 64).tolist())) > 32           # the sets really differ from item to item
        for rank in range(3):
            rt.set_shard(tile_rays, rank, 3)
            part = rt.render_ao(dirs, K, BIAS, want=BOTH)
            g = global_items(n, tile_rays, rank, 3, rt.local_rays)
            real = g < n
            assert len(part["ao"]) == rt.local_rays and real.sum() > 0
            for k in BOTH:
                assert np.array_equal(bits(part[k][real]), bits(whole[k][g[real]])), (rank, k)
                assert (part[k][~real] == (K if k == "unoccluded" else 1.0)).all(), (rank, k, "padding is dead")
            padding_seen += int((~real).sum())
            assert rt.ao_info()["n_items"] == rt.local_rays
        rt.set_shard(n, 0, 1)
        again = rt.render_ao(dirs, K, BIAS, want=BOTH)
        assert_ao(again, whole["unoccluded"], whole["ao"], "unsharded again")
    assert padding_seen == 28 and (whole["unoccluded"] < K).sum() > 300


def test_supersampling_delivers_samples_and_leaves_the_pixels():
    objs = cloud()
    K = 4
    dirs = table(K)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), supersample=2) as rt:
        assert rt.local_rays == 4 * W * H
        before = rt.Render()
        got = rt.render_ao(dirs, K, BIAS, want=BOTH)
        unoccluded, ao, live, _ = defined(rt, rt.render_gbuffer(), dirs, K)
        assert len(got["ao"]) == 4 * W * H and live.sum() > 8000
        assert_ao(got, unoccluded, ao, "samples")
        after = rt.Render()
        assert len(after) == W * H and np.array_equal(bits(after), bits(before))


# ---- 4. live state --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_pass_follows_the_setters(size):
    objs = cloud() if size == "large" else small()
    moves = three_moves(objs)
    mask = random_mask(len(objs), seed=33)
    mask[moves[0][0]] = 1
    K = 8
    dirs = table(K, radius=4.0)
    now = objs.copy()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        first = rt.render_ao(dirs, K, BIAS, want=BOTH)
        for i, t in moves:
            rt.set_transforms(t, i)
            now = R.with_transforms(now, t, i)
        rt.set_visibility(mask)
        now = R.with_visibility(now, mask)
        rt.set_materials(new_materials(len(objs), seed=35))
        live_state = rt.render_ao(dirs, K, BIAS, want=BOTH)
        unoccluded, ao, _, _ = defined(rt, rt.render_gbuffer(), dirs, K)
        assert_ao(live_state, unoccluded, ao, f"{size}: the definition on the live context")
    with hip(now, lights(), None, DEPTH, camera=(W, H, Z)) as fresh:
        want = fresh.render_ao(dirs, K, BIAS, want=BOTH)
    assert_ao(live_state, want["unoccluded"], want["ao"], f"{size}: a fresh context")
    assert not np.array_equal(live_state["unoccluded"], first["unoccluded"])


# ---- 5. the frame is untouched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_the_frame_is_untouched(size):
    import torch
    objs = cloud() if size == "large" else small()
    n, K = W * H, 8
    dirs = table(K)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        aux = rt.render_aux()
        first = rt.render_ao(dirs, K, BIAS, want=BOTH)
        assert_same(snapshot(rt), before, "a render before and after a pass")
        # a pending aux pair still receives the NEXT render's values
        d_t = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        d_i = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        assert rt._lib.rt_set_aux_device(rt._ctx, VP(d_t.data_ptr()), VP(d_i.data_ptr())) == 0
        again = rt.render_ao(dirs, K, BIAS, want=BOTH)
        torch.cuda.synchronize()
        assert (d_t.cpu().numpy() == -1.0).all() and (d_i.cpu().numpy() == -5).all()       # the pass did not consume the pair
        rt.render_device(frame.data_ptr())
        torch.cuda.synchronize()
        assert_query((d_t.cpu().numpy(), d_i.cpu().numpy()), aux, "the aux pair after the pass")
        assert np.array_equal(bits(frame.cpu().numpy()), bits(before["frame"]))
        assert_ao(again, first["unoccluded"], first["ao"], "a second pass")
        # stats and the timing summary keep describing renders; the G-buffer info describes the internal pass
        rt.timing_reset()
        rt.Render()
        st, summary = rt.stats(), rt.timing_summary()
        rt.render_ao(dirs, K, BIAS)
        st2, summary2 = rt.stats(), rt.timing_summary()
        for field, _ in st._fields_:
            assert getattr(st, field) == getattr(st2, field), field
        assert summary == summary2 and summary[1] == 1
        assert rt.gbuffer_info()["n_items"] == n and rt.gbuffer_info()["hits"] >= rt.ao_info()["n_live"] > 0


# ---- 6. torch outputs on a side stream ------------------------------------------------------------------------------------------------
def test_torch_out_on_a_side_stream_behind_a_torch_kernel():
    import torch
    objs = cloud()
    n, K = W * H, 16
    dirs = table(K)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        want = rt.render_ao(dirs, K, BIAS, want=BOTH)
        g = rt.render_gbuffer()
        work = torch.full((1024, 1024), 1.0 / 1024.0, device="cuda")
        d_dirs = torch.from_numpy(dirs).cuda()
        d_g = {k: torch.from_numpy(g[k]).cuda() for k in ("point", "normal", "index")}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(4):
                work = work @ work
            out = {"unoccluded": torch.empty(n, dtype=torch.uint8, device="cuda"), "ao": torch.empty(n, dtype=torch.float32, device="cuda")}
            res = rt.render_ao(d_dirs, K, BIAS, want=BOTH, out=out)
            assert all(res[k] is out[k] for k in BOTH)
            only = rt.render_ao(dirs, K, BIAS, out={"ao": torch.empty(n, dtype=torch.float32, device="cuda")})       # a host table: uploaded
            alone = rt.ao_pass(d_g["point"], d_g["normal"], d_g["index"], d_dirs, K, BIAS, want=BOTH)
        side.synchronize()
        assert_ao({k: v.cpu().numpy() for k, v in res.items()}, want["unoccluded"], want["ao"], "side stream")
        assert list(only) == ["ao"] and np.array_equal(bits(only["ao"].cpu().numpy()), bits(want["ao"]))
        assert_ao({k: v.cpu().numpy() for k, v in alone.items()}, want["unoccluded"], want["ao"], "the pass alone, device tensors")
        with pytest.raises(ValueError):
            rt.render_ao(dirs, K, BIAS, out={"ao": torch.empty(n - 1, dtype=torch.float32, device="cuda")})
        with pytest.raises(ValueError):
            rt.render_ao(dirs, K, BIAS, want=("colour",))
        with pytest.raises(ValueError):
            rt.render_ao(dirs, 3, BIAS)


# ---- 7. acceptance and refusals -------------------------------------------------------------------------------------------------------
def test_a_hittest_context_is_accepted():
    objs = cloud()
    K = 8
    dirs = table(K)
    with hip(objs, lights(), None, 0, camera=(W, H, Z), kernel="hittest") as rt:
        frame = rt.Render()
        got = rt.render_ao(dirs, K, BIAS, want=BOTH)
        unoccluded, ao, live, _ = defined(rt, rt.render_gbuffer(), dirs, K)
        assert_ao(got, unoccluded, ao, "hittest")
        assert live.sum() > 2000 and np.array_equal(bits(rt.Render()), bits(frame))


def test_refusals_touch_nothing_and_an_empty_shard_is_ok():
    import torch
    from opencl_raytracer_amd.hip_raytracer import load_library
    objs = cloud()
    n, K = W * H, 8
    dirs = table(K)
    d_dirs = torch.from_numpy(dirs).cuda()
    out = guarded(n)
    host_ao = np.full(n, 5.0, dtype=F)
    point = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    inf, nan = float("inf"), float("nan")

    def P(samples=K, n_sets=16, bias=BIAS, reserved=0, dirs=d_dirs.data_ptr()):
        return RTAOParams(samples, n_sets, bias, reserved, dirs)

    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        lib, ctx = rt._lib, rt._ctx
        info = RTAOInfo()
        assert lib.rt_get_ao_info(ctx, ctypes.byref(info)) == -5                 # RT_ERR_STATE before the first pass
        before = snapshot(rt)
        first = rt.render_ao(dirs, K, BIAS, want=BOTH)
        said = rt.ao_info()
        both = RTAO(out["unoccluded"].data_ptr(), out["ao"].data_ptr())
        host_both = RTAO(None, host_ao.ctypes.data)
        bad_params = [P(samples=0), P(samples=3), P(samples=128), P(n_sets=0), P(n_sets=4097), P(bias=-1e-3), P(bias=inf), P(bias=nan),
                      P(reserved=1), P(dirs=None)]
        refused = [lambda p=p: lib.rt_render_ao_device(ctx, ctypes.byref(p), ctypes.byref(both), None) for p in bad_params]
        refused += [lambda p=p: lib.rt_render_ao(ctx, ctypes.byref(p), ctypes.byref(host_both)) for p in bad_params]
        refused += [lambda p=p: lib.rt_ao_device(ctx, VP(point.data_ptr()), VP(point.data_ptr()), None, n, ctypes.byref(p), ctypes.byref(both), None)
                    for p in bad_params]
        ok = P()
        refused += [
            lambda: lib.rt_render_ao_device(ctx, None, ctypes.byref(both), None),
            lambda: lib.rt_render_ao_device(ctx, ctypes.byref(ok), None, None),
            lambda: lib.rt_render_ao_device(ctx, ctypes.byref(ok), ctypes.byref(RTAO()), None),
            lambda: lib.rt_render_ao(ctx, ctypes.byref(ok), ctypes.byref(RTAO())),
            lambda: lib.rt_render_ao(ctx, None, ctypes.byref(host_both)),
            lambda: lib.rt_render_ao_device(ctx, ctypes.byref(P(dirs=d_dirs.data_ptr() + 4)), ctypes.byref(both), None),
            lambda: lib.rt_render_ao_device(ctx, ctypes.byref(ok), ctypes.byref(RTAO(None, out["ao"].data_ptr() + 2)), None),
            lambda: lib.rt_ao_device(ctx, None, VP(point.data_ptr()), None, n, ctypes.byref(ok), ctypes.byref(both), None),
            lambda: lib.rt_ao_device(ctx, VP(point.data_ptr()), None, None, n, ctypes.byref(ok), ctypes.byref(both), None),
            lambda: lib.rt_ao_device(ctx, VP(point.data_ptr() + 8), VP(point.data_ptr()), None, n - 1, ctypes.byref(ok), ctypes.byref(both), None),
            lambda: lib.rt_ao_device(ctx, VP(point.data_ptr()), VP(point.data_ptr() + 4), None, n - 1, ctypes.byref(ok), ctypes.byref(both), None),
            lambda: lib.rt_ao_device(ctx, VP(point.data_ptr()), VP(point.data_ptr()), VP(point.data_ptr() + 2), n, ctypes.byref(ok), ctypes.byref(both), None),
            lambda: lib.rt_ao(ctx, None, None, None, n, ctypes.byref(P(dirs=dirs.ctypes.data)), ctypes.byref(host_both)),
        ]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        torch.cuda.synchronize()
        for k, tensor in out.items():
            assert (tensor.cpu().numpy() == F(GUARD[k])).all(), k
        assert (host_ao == 5.0).all()
        now = rt.ao_info()
        assert all(now[k] == said[k] for k in ("n_items", "n_live", "n_rays", "n_grid", "n_brute"))     # the last pass is still the last pass
        # an unaligned byte output is fine; n == 0 is RT_OK with nothing launched
        odd = RTAO(out["unoccluded"].data_ptr() + 1, None)
        assert lib.rt_ao_device(ctx, None, None, None, 0, ctypes.byref(ok), ctypes.byref(odd), None) == 0
        # an empty shard: RT_OK, nothing launched, nothing written
        rt.set_shard(n, 1, 2)                               # one tile: rank 1 of 2 owns nothing
        assert rt.local_rays == 0
        assert lib.rt_render_ao_device(ctx, ctypes.byref(ok), ctypes.byref(both), None) == 0
        assert lib.rt_render_ao(ctx, ctypes.byref(P(dirs=dirs.ctypes.data)), ctypes.byref(host_both)) == 0
        assert all(len(v) == 0 for v in rt.render_ao(dirs, K, BIAS, want=BOTH).values())
        torch.cuda.synchronize()
        assert all((out[k].cpu().numpy() == F(GUARD[k])).all() for k in out) and (host_ao == 5.0).all()
        rt.set_shard(n, 0, 1)
        assert_same(snapshot(rt), before, "the frame after the refusals")
        again = rt.render_ao(dirs, K, BIAS, want=BOTH)
        assert_ao(again, first["unoccluded"], first["ao"], "after the refusals")
        # the byte output at an odd address
        rc = lib.rt_render_ao_device(ctx, ctypes.byref(ok), ctypes.byref(odd), None)
        torch.cuda.synchronize()
        a = out["unoccluded"].cpu().numpy()
        assert rc == 0 and a[0] == GUARD["unoccluded"] and np.array_equal(a[1:], first["unoccluded"])
        g = rt.render_gbuffer()
    # no primary rays yet: the frame form is RT_ERR_STATE, the pass alone works
    lib = load_library()
    o, lts = np.ascontiguousarray(objs), np.ascontiguousarray(lights())
    ctx = VP()
    assert lib.rt_create(ctypes.byref(ctx), o.ctypes.data_as(VP), len(o), lts.ctypes.data_as(VP), len(lts), None, n, 0, 0, 0, 0) == 0
    try:
        host_params = P(dirs=dirs.ctypes.data)
        assert lib.rt_render_ao(ctx, ctypes.byref(host_params), ctypes.byref(host_both)) == -5
        assert lib.rt_last_error(ctx) and (host_ao == 5.0).all()
        p, nr, ix = (np.ascontiguousarray(g[k]) for k in ("point", "normal", "index"))
        assert lib.rt_ao(ctx, p.ctypes.data_as(VP), nr.ctypes.data_as(VP), ix.ctypes.data_as(VP), n, ctypes.byref(host_params), ctypes.byref(host_both)) == 0
        assert np.array_equal(bits(host_ao), bits(first["ao"]))
    finally:
        lib.rt_destroy(ctx)


def test_a_triangle_context_is_refused():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    K = 4
    dirs = table(K)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = rt.Render()
        with pytest.raises(RTError) as e:
            rt.render_ao(dirs, K, BIAS)
        assert e.value.code == -5
        g = rt.render_gbuffer()
        with pytest.raises(RTError) as e:
            rt.ao_pass(g["point"], g["normal"], g["index"], dirs, K, BIAS)
        assert e.value.code == -5
        assert np.array_equal(bits(rt.Render()), bits(before))
