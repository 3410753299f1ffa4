"""GPU: filtered ambient occlusion (hip_raytracer.h, "filtered ambient occlusion") - rt_ao_filter_device, rt_ao_filter,
rt_render_ao_filtered_device, rt_render_ao_filtered, rt_get_ao_filter_info. Everything is compared bit for bit with ao.filter.

1. the pass alone: every radius on 1x1, 3x2, 65x5, 130x37 and 257x19 (one and two tile widths plus a remainder, rows below and above
   the halo) over fields that mix the CPU test's adversarial items with two planes and a sphere cap; index = None; every selection
   of outputs, written into slices of larger tensors whose guard elements stay; a side stream; info.accepted == taps.sum(); a
   device_opencl context and an unfused one give the same bits;
2. the frame form on multipleSpheres.txt at 96 x 64 (the small-scene kernel) and on a 600-object scene at 128 x 64 (the round
   machine): against ao.filter of the same context's render_ao and render_gbuffer, against CPURaytracer.render_ao_filtered, under
   supersampling, after set_pose / set_visibility / set_transforms; the frame and a pending aux pair are left alone;
3. every refusal, each leaving the next frame and the caller's outputs as they were.
(The file's name sorts behind test_bench_launcher.py, whose launcher test needs a process that has not initialised the GPU yet.)"""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import R, SCENES, random_scene, rotation
from opencl_raytracer_amd import ao as AO
from opencl_raytracer_amd import camera, scene_loader
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from opencl_raytracer_amd.hip_raytracer import AO_FILTER_FIELDS, RTAOFiltered, RTAOFilterInfo, RTAOFilterParams, RTAOParams, RTError
from test_ao_filter_cpu import MEMBERS, RADII, adversarial_field, random_field, same
from test_frame_shapes_cpu import camera_z_for, pinhole_rays, scene
from test_primary_depth_order_gpu import bits, hip
from test_query_gpu import assert_query
from test_set_materials_gpu import DEPTH, H, W, Z, assert_same, cloud, lights, snapshot
from test_set_visibility_gpu import random_mask

pytestmark = pytest.mark.gpu
F = np.float32
VP = ctypes.c_void_p
BIAS = 1e-3
SHAPES = ((1, 1), (3, 2), (65, 5), (130, 37), (257, 19))     # (width, rows)
GUARD = {"ao": -7.25, "grey": 77, "taps": 201}
OFFSET = {"ao": 3, "grey": 1, "taps": 5}                      # where the slices start: the byte arrays at odd addresses


def field(width, rows, K, seed):
    """adversarial_field plus a band of clean geometry - two planes meeting in a crease and a sphere cap - so that whole windows accept"""
    u, p, nr, ix = adversarial_field(width, rows, K, seed)
    n = width * rows
    col, row = np.arange(n) % width, np.arange(n) // width
    clean = (row % 16 < 11) & (col % 40 < 30)
    x, y = (0.05 * col).astype(F), (0.05 * row).astype(F)
    crease = col % 40 < 12
    cap = ~crease & (col % 40 < 24)
    cz = np.sqrt(np.maximum(16.0 - (x - 1.0) ** 2 - (y - 0.5) ** 2, 1.0))
    capn = np.stack([x - 1.0, y - 0.5, cz], axis=1) / 4.0
    pz = np.where(crease, -10.0 - 0.75 * x, np.where(cap, -14.0 + cz, -10.0))
    pn = np.where(crease[:, None], np.array([0.6, 0.0, 0.8]), np.where(cap[:, None], capn, np.array([0.0, 0.0, 1.0])))
    p[clean, 0], p[clean, 1], p[clean, 2] = x[clean], y[clean], pz[clean].astype(F)
    nr[clean, :3] = pn[clean].astype(F)
    ix[clean] = 1
    return u, p, nr, ix


def guarded(n):
    import torch
    big = {"ao": torch.full((n + 8,), GUARD["ao"], dtype=torch.float32, device="cuda"),
           "grey": torch.full((n + 8,), GUARD["grey"], dtype=torch.uint8, device="cuda"),
           "taps": torch.full((n + 8,), GUARD["taps"], dtype=torch.uint8, device="cuda")}
    return big, {k: v[OFFSET[k]:OFFSET[k] + n] for k, v in big.items()}


def guards_stand(big, n, written=()):
    for k, v in big.items():
        a = v.cpu().numpy()
        inside = slice(OFFSET[k], OFFSET[k] + n)
        keep = np.ones(len(a), bool)
        if k in written:
            keep[inside] = False
        assert (a[keep] == (F(GUARD[k]) if k == "ao" else GUARD[k])).all(), (k, "guard")


# ---- 1. the pass alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RADII)
def test_the_pass_alone_equals_the_definition(r):
    import torch
    selections = [c for k in (1, 2, 3) for c in itertools.combinations(AO_FILTER_FIELDS, k)]
    assert len(selections) == 7
    objs = cloud()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for k, (width, rows) in enumerate(SHAPES):
            n, K = width * rows, (4, 1, 16, 4, 64)[k]
            u, p, nr, ix = field(width, rows, K, seed=7 * r + k)
            for normal_min, plane_max in ((0.9, 0.05), (F(0.8), F(0.25))):
                label = f"r = {r}, {width} x {rows}, ({normal_min}, {plane_max})"
                want = AO.filter(u, p, nr, ix, width, K, r, normal_min, plane_max)
                got = rt.ao_filter(u, p, nr, ix, width, K, r, normal_min, plane_max, want=MEMBERS)          # the host twin
                same(got, want)
                said = rt.ao_filter_info()
                assert (said["n_items"], said["n_live"], said["accepted"]) == (n, int((want["taps"] > 0).sum()), int(want["taps"].sum())), (label, said)
                assert said["filter_ms"] > 0 and said["ao_ms"] == 0 and said["gbuffer_ms"] == 0, (label, said)
                same(rt.ao_filter(u, p, nr, None, width, K, r, normal_min, plane_max, want=MEMBERS),
                     AO.filter(u, p, nr, None, width, K, r, normal_min, plane_max))                          # index = None
            if n >= 100:
                assert want["taps"].max() == (2 * r + 1) * min(rows, 2 * r + 1) and (want["taps"] == 0).any(), label   # whole windows accept somewhere
            # device tensors: every selection of outputs into slices of larger tensors
            d_u, d_p, d_n, d_i = (torch.from_numpy(a).cuda() for a in (u, p, nr, ix))
            for chosen in (selections if (width, rows) in ((3, 2), (130, 37)) else selections[-1:]):
                big, out = guarded(n)
                res = rt.ao_filter(d_u, d_p, d_n, d_i, width, K, r, normal_min, plane_max, want=chosen, out={c: out[c] for c in chosen})
                torch.cuda.synchronize()
                assert list(res) == list(chosen) and all(res[c] is out[c] for c in chosen)
                same({c: res[c].cpu().numpy() for c in chosen}, want, chosen)
                guards_stand(big, n, chosen)
            res = rt.ao_filter(d_u, d_p, d_n, None, width, K, r, normal_min, plane_max, want=MEMBERS)              # index = None on the device
            same({c: v.cpu().numpy() for c, v in res.items()}, AO.filter(u, p, nr, None, width, K, r, normal_min, plane_max))
        assert rt.ao_filter_info()["n_items"] == 257 * 19


def test_the_pass_alone_on_a_side_stream_and_in_every_arithmetic_mode():
    import torch
    width, rows, K, r = 130, 37, 4, 2
    u, p, nr, ix = field(width, rows, K, seed=99)
    want = AO.filter(u, p, nr, ix, width, K, r, 0.9, 0.05)
    objs = cloud()
    for mode in (dict(), dict(device_opencl=True), dict(fused=False)):
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), **mode) as rt:
            d_u, d_p, d_n, d_i = (torch.from_numpy(a).cuda() for a in (u, p, nr, ix))
            work = torch.full((512, 512), 1.0 / 512.0, device="cuda")
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(4):
                    work = work @ work
                res = rt.ao_filter(d_u, d_p, d_n, d_i, width, K, r, 0.9, plane_max=0.05, want=MEMBERS)
            side.synchronize()
            same({k: v.cpu().numpy() for k, v in res.items()}, want)
            assert rt.ao_filter_info()["accepted"] == int(want["taps"].sum()), mode
            with pytest.raises(TypeError):
                rt.ao_filter(u, p, nr, ix, width, K)                                   # plane_max has no default
            with pytest.raises(ValueError):
                rt.ao_filter(u, p, nr, ix, width + 1, K, plane_max=0.05)
            with pytest.raises(ValueError):
                rt.ao_filter(u, p, nr, ix, width, K, 5, plane_max=0.05)
            with pytest.raises(ValueError):
                rt.ao_filter(u, p, nr, ix, width, K, plane_max=0.05, want=("colour",))


# ---- 2. the frame form ---------------------------------------------------------------------------------------------------------------------
FILTER = dict(radius=2, normal_min=0.9, plane_max=0.1)


def table(K):
    return AO.directions(K, 16, 2.0, seed=100 + K)


def frame_scene(name):
    if name == "small":
        objs, lts = scene_loader.load_scene(str(SCENES / "multipleSpheres.txt"))
        return objs, lts, 96, 64, float(-64.0)
    objs, lts = random_scene(600, 100, 2, seed=21, spread=8.0, zrange=(-40.0, -10.0))
    return objs, lts, 128, 64, float(camera.camera_z(64))


def nudged(objs, i, delta):
    """(i, TRANSFORM_DTYPE[1]): object i translated by `delta`, its rotation and scale kept"""
    mv = objs["mv"][i].reshape(4, 4).T.astype(np.float64)
    mv[:3, 3] += delta
    t = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
    t["mv"][0], t["mvInverse"][0] = mv.T.astype(F).reshape(16), np.linalg.inv(mv).T.astype(F).reshape(16)
    return i, t


def defined(rt, width, K, dirs):
    """ao.filter of the same context's render_ao and render_gbuffer"""
    g = rt.render_gbuffer()
    a = rt.render_ao(dirs, K, BIAS, want=("unoccluded",))
    return AO.filter(a["unoccluded"], g["point"], g["normal"], g["index"], width, K, **FILTER)


@pytest.mark.parametrize("name", ["small", "large"])
def test_the_frame_form_equals_the_definition_and_the_cpu_backend(name):
    import torch
    objs, lts, w, h, z = frame_scene(name)
    K, n = 4, w * h
    dirs = table(K)
    cpu = CPURaytracer(objs, lts, pinhole_rays(w, h, z), 0, kernel="hittest")
    with hip(objs, lts, None, DEPTH, camera=(w, h, z)) as rt:
        before = snapshot(rt)
        assert rt.stats().wavefront == int(name == "large")
        aux = rt.render_aux()
        got = rt.render_ao_filtered(dirs, K, BIAS, want=MEMBERS, **FILTER)
        said = rt.ao_filter_info()
        same(got, defined(rt, w, K, dirs))
        same(got, cpu.render_ao_filtered(dirs, K, BIAS, width=w, **FILTER))
        assert (said["n_items"], said["accepted"]) == (n, int(got["taps"].sum())) and said["n_live"] == int((got["taps"] > 0).sum())
        assert said["filter_ms"] > 0 and said["ao_ms"] > 0 and said["gbuffer_ms"] > 0
        assert (got["taps"] > 4).sum() > 500 and (got["taps"] == 0).sum() > 100 and len(set(got["grey"].tolist())) > 8        # a test with signal
        assert rt.ao_info()["n_items"] == n and rt.gbuffer_info()["n_items"] == n
        # a later AO pass of another K re-records the AO family's events, not this pass's: its info stays what it was
        rt.render_ao(table(16), 16, BIAS)
        later = rt.ao_filter_info()      # (the same events read again: the conversion to ms wobbles in the sixth digit; another pass's pair would not)
        assert all(later[k] == said[k] for k in ("n_items", "n_live", "accepted")) and rt.ao_info()["n_rays"] == 16 * rt.ao_info()["n_live"]
        assert all(abs(later[k] - said[k]) < 1e-3 for k in ("gbuffer_ms", "ao_ms", "filter_ms")), (later, said)
        assert_same(snapshot(rt), before, "a render before and after a filtered pass")
        # a pending aux pair still receives the NEXT render's values; torch outputs on the current stream
        d_t = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        d_i = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        assert rt._lib.rt_set_aux_device(rt._ctx, VP(d_t.data_ptr()), VP(d_i.data_ptr())) == 0
        big, out = guarded(n)
        res = rt.render_ao_filtered(torch.from_numpy(dirs).cuda(), K, BIAS, want=MEMBERS, out=out, **FILTER)
        torch.cuda.synchronize()
        same({k: v.cpu().numpy() for k, v in res.items()}, got)
        guards_stand(big, n, MEMBERS)
        assert (d_t.cpu().numpy() == -1.0).all() and (d_i.cpu().numpy() == -5).all()
        rt.render_device(frame.data_ptr())
        torch.cuda.synchronize()
        assert_query((d_t.cpu().numpy(), d_i.cpu().numpy()), aux, "the aux pair after the pass")
        assert np.array_equal(bits(frame.cpu().numpy()), bits(before["frame"]))
        assert list(rt.render_ao_filtered(dirs, K, plane_max=0.1)) == ["ao"]
        # the live context: a pose, hidden objects, moved objects
        rot = rotation((0.0, 1.0, 0.0), 0.08) @ rotation((1.0, 0.0, 0.0), -0.05)
        origin = (0.3, -0.2, 0.5)
        rt.set_pose(w, h, z, rot, origin)
        cpu.set_pose(w, h, z, rot, origin)
        mask = random_mask(len(objs), seed=33)
        mask[0] = mask[-1] = 1
        mask[len(objs) // 2] = 0
        rt.set_visibility(mask)
        moves = [nudged(objs, int(np.flatnonzero(mask)[0]), (0.5, -0.3, 0.4)), nudged(objs, int(np.flatnonzero(mask)[-1]), (-0.4, 0.2, -0.6))]
        now = R.with_visibility(objs, mask)
        for i, t in moves:
            rt.set_transforms(t, i)
            now = R.with_transforms(now, t, i)
        posed = rt.render_ao_filtered(dirs, K, BIAS, want=MEMBERS, **FILTER)
        same(posed, defined(rt, w, K, dirs))
        cpu_now = CPURaytracer(now, lts, pinhole_rays(w, h, z), 0, kernel="hittest")
        cpu_now.set_pose(w, h, z, rot, origin)
        same(posed, cpu_now.render_ao_filtered(dirs, K, BIAS, **FILTER))                # (the pose's width)
        assert not np.array_equal(posed["taps"], got["taps"])


@pytest.mark.parametrize("name", ["small", "large"])
def test_under_supersampling_the_frame_form_filters_samples(name):
    objs, lts, w, h, z = frame_scene(name)
    w, h = w // 2, h // 2
    z = z / 2
    K = 4
    dirs = table(K)
    sw, sh, sz = camera.supersampled(w, h, z, 2)
    cpu = CPURaytracer(objs, lts, pinhole_rays(sw, sh, sz), 0, kernel="hittest")
    with hip(objs, lts, None, DEPTH, camera=(w, h, z), supersample=2) as rt:
        before = rt.Render()
        assert rt.local_rays == 4 * w * h == sw * sh
        got = rt.render_ao_filtered(dirs, K, BIAS, want=MEMBERS, **FILTER)
        assert len(got["ao"]) == 4 * w * h
        same(got, defined(rt, sw, K, dirs))
        same(got, cpu.render_ao_filtered(dirs, K, BIAS, width=sw, **FILTER))
        after = rt.Render()
        assert len(after) == w * h and np.array_equal(bits(after), bits(before))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    import torch
    from opencl_raytracer_amd.hip_raytracer import load_library
    objs = cloud()
    n, K = W * H, 8
    dirs = table(K)
    d_dirs = torch.from_numpy(dirs).cuda()
    big, out = guarded(n)
    host_ao = np.full(n, 5.0, dtype=F)
    point = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros((n + 1,), dtype=torch.uint8, device="cuda")
    inf, nan = float("inf"), float("nan")

    def P(samples=K, n_sets=16, bias=BIAS, reserved=0, dirs=d_dirs.data_ptr()):
        return RTAOParams(samples, n_sets, bias, reserved, dirs)

    def FP(radius=2, normal_min=0.9, plane_max=0.1, reserved=0):
        return RTAOFilterParams(radius, normal_min, plane_max, reserved)

    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        lib, ctx = rt._lib, rt._ctx
        info = RTAOFilterInfo()
        assert lib.rt_get_ao_filter_info(ctx, ctypes.byref(info)) == -5                 # RT_ERR_STATE before the first pass
        before = snapshot(rt)
        first = rt.render_ao_filtered(dirs, K, BIAS, want=MEMBERS, **FILTER)
        said = rt.ao_filter_info()
        all3 = RTAOFiltered(out["ao"].data_ptr(), out["grey"].data_ptr(), out["taps"].data_ptr())
        host3 = RTAOFiltered(host_ao.ctypes.data, None, None)
        ok, fok = P(), FP()
        cp, pp = VP(counts.data_ptr()), VP(point.data_ptr())

        def frame_dev(p=ok, f=fok, o=all3):
            return lib.rt_render_ao_filtered_device(ctx, ctypes.byref(p) if p else None, ctypes.byref(f) if f else None, ctypes.byref(o) if o else None, None)

        def frame_host(p, f=fok, o=host3):
            return lib.rt_render_ao_filtered(ctx, ctypes.byref(p) if p else None, ctypes.byref(f) if f else None, ctypes.byref(o) if o else None)

        def alone(u=cp, p=pp, nr=pp, ix=None, width=W, rows=H, samples=K, f=fok, o=all3):
            return lib.rt_ao_filter_device(ctx, u, p, nr, ix, width, rows, samples, ctypes.byref(f) if f else None, ctypes.byref(o) if o else None, None)

        bad_filters = [FP(radius=0), FP(radius=5), FP(plane_max=-1e-3), FP(plane_max=inf), FP(plane_max=nan), FP(reserved=1)]
        bad_params = [P(samples=0), P(samples=3), P(samples=128), P(n_sets=0), P(n_sets=4097), P(bias=-1e-3), P(bias=inf), P(bias=nan),
                      P(reserved=1), P(dirs=None)]
        host_ok = P(dirs=dirs.ctypes.data)
        refused = [lambda f=f: frame_dev(f=f) for f in bad_filters] + [lambda f=f: frame_host(host_ok, f=f) for f in bad_filters]
        refused += [lambda f=f: alone(f=f) for f in bad_filters]
        refused += [lambda p=p: frame_dev(p=p) for p in bad_params] + [lambda p=p: frame_host(p) for p in bad_params]
        refused += [lambda k=k: alone(samples=k) for k in (0, 3, 128)]
        refused += [
            lambda: frame_dev(p=None), lambda: frame_dev(f=None), lambda: frame_dev(o=None), lambda: frame_dev(o=RTAOFiltered()),
            lambda: frame_host(None), lambda: frame_host(host_ok, o=RTAOFiltered()), lambda: frame_host(host_ok, o=None),
            lambda: frame_dev(p=P(dirs=d_dirs.data_ptr() + 4)),
            lambda: frame_dev(o=RTAOFiltered(out["ao"].data_ptr() + 2, None, None)),
            lambda: alone(f=None), lambda: alone(o=None), lambda: alone(o=RTAOFiltered()),
            lambda: alone(o=RTAOFiltered(out["ao"].data_ptr() + 2, None, None)),
            lambda: alone(u=None), lambda: alone(p=None), lambda: alone(nr=None),
            lambda: alone(p=VP(point.data_ptr() + 8), rows=H - 1), lambda: alone(nr=VP(point.data_ptr() + 4), rows=H - 1),
            lambda: alone(ix=VP(point.data_ptr() + 2)),
            lambda: alone(width=1 << 40, rows=1 << 40),                                   # width * rows overflows
            lambda: lib.rt_ao_filter(ctx, None, None, None, None, W, H, K, ctypes.byref(fok), ctypes.byref(host3)),
        ]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        # RT_ERR_STATE: a sharded context
        rt.set_shard(16 * W, 0, 2)
        assert frame_dev() == -5 and frame_host(host_ok) == -5 and lib.rt_last_error(ctx)
        with pytest.raises(RTError) as e:
            rt.render_ao_filtered(dirs, K, plane_max=0.1)
        assert e.value.code == -5
        rt.set_shard(n, 0, 1)
        torch.cuda.synchronize()
        guards_stand(big, n)
        assert (host_ao == 5.0).all()
        now = rt.ao_filter_info()
        assert all(now[k] == said[k] for k in ("n_items", "n_live", "accepted"))          # the last pass is still the last pass
        # n == 0 is RT_OK with nothing launched; an unaligned byte input is fine
        assert alone(u=None, p=None, nr=None, width=0, rows=5) == 0 and alone(width=7, rows=0) == 0
        scratch = torch.empty(n, dtype=torch.float32, device="cuda")
        assert alone(u=VP(counts.data_ptr() + 1), o=RTAOFiltered(scratch.data_ptr(), None, None)) == 0
        torch.cuda.synchronize()
        assert_same(snapshot(rt), before, "the frame after the refusals")
        again = rt.render_ao_filtered(dirs, K, BIAS, want=MEMBERS, **FILTER)
        same(again, first)
        g = rt.render_gbuffer()
        u = rt.render_ao(dirs, K, BIAS, want=("unoccluded",))["unoccluded"]
        # primary rays from a plain ray buffer: it has no width
        rt.set_rays(pinhole_rays(W, H, Z))
        held = rt.Render()
        assert frame_dev() == -5 and frame_host(host_ok) == -5 and lib.rt_last_error(ctx)
        torch.cuda.synchronize()
        guards_stand(big, n)
        assert (host_ao == 5.0).all() and np.array_equal(bits(rt.Render()), bits(held))
    with hip(objs, lights(), pinhole_rays(W, H, Z), DEPTH, raygen=False) as rt:            # RT_FLAG_NO_RAYGEN
        held = rt.Render()
        with pytest.raises(RTError) as e:
            rt.render_ao_filtered(dirs, K, plane_max=0.1)
        assert e.value.code == -5 and np.array_equal(bits(rt.Render()), bits(held))
        same(rt.ao_filter(u, g["point"], g["normal"], g["index"], W, K, want=MEMBERS, **FILTER), first)       # the pass alone works
    # no primary rays yet: the frame form is RT_ERR_STATE, the pass alone works
    lib = load_library()
    o, lts = np.ascontiguousarray(objs), np.ascontiguousarray(lights())
    ctx = VP()
    assert lib.rt_create(ctypes.byref(ctx), o.ctypes.data_as(VP), len(o), lts.ctypes.data_as(VP), len(lts), None, n, 0, 0, 0, 0) == 0
    try:
        assert lib.rt_render_ao_filtered(ctx, ctypes.byref(host_ok), ctypes.byref(fok), ctypes.byref(host3)) == -5
        assert lib.rt_last_error(ctx) and (host_ao == 5.0).all()
        p, nr, ix = (np.ascontiguousarray(g[k]) for k in ("point", "normal", "index"))
        assert lib.rt_ao_filter(ctx, u.ctypes.data_as(VP), p.ctypes.data_as(VP), nr.ctypes.data_as(VP), ix.ctypes.data_as(VP), W, H, K,
                                ctypes.byref(fok), ctypes.byref(host3)) == 0
        assert np.array_equal(bits(host_ao), bits(first["ao"]))
    finally:
        lib.rt_destroy(ctx)


def test_a_triangle_context_refuses_the_frame_form():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    K = 4
    dirs = table(K)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = rt.Render()
        with pytest.raises(RTError) as e:
            rt.render_ao_filtered(dirs, K, plane_max=0.1)
        assert e.value.code == -5
        assert np.array_equal(bits(rt.Render()), bits(before))


def test_the_several_gpu_object_filters_through_shard_0():
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    width, rows, K, r = 65, 5, 4, 3
    u, p, nr, ix = field(width, rows, K, seed=5)
    with MultiHIPRaytracer(cloud(), lights(), None, DEPTH, devices=(0, 0), camera=(W, H, Z)) as rt:
        got = rt.ao_filter(u, p, nr, ix, width, K, r, 0.9, plane_max=0.05, want=MEMBERS)
        same(got, AO.filter(u, p, nr, ix, width, K, r, 0.9, 0.05))
        assert rt.ao_filter_info()["accepted"] == int(got["taps"].sum())
        assert not hasattr(rt, "render_ao_filtered")
