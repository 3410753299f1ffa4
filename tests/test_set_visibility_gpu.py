"""GPU: replaceable visibility (rt_set_visibility, rt_set_visibility_device, rt_set_visibility_multi, rt_read_visibility) - the
type words read back from every device copy against the expected mask, and the frames against a FRESH context created with
records.with_visibility(objects, mask), on uint32 words, with rays_reference and hit_pixels.

1. the patch kernel's boundaries (one lane per object: 64 per wave, 128 per workgroup; the pad half of an odd count); 2. the two
halves of a pair and the shadow stream; 3. every kernel x path x arithmetic mode, triangles; 4. history; 5. with the other
live-context calls, in both orders; 6. the last sphere / box (the NaN-ray winner); 7. RT_FLAG_DEVICE_OPENCL's predicate on the
lights; 8. the device form behind a torch kernel on another stream; 9. refusals; 10. several contexts, several ranks.
Every test that hides something asserts that the frame differs from the unhidden one. Every test here fails on a library from
before the feature, on the missing symbol. Depth 2, 64 x 48 frames; the scenes are test_set_materials_gpu.py's cloud: 200 objects
(the round machine) and its first 40 (the small-scene kernel)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import R, ROOT, light_in_reach, object_reach, rotation
from opencl_raytracer_amd import ppm, rays as RY, sharding
from test_frame_shapes_cpu import camera_z_for, scene
from test_primary_depth_order_gpu import bits, box, hip, sphere
from test_set_lights_cpu import POSITIONS, make_lights
from test_set_materials_cpu import live_words, new_materials
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, fresh, lights, same_records, small, snapshot
from test_set_transforms_cpu import transform

pytestmark = pytest.mark.gpu
U8 = np.uint8
KERNELS = ("hittest", "shade", "shade_and_reflect")


def random_mask(n, seed, hidden=0.5):
    """n bytes, about `hidden` of them 0; the visible ones carry 1, 2 or 255 (anything non-zero shows)."""
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=n) < hidden, 0, rng.choice(np.array([1, 2, 255]), size=n)).astype(U8)


def shown(mask):
    return (np.asarray(mask) != 0).astype(U8)


def differs(a, b):
    return not np.array_equal(bits(a["frame"]), bits(b["frame"]))


def names_no_hidden_object(rt, mask):
    _, idx = rt.render_aux()
    hit = idx[idx >= 0]
    return hit.size > 0 and not np.isin(hit, np.nonzero(np.asarray(mask) == 0)[0]).any()


# ---- 1. kernel boundaries ------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 127, 128, 129)    # one object, a wave of 64 and a workgroup of 128 objects, each -1 / +1
FIRSTS = (0, 1, 3, 17)


@pytest.mark.parametrize("n_objs", [N, N - 1])
def test_kernel_boundaries(n_objs):
    objs = cloud(n_objs)
    ranges = [(f, c) for c in COUNTS for f in FIRSTS]
    ranges += [(n_objs - c, c) for c in COUNTS]                  # ending on the last object (199: its pair's other half is the pad)
    ranges += [(n_objs // 2, 1), (0, n_objs), (n_objs - 1, 1)]   # one object in the middle, every object, the last one alone
    expect = np.ones(n_objs, dtype=U8)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        materials, transforms = rt.read_materials(), rt.read_transforms()
        assert same_records(materials, live_words(objs)) and np.array_equal(rt.read_visibility(), expect)
        for k, (first, count) in enumerate(ranges):
            mask = random_mask(count, seed=200 + k)
            if k % 2 == 0:
                mask[0], mask[-1] = 0, 0                         # the ends of the range do change
            expect[first:first + count] = shown(mask)
            rt.set_visibility(mask, first)
            got = rt.read_visibility()                           # the WHOLE array, from every copy: the range set, every neighbour untouched
            assert np.array_equal(got, expect), (first, count, np.nonzero(got != expect)[0][:8])
            assert np.array_equal(rt.read_visibility(first, count), shown(mask))
            assert same_records(rt.read_materials(), materials) and same_records(rt.read_transforms(), transforms), (first, count)
        assert 0 < expect.sum() < n_objs
        got = snapshot(rt)
    assert_same(got, fresh(("vis boundaries", n_objs), R.with_visibility(objs, expect)), f"{n_objs} objects after {len(ranges)} patches")


# ---- 2. pair halves, the shadow stream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objs", [N, N - 1, 40, 39])
def test_pair_halves(n_objs):
    objs = cloud(n_objs)
    even, odd = (np.arange(n_objs) % 2).astype(U8), ((np.arange(n_objs) + 1) % 2).astype(U8)   # even: the even indices hidden
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        assert before["wavefront"] == (1 if n_objs >= 96 else 0)
        for label, mask in (("even hidden", even), ("odd hidden", odd)):
            rt.set_visibility(mask)
            got = snapshot(rt)
            assert np.array_equal(rt.read_visibility(), mask)
            assert differs(got, before) and names_no_hidden_object(rt, mask), label
            assert_same(got, fresh(("vis halves", n_objs, label), R.with_visibility(objs, mask)), f"{n_objs}: {label}")


def shadow_scene():
    """Index order is not size order (the shadow stream sorts by size: 1, 3, 2, 0, 4), and object 0 - a small sphere between
    the light and the big sphere 1 - shadows it. Five objects: the last pair of either stream has a pad half."""
    objs = [sphere(1, (0.3, 0.3, -30.0), 0.6), sphere(2, (0.0, 0.0, -40.0), 3.0), box(3, (-4.0, 2.5, -38.0), (1.2, 1.2, 1.2)),
            sphere(4, (4.0, -2.0, -36.0), 1.5), sphere(5, (-3.0, -3.0, -33.0), 0.3)]
    return R.objects_array(objs), make_lights((3.0, 3.0, -10.0))


@pytest.mark.parametrize("path", ["monolithic", "wavefront"])
def test_the_shadow_stream(path):
    objs, lts = shadow_scene()
    with hip(objs, lts, None, DEPTH, camera=(W, H, Z), path=path) as rt:
        before = snapshot(rt)
        _, idx_before = rt.render_aux()
        cases = [("the occluder", [0, 1, 1, 1, 1]), ("the receiver", [1, 0, 1, 1, 1]), ("both, and the last", [0, 0, 1, 1, 0]), ("the occluder again", [0, 1, 1, 1, 1])]
        for label, mask in cases:
            rt.set_visibility(mask)
            got = snapshot(rt)
            assert np.array_equal(rt.read_visibility(), np.array(mask, dtype=U8))
            assert names_no_hidden_object(rt, mask), label
            assert_same(got, fresh(("vis shadow", path, label), R.with_visibility(objs, mask), lts, path=path), f"{path}: {label}")
            if label == "the occluder":   # its shadow on the receiver is gone too: pixels that show the receiver in both frames change
                _, idx = rt.render_aux()
                both = (idx == 1) & (idx_before == 1)
                changed = np.any(bits(got["frame"]) != bits(before["frame"]), axis=1)
                assert (both & changed).sum() > 0 and (both & ~changed).sum() > 0
        rt.set_visibility([1] * 5)
        assert_same(snapshot(rt), before, f"{path}: all shown")


# ---- 3. every kernel x path x arithmetic mode ----------------------------------------------------------------------------------
MODES = {"default": {}, "unfused": dict(fused=False), "fast phong": dict(fast_phong=True), "device_opencl": dict(device_opencl=True)}
PATHS = {"small scene": dict(n=40), "round machine": dict(n=N), "literal": dict(n=N, literal=True), "no grid": dict(n=N, grid=False),
         "brute force": dict(n=N, off_box=True)}


def far_rays():
    return RY.posed_rays(W, H, Z, np.eye(3), (0.0, 0.0, 500.0))   # origins off the grid's box: a brute-force frame


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("path", list(PATHS))
def test_every_kernel_path_and_mode(path, mode):
    spec = dict(PATHS[path])
    objs = cloud(spec.pop("n"))
    off_box = spec.pop("off_box", False)
    kw = dict(spec, **MODES[mode])
    mask = random_mask(len(objs), seed=31)
    changed = R.with_visibility(objs, mask)
    for kernel in KERNELS:
        with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel=kernel, **kw) as rt, \
                hip(changed, lights(), None, DEPTH, camera=(W, H, Z), kernel=kernel, **kw) as ref:
            if off_box:
                rt.set_rays(far_rays()), ref.set_rays(far_rays())
                assert rt.rays_info()["grid_in_use"] == 0 and rt.rays_info()["grid_built"] == 1
            before = snapshot(rt)
            rt.set_visibility(mask)
            got, want = snapshot(rt), snapshot(ref)
            if path in ("small scene", "round machine"):
                assert got["wavefront"] == (1 if path == "round machine" and "literal" not in kw else 0)
            assert before["hits"] > got["hits"] > 0
            assert_same(got, want, f"{path}, {mode}, {kernel}")
            assert differs(got, before), (path, mode, kernel)          # hittest included: its times change
            rt.set_visibility(np.ones(len(objs), dtype=U8))
            assert_same(snapshot(rt), before, f"{path}, {mode}, {kernel}: shown again")


def test_triangles():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    assert (objs["type"] == 2).all() and len(objs) > 400
    mask = np.ones(len(objs), dtype=U8)
    mask[::3] = 0
    mask[100:171] = 0
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = snapshot(rt)
        rt.set_visibility(mask)
        got = snapshot(rt)
        assert np.array_equal(rt.read_visibility(), mask) and names_no_hidden_object(rt, mask)
        rt.set_visibility(np.ones(len(objs), dtype=U8))
        back = snapshot(rt)
    with hip(R.with_visibility(objs, mask), lts, None, DEPTH, camera=(W, H, z)) as rt:
        want = snapshot(rt)
    assert before["hits"] > want["hits"] > 100 and differs(got, before)
    assert_same(got, want, "triangles")
    assert_same(back, before, "triangles shown again")


# ---- 4. history ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_history(size):
    objs = cloud() if size == "large" else small()
    n = len(objs)
    A, B, C = random_mask(n, seed=41), random_mask(n, seed=42, hidden=0.8), random_mask(n, seed=43, hidden=0.2)
    nothing = np.zeros(n, dtype=U8)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as a, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as b:
        untouched = snapshot(a)
        a.set_visibility(A)
        hidden = snapshot(a)
        a.set_visibility(np.ones(n, dtype=U8))
        assert_same(snapshot(a), untouched, f"{size}: hide, then show")
        assert differs(hidden, untouched)
        for m in (A, B, C):                     # three masks in sequence, rendering in between ...
            a.set_visibility(m)
            a.Render()
        b.set_visibility(C[n // 2:], n // 2)    # ... against the last one alone, in two parts
        b.set_visibility(C[:n // 2])
        got_a, got_b = snapshot(a), snapshot(b)
        assert np.array_equal(a.read_visibility(), shown(C)) and np.array_equal(b.read_visibility(), shown(C))
        a.set_visibility(nothing)
        empty = snapshot(a)
        assert not a.read_visibility().any()
    want = fresh(("vis history", size), R.with_visibility(objs, C))
    assert_same(got_a, want, f"{size}: three masks")
    assert_same(got_b, want, f"{size}: the last one alone")
    assert_same(empty, fresh(("vis nothing", size), R.with_visibility(objs, nothing)), f"{size}: all hidden")
    assert empty["hits"] == 0 and untouched["hits"] > 0
    assert (bits(empty["frame"]) == bits(empty["frame"])[0]).all()   # the background, on every pixel


# ---- 5. with the other live-context calls --------------------------------------------------------------------------------------
def same_info(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        if k != "build_device_ms":
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (label, k, a[k], b[k])


def test_with_the_other_live_context_calls(monkeypatch):
    import torch
    for knob in ("RT_RENDER_PASSES", "RT_RENDER_SPLIT"):
        monkeypatch.delenv(knob, raising=False)
    objs = cloud()
    mask = random_mask(N, seed=51)
    everything = np.ones(N, dtype=U8)
    changed = R.with_visibility(objs, mask)
    M, inside, outside = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0), (1.0, 0.5, 60.0)
    turned = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    d_rays = torch.from_numpy(turned.view(np.float32).reshape(-1, 8).copy()).cuda()
    other_lights = make_lights(POSITIONS["-x"], (0.0, 0.0, -25.0), POSITIONS["+z"])
    acts = [("pose inside the box", lambda c: c.set_pose(W, H, Z, M, inside)), ("pose outside the box", lambda c: c.set_pose(W, H, Z, M, outside)),
            ("rays (numpy, off the box)", lambda c: c.set_rays(far_rays())), ("rays (torch)", lambda c: c.set_rays(d_rays)),
            ("camera", lambda c: c.set_camera(H, W, -120.0)), ("lights", lambda c: c.set_lights(other_lights)),
            ("camera back", lambda c: c.set_camera(W, H, Z)), ("lights back", lambda c: c.set_lights(lights())),
            ("supersampling", lambda c: c.set_supersampling(2)), ("supersampling off", lambda c: c.set_supersampling(1)),
            ("shard, world 2", lambda c: c.set_shard(8 * W, 1, 2)), ("shard, world 3", lambda c: c.set_shard(8 * W, 2, 3)), ("shard off", lambda c: c.set_shard(0, 0, 1))]
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as after, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as before, \
            hip(changed, lights(), None, DEPTH, camera=(W, H, Z)) as ref:
        untouched = snapshot(before)
        after.set_visibility(mask)                 # `after`: the mask first, every other call behind it
        assert differs(snapshot(after), untouched)
        for label, act in acts:
            act(after), act(ref), act(before)      # `before`: the other call first, the mask behind it
            infos = [(before.tiles_info(), before.light_tiles_info(), before.geometry_info())]
            before.set_visibility(mask)
            infos.append((before.tiles_info(), before.light_tiles_info(), before.geometry_info()))
            for x, y in zip(*infos):               # no table is rebuilt
                same_info(x, y, label)
            want = snapshot(ref)
            assert_same(snapshot(after), want, f"{label}, then the mask")
            assert_same(snapshot(before), want, f"the mask, then {label}")
            before.set_visibility(everything)
        # the other two patch calls go by the create-time type: on a hidden and on a visible object, in both orders
        h, v = int(np.nonzero(mask == 0)[0][3]), int(np.nonzero(mask)[0][3])
        mats = new_materials(60, seed=52)
        moved = {h: transform((-2.0, 1.0, -30.0), rotation((1.0, 1.0, 0.2), 0.9), (1.0, 0.7, 1.2)), v: transform((2.0, -1.0, -29.0), None, (0.8, 0.8, 0.8))}
        records = objs
        steps = [("materials", lambda c: c.set_materials(mats, min(h, v)), lambda o: R.with_materials(o, mats, min(h, v))),
                 ("transform of a hidden object", lambda c: c.set_transforms(moved[h], h), lambda o: R.with_transforms(o, moved[h], h)),
                 ("transform of a visible object", lambda c: c.set_transforms(moved[v], v), lambda o: R.with_transforms(o, moved[v], v))]
        for label, act, definition in steps:
            act(after), act(before)
            before.set_visibility(mask)
            records = definition(records)
            want = fresh(("vis others", label), R.with_visibility(records, mask))
            assert_same(snapshot(after), want, f"the mask, then {label}")
            assert_same(snapshot(before), want, f"{label}, then the mask")
            before.set_visibility(everything)
        assert after.geometry_info()["n_dynamic"] == 2 and after.geometry_info()["dynamic_ids"][:2] == [h, v]   # a moved hidden object is dynamic like any other
        want = fresh(("vis others", "packed"), R.with_visibility(records, mask))["frame"]
        assert np.array_equal(ppm.quantise_bytes(want), after.render_packed("rgba8"))
        pieces = []
        for rank in range(3):   # three shards of 8-row tiles, stitched
            after.set_shard(8 * W, rank, 3)
            pieces.append(after.Render())
        after.set_shard(0, 0, 1)
        assert np.array_equal(bits(sharding.assemble_frame(pieces, 8 * W, W * H)), bits(want))
        monkeypatch.setenv("RT_RENDER_PASSES", "3")
        assert np.array_equal(bits(after.Render()), bits(want))
        monkeypatch.delenv("RT_RENDER_PASSES")
        after.set_visibility(everything)           # what the other calls set on a hidden object shows when it is shown
        assert_same(snapshot(after), fresh(("vis others", "shown"), records), "everything shown again")


# ---- 6. the last sphere / box --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["wavefront", "auto"])
def test_the_last_sphere_or_box_decides_a_nan_ray(path):
    """test_device_opencl_fuzz_gpu.py's tiny far box: a fifth of its hit points get a zero normal and, under the default arithmetic,
    a NaN reflection ray, which the reference shades with the LAST sphere / box of the scene. Behind the scene two objects no ray
    reaches: a sphere, then a box. Hiding the box makes the sphere the winner, hiding both a background object."""
    from test_device_opencl_fuzz_gpu import obj, tiny_far_box_scene
    scene_objs, lts, rays = tiny_far_box_scene()
    objs = R.objects_array(list(scene_objs) + [obj(R.SPHERE, (0.0, 0.0, 5.0e4), 1.0, seed=98), obj(R.BOX, (0.0, 5.0e4, 0.0), 1.0, seed=99)])
    n = len(objs)
    assert objs["type"][n - 2] == R.SPHERE and objs["type"][n - 1] == R.BOX and objs["type"][n - 3] == R.BOX
    masks = {"the box": [1, 1, 0], "the box and the sphere": [1, 0, 0], "the sphere": [1, 0, 1], "none": [1, 1, 1]}
    frames = {}
    with hip(objs, lts, rays, 3, path=path) as rt:
        untouched = snapshot(rt)
        for label, tail in masks.items():
            rt.set_visibility(tail, n - 3)
            frames[label] = snapshot(rt)
            with hip(R.with_visibility(objs, tail, n - 3), lts, rays, 3, path=path) as ref:
                assert_same(frames[label], snapshot(ref), f"{path}: hidden: {label}")
    nan_route = np.any(bits(frames["the box"]["frame"]) != bits(untouched["frame"]), axis=1).sum()
    assert nan_route > 100                                               # the pixels whose ray ends on the winner: it changed kind, box -> sphere
    assert differs(frames["the box and the sphere"], frames["the box"])  # ... and sphere -> the tiny box itself
    assert_same(frames["the sphere"], untouched, f"{path}: the winner is the box again")
    assert_same(frames["none"], untouched, f"{path}: all shown")


# ---- 7. RT_FLAG_DEVICE_OPENCL's predicate --------------------------------------------------------------------------------------
def lonely_object(objs):
    """(index, centre): an object whose centre lies in no other object's reach - a light there makes the context literal for it alone."""
    centre, reach = object_reach(objs)
    for i in range(len(objs)):
        if np.isfinite(reach[i]) and not light_in_reach(np.delete(objs, i), centre[i].astype(np.float32), slack=0.05):
            return i, tuple(float(x) for x in centre[i].astype(np.float32))
    raise AssertionError("every centre lies in another object's reach")


@pytest.mark.parametrize("size", ["large", "small"])
def test_device_opencl_predicate_skips_hidden_objects(size):
    objs = cloud() if size == "large" else small()
    A, at = lonely_object(objs)
    lts = make_lights(at, POSITIONS["+y"])
    later = make_lights(POSITIONS["-x"], tuple(np.float32(x) + np.float32(0.001) for x in at))
    hide_A = np.ones(len(objs), dtype=U8)
    hide_A[A] = 0
    kw = dict(device_opencl=True)
    with hip(objs, lts, None, DEPTH, camera=(W, H, Z), **kw) as rt:
        assert rt.rays_info()["literal"] == 1
        untouched = snapshot(rt)
        rt.set_visibility([0], A)
        assert rt.rays_info()["literal"] == 0
        got = snapshot(rt)
        rt.set_lights(later)                       # a later set_lights with A hidden: the light is still inside A's bound alone
        assert rt.rays_info()["literal"] == 0
        got_later = snapshot(rt)
        rt.set_visibility([1], A)
        assert rt.rays_info()["literal"] == 1
        shown_later = snapshot(rt)
        rt.set_lights(lts)
        assert rt.rays_info()["literal"] == 1
        assert_same(snapshot(rt), untouched, f"{size}: A shown, the first lights")
    with hip(R.with_visibility(objs, hide_A), lts, None, DEPTH, camera=(W, H, Z), **kw) as ref:
        assert ref.rays_info()["literal"] == 0
        assert_same(got, snapshot(ref), f"{size}: A hidden")
        ref.set_lights(later)
        assert ref.rays_info()["literal"] == 0
        assert_same(got_later, snapshot(ref), f"{size}: A hidden, later lights")
    assert differs(got, untouched)
    assert_same(shown_later, fresh(("vis opencl", size), objs, later, **kw), f"{size}: A shown, later lights")


# ---- 8. the device form --------------------------------------------------------------------------------------------------------
def test_device_form_behind_a_torch_kernel_on_another_stream():
    import torch
    objs = cloud()
    first, mask = 13, random_mask(170, seed=61)
    want = fresh("vis device form", R.with_visibility(objs, mask, first))
    inverse = torch.from_numpy(mask == 0).cuda()
    d_mask = torch.zeros_like(inverse)              # torch.bool: one byte per object
    work = torch.full((2048, 2048), 1.0 / 2048.0, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    expect = np.ones(N, dtype=U8)
    expect[first:first + 170] = shown(mask)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as dev, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as host:
        with torch.cuda.stream(side):
            for _ in range(8):                          # the stream is busy for a while ...
                work = work @ work
            torch.logical_not(inverse, out=d_mask)      # ... then a torch kernel fills the mask (until then it hides everything) ...
            dev.set_visibility(d_mask, first)           # ... immediately before the call, which is ordered behind it on that stream
        got = snapshot(dev)
        assert np.array_equal(dev.read_visibility(), expect)
        host.set_visibility(mask, first)
        assert_same(got, snapshot(host), "device form vs host form")
        assert_same(got, want, "device form vs fresh")
        # uint8 on the legacy default stream, at odd addresses, down to one object
        bytes_ = torch.from_numpy(np.concatenate([[7], mask, [9]]).astype(U8)).cuda()
        for shift, count in ((1, 170), (2, 3), (3, 1)):
            dev.set_visibility(torch.ones(170, dtype=torch.uint8, device="cuda"), first)
            dev.set_visibility(bytes_[shift:shift + count], first)
            expect[first:first + 170] = 1
            expect[first:first + count] = shown(mask[shift - 1:shift - 1 + count])
            assert bytes_[shift:].data_ptr() == bytes_.data_ptr() + shift
            assert np.array_equal(dev.read_visibility(), expect), (shift, count)
        dev.set_visibility(torch.zeros(N, dtype=torch.bool, device="cuda"))
        assert snapshot(dev)["hits"] == 0
        with pytest.raises(ValueError):
            dev.set_visibility(torch.ones(4, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            dev.set_visibility(torch.ones(4, dtype=torch.bool))


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    objs = cloud()
    mask = np.zeros(8, dtype=U8)
    ptr = mask.ctypes.data_as(ctypes.c_void_p)
    d_buf = torch.zeros(8, dtype=torch.uint8, device="cuda")
    d_ptr = ctypes.c_void_p(d_buf.data_ptr())
    out = np.full(8, 5, dtype=U8)
    o_ptr = out.ctypes.data_as(ctypes.c_void_p)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_visibility(random_mask(N, seed=71))
        before, words = snapshot(rt), rt.read_visibility()
        lib, ctx = rt._lib, rt._ctx
        refused = [lambda: lib.rt_set_visibility(ctx, ptr, N - 7, 8), lambda: lib.rt_set_visibility(ctx, ptr, N, 1),
                   lambda: lib.rt_set_visibility(ctx, ptr, 0xffffffff, 2), lambda: lib.rt_set_visibility(ctx, ptr, 2, 0xffffffff),   # first + count wraps 32 bits
                   lambda: lib.rt_set_visibility(ctx, None, 0, 3), lambda: lib.rt_set_visibility(ctx, ptr, N + 1, 0),
                   lambda: lib.rt_set_visibility_device(ctx, d_ptr, N - 7, 8, None), lambda: lib.rt_set_visibility_device(ctx, d_ptr, 0xffffffff, 2, None),
                   lambda: lib.rt_set_visibility_device(ctx, None, 0, 3, None),
                   lambda: lib.rt_read_visibility(ctx, o_ptr, N - 7, 8), lambda: lib.rt_read_visibility(ctx, o_ptr, 0xffffffff, 2),
                   lambda: lib.rt_read_visibility(ctx, None, 0, 3)]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert rt._lib.rt_last_error(ctx)
            assert np.array_equal(rt.read_visibility(), words), k
            assert_same(snapshot(rt), before, f"after refusal {k}")
        assert (out == 5).all()
        # count == 0 is RT_OK and changes nothing
        for call in (lambda: lib.rt_set_visibility(ctx, None, 0, 0), lambda: lib.rt_set_visibility(ctx, ptr, N, 0), lambda: lib.rt_set_visibility(ctx, ptr, 5, 0),
                     lambda: lib.rt_set_visibility_device(ctx, None, 0, 0, None), lambda: lib.rt_set_visibility_device(ctx, d_ptr, N, 0, None),
                     lambda: lib.rt_read_visibility(ctx, None, 0, 0)):
            assert call() == 0
        rt.set_visibility(mask[:0])
        assert np.array_equal(rt.read_visibility(), words)
        assert_same(snapshot(rt), before, "after empty calls")
        with pytest.raises(ValueError):
            R.with_visibility(objs, mask, N - 7)   # the definition refuses the same range


def test_an_object_created_with_another_type_is_left_alone():
    objs = cloud().copy()
    objs["type"][150] = 7
    objs["type"][151] = R.TYPE_HIDDEN
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        assert rt.read_visibility().all()          # never hit as they are, and reading as visible
        mask = np.ones(N, dtype=U8)
        mask[148:154] = 0
        rt.set_visibility(mask)
        mask[150:152] = 1
        assert np.array_equal(rt.read_visibility(), mask)
        got = snapshot(rt)
        rt.set_visibility(np.ones(N, dtype=U8))
        assert_same(snapshot(rt), before, "shown again")
    assert_same(got, fresh("vis other types", R.with_visibility(objs, mask)), "types of their own")


# ---- 10. several contexts, several ranks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_multi_set_visibility_equals_the_single_frame(shards):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs = cloud()
    first, mask = 3, random_mask(190, seed=81)
    want = fresh("vis multi", R.with_visibility(objs, mask, first))
    with MultiHIPRaytracer(objs, lights(), None, DEPTH, devices=(0,) * shards, camera=(W, H, Z)) as m:
        constructor = m.Render()
        m.set_visibility(mask, first)
        got = m.Render()
        buf = np.zeros(2, dtype=U8)
        assert m._lib.rt_set_visibility_multi(m._m, buf.ctypes.data_as(ctypes.c_void_p), N - 1, 2) == -1   # refused before any shard is touched
        assert m._lib.rt_set_visibility_multi(m._m, None, 0, 2) == -1
        assert np.array_equal(bits(m.Render()), bits(got))
        m.set_visibility(np.ones(N, dtype=U8))
        assert np.array_equal(bits(m.Render()), bits(constructor))
    assert np.array_equal(bits(got[:W * H]), bits(want["frame"]))
    assert not np.array_equal(bits(got), bits(constructor))


def test_two_contexts_do_not_see_each_others_masks():
    objs = cloud()
    mask = random_mask(N, seed=82)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as a, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as b:
        constructor = snapshot(b)
        a.set_visibility(mask)
        got_a, got_b = snapshot(a), snapshot(b)
        assert b.read_visibility().all() and np.array_equal(a.read_visibility(), shown(mask))
    assert_same(got_b, constructor, "the other context")
    assert_same(got_a, fresh("vis two contexts", R.with_visibility(objs, mask)), "the masked context")


def test_ranks_sharing_one_gpu_over_gloo():
    """world 2 over gloo on the one GPU: ShardedHIPRaytracer.set_visibility on every rank, gathered on rank 0, equals the single fresh
    context's frame, synchronous and pipelined, on the small-scene kernel and on the grid path."""
    world = 2
    port = 32700 + (os.getpid() % 1500) + 23
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "tests" / "mp_visibility_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count(": ok") == 4 and "MISMATCH" not in res.stdout, res.stdout
