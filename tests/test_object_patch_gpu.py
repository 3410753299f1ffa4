"""GPU: what rt_set_materials, rt_set_transforms, rt_set_visibility (and rt_set_lights) share on the host (csrc/rt_object_patch.cpp,
rt_multi.cpp) - the records read back against records.with_materials / with_transforms / with_visibility on bytes, the frames against
a FRESH context created with the composed records, on uint32 words, with rays_reference and hit_pixels.

1. one staging buffer under every order of the three host forms (stale bytes past a call's count, the transforms' slot offset, growth
between calls); 2. the device forms, which never touch it, between them; 3. RT_FLAG_DEVICE_OPENCL's predicate on the lights through
its three callers, flipping at every step; 4. the all-or-none loop of the four _multi calls. Depth 2, 64 x 48 frames."""
import ctypes

import numpy as np
import pytest

from helpers import R, light_in_reach
from test_primary_depth_order_gpu import bits, hip
from test_set_lights_cpu import POSITIONS, make_lights
from test_set_materials_cpu import live_words, new_materials
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, fresh, lights, same_records, small, snapshot
from test_set_transforms_cpu import new_transforms, transform
from test_set_transforms_gpu import FRONT
from test_set_visibility_gpu import lonely_object, random_mask, same_info, shown

pytestmark = pytest.mark.gpu
U8 = np.uint8
IN_BOX = dict(centre=(0.0, 0.0, -36.0), spread=3.0)   # places inside the box the cloud's grid was built for


# ---- 1, 2. one staging buffer --------------------------------------------------------------------------------------------------
def stage_steps():
    """[(kind, first, array)]: 7 B, 396 B (slots at byte 384), 3840 B, 200 B into the larger buffer, 5280 B (grows; slots at byte 5120),
    64 B. 3 + 40 = 43 distinct moved objects: inside the dynamic set's 64."""
    return [("visibility", 5, random_mask(7, seed=101)), ("transforms", 10, new_transforms(3, seed=102, **IN_BOX)),
            ("materials", 20, new_materials(60, seed=103)), ("visibility", 0, random_mask(N, seed=104)),
            ("transforms", 60, new_transforms(40, seed=105, **IN_BOX)), ("materials", N - 1, new_materials(1, seed=106))]


def composed(steps):
    """(records, mask) after these steps on the cloud: the materials and matrices, and one byte per object."""
    records, mask = cloud(), np.ones(N, dtype=U8)
    for kind, first, a in steps:
        if kind == "materials":
            records = R.with_materials(records, a, first)
        elif kind == "transforms":
            records = R.with_transforms(records, a, first)
        else:
            mask[first:first + len(a)] = shown(a)
    return records, mask


def assert_reads(rt, steps, label):
    records, mask = composed(steps)
    assert same_records(rt.read_materials(), live_words(records)), label
    assert same_records(rt.read_transforms(), R.transforms_of(records)), label
    assert np.array_equal(rt.read_visibility(), mask), label


def fresh_after(k):
    records, mask = composed(stage_steps()[:k])
    return fresh(("object patch", k), R.with_visibility(records, mask))


def host_form(rt, kind, first, a):
    getattr(rt, "set_" + kind)(a, first)


def test_one_stage_every_order():
    steps = stage_steps()
    assert [a.nbytes + (4 * len(a) if kind == "transforms" else 0) for kind, _, a in steps] == [7, 396, 3840, 200, 5280, 64]
    with hip(cloud(), lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for k, step in enumerate(steps, 1):
            host_form(rt, *step)
            assert_reads(rt, steps[:k], f"step {k}")
            if k in (3, 6):
                assert_same(snapshot(rt), fresh_after(k), f"step {k}")
        assert rt.geometry_info()["n_dynamic"] == 43


def test_device_forms_between_host_forms():
    import torch
    steps = stage_steps()
    other = new_materials(60, seed=107)
    d_other = torch.from_numpy(other.view(np.float32).reshape(-1, 16).copy()).cuda()
    d_same = torch.from_numpy(steps[2][2].view(np.float32).reshape(-1, 16).copy()).cuda()
    d_inverse = torch.from_numpy(steps[3][2] == 0).cuda()
    d_mask = torch.from_numpy(steps[3][2].copy()).cuda()
    with hip(cloud(), lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        host_form(rt, *steps[0])
        host_form(rt, *steps[1])
        rt.set_materials(d_other, 20)                 # other materials from device memory, then step 3 from the stage over them
        assert same_records(rt.read_materials(20, 60), live_words(other))
        host_form(rt, *steps[2])
        assert_reads(rt, steps[:3], "step 3 behind a device form")
        rt.set_visibility(d_inverse)                  # the inverse mask from device memory, then step 4 from the stage over it
        assert np.array_equal(rt.read_visibility(), shown(steps[3][2] == 0))
        assert_reads(rt, steps[:3] + [("visibility", 0, steps[3][2] == 0)], "the inverse mask")
        host_form(rt, *steps[3])
        assert_reads(rt, steps[:4], "step 4 behind a device form")
        rt.set_materials(d_other, 20)                 # ... and the device forms last: steps 3 and 4 again, neither through the stage
        rt.set_visibility(d_inverse)
        rt.set_materials(d_same, 20)
        rt.set_visibility(d_mask)
        assert_reads(rt, steps[:4], "steps 3 and 4 as device forms")
        got4 = snapshot(rt)
        host_form(rt, *steps[4])
        host_form(rt, *steps[5])
        assert_reads(rt, steps, "step 6")
        assert_same(snapshot(rt), fresh_after(6), "step 6")
    assert_same(got4, fresh_after(4), "step 4")


# ---- 3. one predicate, three callers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_one_predicate_three_callers(size):
    objs = cloud() if size == "large" else small()
    n = len(objs)
    A, at = lonely_object(objs)
    B = next(i for i in range(n) if i != A)
    out, lit = make_lights((0.0, 0.0, -25.0), POSITIONS["+y"]), make_lights(at, POSITIONS["+y"])
    assert not light_in_reach(objs, (0.0, 0.0, -25.0)) and light_in_reach(objs, at)
    hide, show = np.zeros(1, dtype=U8), np.ones(1, dtype=U8)
    off, onto = transform(FRONT[1], None, (0.7, 0.7, 0.7)), transform(at, None, (0.3, 0.3, 0.3))
    # (caller, the call on the live context, the records a fresh context is created with, its lights, the flag afterwards).
    # tiles_info: rt_set_visibility rebuilds no table and a table lists candidates by their spheres, so the table
    # the flag's flip makes the live context build while A is hidden still lists A - its three list sizes are those of a fresh
    # context that shows A (under lights that leave it the default path), every other field the hidden fresh context's. The two
    # moves keep the box, and with it the cell, the grid was built for: the registration spheres, and so the tables, are a fresh grid's.
    moved_A = R.with_transforms(objs, off, A)
    moved_AB = R.with_transforms(moved_A, onto, B)
    steps = [("rt_set_lights: a light in A's reach", lambda c: c.set_lights(lit), objs, lit, 1),
             ("rt_set_visibility: A hidden", lambda c: c.set_visibility(hide, A), R.with_visibility(objs, hide, A), lit, 0),
             ("rt_set_visibility: A shown", lambda c: c.set_visibility(show, A), objs, lit, 1),
             ("rt_set_transforms: A off the light", lambda c: c.set_transforms(off, A), moved_A, lit, 0),
             ("rt_set_transforms: B onto the light", lambda c: c.set_transforms(onto, B), moved_AB, lit, 1),
             ("rt_set_lights: the light out again", lambda c: c.set_lights(out), moved_AB, out, 0)]
    kw = dict(camera=(W, H, Z), device_opencl=True)
    with hip(objs, out, None, DEPTH, **kw) as rt:
        assert rt.rays_info()["literal"] == 0
        for label, call, records, lts, literal in steps:
            call(rt)
            assert rt.rays_info()["literal"] == literal, label
            got, got_tiles = snapshot(rt), rt.tiles_info()
            with hip(records, lts, None, DEPTH, **kw) as ref:
                assert ref.rays_info()["literal"] == literal, label
                want, want_tiles = snapshot(ref), ref.tiles_info()
            if label.endswith("A hidden"):
                with hip(objs, out, None, DEPTH, **kw) as listed:
                    want_tiles.update({k: v for k, v in listed.tiles_info().items() if k in ("n_entries", "max_list", "n_global")})
            print(size, label, got_tiles, want_tiles)
            assert_same(got, want, f"{size}: {label}")
            same_info(got_tiles, want_tiles, f"{size}: {label}")


# ---- 4. all or none ------------------------------------------------------------------------------------------------------------
def multi_cases(name):
    """(accepted call on a wrapper, the fresh context's objects and lights, [refused raw argument tuples])"""
    objs = cloud()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if name == "lights":
        lts = make_lights(POSITIONS["-x"], (0.0, 0.0, -25.0), POSITIONS["+z"])
        buf = np.ascontiguousarray(lts)
        return (lambda c: c.set_lights(lts)), objs, lts, buf, [(None, 2), (ptr(buf), 1 << 22)]
    if name == "materials":
        mats = new_materials(190, seed=111)
        buf = np.ascontiguousarray(mats)
        return (lambda c: c.set_materials(mats, 3)), R.with_materials(objs, mats, 3), lights(), buf, \
            [(ptr(buf), N - 1, 2), (ptr(buf), 0xffffffff, 2), (None, 0, 2), (None, N, 2)]
    if name == "transforms":
        xf = new_transforms(5, seed=112, **IN_BOX)
        buf = np.concatenate([xf[:1], transform((0.0, 0.0, -400.0))])   # the second record's bound leaves the box
        return (lambda c: c.set_transforms(xf, 30)), R.with_transforms(objs, xf, 30), lights(), buf, \
            [(ptr(buf), N - 1, 2), (ptr(buf), 0xffffffff, 2), (None, 0, 2), (None, N, 2), (ptr(buf), 40, 2)]
    mask = random_mask(190, seed=113)
    buf = np.ascontiguousarray(mask)
    return (lambda c: c.set_visibility(mask, 3)), R.with_visibility(objs, mask, 3), lights(), buf, \
        [(ptr(buf), N - 1, 2), (ptr(buf), 0xffffffff, 2), (None, 0, 2), (None, N, 2)]


@pytest.mark.parametrize("name", ["lights", "materials", "transforms", "visibility"])
def test_all_or_none(name):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    accepted, records, lts, _keep, refused = multi_cases(name)
    with MultiHIPRaytracer(cloud(), lights(), None, DEPTH, devices=(0, 0, 0), camera=(W, H, Z)) as m, \
            hip(cloud(), lights(), None, DEPTH, camera=(W, H, Z)) as single:
        constructor = m.Render()
        assert np.array_equal(bits(constructor[:W * H]), bits(single.Render()))
        multi_call, single_call = getattr(m._lib, f"rt_set_{name}_multi"), getattr(single._lib, f"rt_set_{name}")
        for k, args in enumerate(refused):
            code = single_call(single._ctx, *args)
            assert code == -1 and multi_call(m._m, *args) == code, (name, k)
            assert m._lib.rt_multi_last_error(m._m) == single._lib.rt_last_error(single._ctx) != b"", (name, k)   # (a check's refusal: the context's own text)
            assert np.array_equal(bits(m.Render()), bits(constructor)), (name, k)
        accepted(m)
        accepted(single)
        got = m.Render()
        assert np.array_equal(bits(got[:W * H]), bits(single.Render()))
    assert np.array_equal(bits(got[:W * H]), bits(fresh(("object patch multi", name), records, lts)["frame"]))
    assert not np.array_equal(bits(got), bits(constructor))
