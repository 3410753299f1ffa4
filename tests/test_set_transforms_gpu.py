"""GPU: replaceable transforms (rt_set_transforms, rt_set_transforms_multi, rt_read_transforms, rt_get_geometry_info) - the patched
records read back against records.with_transforms, and the frames against a FRESH context created with that object array, on
uint32 words, on every pixel, with rays_reference and hit_pixels.

1. the patch kernel's boundaries (eight lanes per object, the last pair's padding half); 2. every kernel and path; 3. the grid
path, where a stale table would show; 4. the registration spheres; 5. history; 6. with the other setters, in both orders;
7. RT_FLAG_DEVICE_OPENCL's predicate; 8. refusals; 9. a context that never calls the setter.
Every test that moves something asserts first that the frame after the move differs from the frame before, and where it names
a moved object that rt_render_aux's index buffer contains it. Every test here fails on a library from before the feature, on the
missing symbol - test 9 included, which asserts nothing about moved objects but needs rt_get_geometry_info for its n_dynamic.
Depth 2, 64 x 48 frames; the scenes are test_set_materials_gpu.py's cloud: 200 objects (the large-scene path), its first 80 (neither
a grid nor the small-scene kernel's spheres) and its first 40 (the small-scene kernel)."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import R, rotation
from opencl_raytracer_amd import ppm, rays as RY, sharding
from test_primary_depth_order_gpu import bits, hip
from test_set_lights_cpu import POSITIONS, make_lights
from test_set_materials_cpu import live_words, new_materials
from test_set_materials_gpu import DEPTH, H, N, W, Z, assert_same, cloud, lights, same_records, snapshot
from test_set_transforms_cpu import new_transforms, transform

pytestmark = pytest.mark.gpu
F = np.float32
_FRESH = {}
SCENES = {"small": 40, "80": 80, "large": N}
FRONT = [(-2.0, 1.0, -30.0), (2.0, -1.0, -29.0), (0.0, 2.5, -31.0)]   # free places in front of the cloud, inside the frame and the grid's box


def fresh(key, objs, lts=None, **kw):
    """Snapshot of a fresh context created with these objects; remembered per key."""
    if key not in _FRESH:
        kw.setdefault("camera", (W, H, Z))
        with hip(objs, lights() if lts is None else lts, None, DEPTH, **kw) as rt:
            _FRESH[key] = snapshot(rt)
    return _FRESH[key]


def differs(a, b):
    return not np.array_equal(bits(a["frame"]), bits(b["frame"]))


def first_of_type(objs, ty, skip=0):
    return int(np.nonzero(objs["type"] == ty)[0][skip])


def three_moves(objs):
    """[(object, TRANSFORM_DTYPE[1])]: one translated (its own rotation and scale), one rotated box, one non-uniformly scaled sphere
    of kappa^2 = 16 > 4 (the negative pre-test form on a grid) - each to a free place in front of the cloud."""
    a, b, c = first_of_type(objs, R.SPHERE, 3), first_of_type(objs, R.BOX, 2), first_of_type(objs, R.SPHERE, 5)
    mv = objs["mv"][a].reshape(4, 4).T.astype(np.float64)
    mv[:3, 3] = FRONT[0]
    inv = np.linalg.inv(mv)
    ta = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
    ta["mv"][0], ta["mvInverse"][0] = mv.T.astype(F).reshape(16), inv.T.astype(F).reshape(16)
    return [(a, ta), (b, transform(FRONT[1], rotation((1.0, 1.0, 0.2), 0.9), (1.0, 0.7, 1.2))), (c, transform(FRONT[2], rotation((0.0, 0.0, 1.0), 0.4), (1.2, 0.3, 0.6)))]


def apply(objs, moves):
    for i, t in moves:
        objs = R.with_transforms(objs, t, i)
    return objs


def seen_objects(rt):
    _, idx = rt.render_aux()
    return set(int(i) for i in np.unique(idx[idx >= 0]))


# ---- 1. patch boundaries -------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 63, 64, 65)
FIRSTS = (0, 1, 2, 17)


@pytest.mark.parametrize("n_objs", [N, N - 1])
def test_patch_boundaries(n_objs):
    objs = cloud(n_objs)
    ranges = [(f, c) for c in COUNTS for f in FIRSTS] + [(n_objs - c, c) for c in COUNTS]   # ... and ending on the last object
    expect = objs.copy()
    kw = dict(camera=(W, H, Z), grid=False)   # RT_FLAG_NO_GRID: no cap
    with hip(objs, lights(), None, DEPTH, kernel="hittest", **kw) as ht, hip(objs, lights(), None, DEPTH, **kw) as rt:
        before, times = snapshot(rt), ht.Render()
        materials = rt.read_materials()
        assert same_records(rt.read_transforms(), R.transforms_of(objs)) and same_records(ht.read_transforms(), R.transforms_of(objs))
        for k, (first, count) in enumerate(ranges):
            xf = new_transforms(count, seed=200 + k)
            expect = R.with_transforms(expect, xf, first)
            for c in (ht, rt):
                c.set_transforms(xf, first)
                got = c.read_transforms()                         # the WHOLE array: the range replaced, every neighbour untouched
                assert same_records(got, R.transforms_of(expect)), (first, count)
            assert same_records(rt.read_transforms(first, count), xf)
            assert same_records(rt.read_materials(), materials), (first, count)   # materials and type words survived
        assert rt.geometry_info()["n_dynamic"] == 0 and rt.geometry_info()["grid_built"] == 0
        got, got_times = snapshot(rt), ht.Render()
    assert differs(got, before)
    assert_same(got, fresh(("boundaries", n_objs), expect, grid=False), f"{n_objs} objects after {len(ranges)} patches")
    with hip(expect, lights(), None, DEPTH, kernel="hittest", **kw) as ht:
        want_times = ht.Render()
    assert np.array_equal(bits(got_times), bits(want_times)) and not np.array_equal(bits(got_times), bits(times))


# ---- 2. every kernel and path --------------------------------------------------------------------------------------------------
FLAGS = [("default", {}), ("unfused", dict(fused=False)), ("fast phong", dict(fast_phong=True)), ("device_opencl", dict(device_opencl=True)),
         ("literal", dict(literal=True)), ("no grid", dict(grid=False)), ("wavefront no grid", dict(grid=False, path="wavefront")),
         ("monolithic", dict(path="monolithic"))]


@pytest.mark.parametrize("size", list(SCENES))
@pytest.mark.parametrize("label,kw", FLAGS, ids=[f[0] for f in FLAGS])
def test_every_kernel_and_path(label, kw, size):
    objs = cloud(SCENES[size])
    moves = three_moves(objs)
    expect = apply(objs, moves)
    lts = make_lights((0.0, 0.0, -25.0), POSITIONS["+y"])   # (no light on an object, before or after: device_opencl stays off the literal loops)
    for kernel in ("hittest", "shade", "shade_and_reflect"):
        with hip(objs, lts, None, DEPTH, camera=(W, H, Z), kernel=kernel, **kw) as rt:
            before = snapshot(rt)
            for i, t in moves:
                rt.set_transforms(t, i)
            got = snapshot(rt)
            seen = seen_objects(rt)
            info = rt.geometry_info()
            assert same_records(rt.read_transforms(), R.transforms_of(expect))
        assert differs(got, before), (label, kernel)
        assert {i for i, _ in moves} <= seen, (label, kernel)
        assert_same(got, fresh((size, label, kernel), expect, lts, kernel=kernel, **kw), f"{size} {label} {kernel}")
        if size == "large" and kw.get("grid", True):
            assert info["grid_built"] == 1 and info["dynamic_ids"] == [i for i, _ in moves]
            if kernel == "shade_and_reflect" and label == "default":
                assert got["wavefront"] == 1
        else:
            assert info["n_dynamic"] == 0


# ---- 3. the grid path ----------------------------------------------------------------------------------------------------------
def primary_hits(objs):
    """rt_render_aux of the cloud: (t, index) per pixel, and its objects by the number of pixels they win, most first."""
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        t, idx = rt.render_aux()
    count = np.bincount(idx[idx >= 0], minlength=len(objs))
    return t, idx, [int(i) for i in np.argsort(-count) if count[i] > 0]


@functools.lru_cache(maxsize=None)
def grid_cases():
    objs = cloud()
    t, idx, vis = primary_hits(objs)
    hidden = [i for i in range(N) if i not in vis]   # objects no primary ray reaches: moved into view they change the frame
    assert len(hidden) >= 8
    cases = {}
    # (a) far from every cell it was registered in: found only through the always-list
    cases["far"] = ("shade_and_reflect", [(hidden[0], transform((1.0, 0.5, -12.0), None, (0.5, 0.5, 0.5)))], [hidden[0]])
    # (b) a slab high in the cloud, between its objects and the LAST light (+y) ...
    cases["shadows from the last light"] = ("shade_and_reflect", [(hidden[1], transform((0.0, 3.5, -40.0), None, (2.5, 0.25, 2.5)))], [])
    # ... and, under `shade`, a disc behind the first light, which sits in front of the cloud
    cases["shadows from a non-last light"] = ("shade", [(hidden[2], transform((0.6, 0.3, -29.0), None, (1.2, 1.2, 0.4)))], [hidden[2]])
    # (c) in front of a reflecting neighbour (absorption < 1), on the ray of one of ITS pixels at 0.9 of its hit time, so that the
    # moved object wins that pixel: secondary rays leave and hit dynamic objects (the mirror is named too, with its own matrices)
    mirror = next(i for i in vis if objs["absorption"][i] < 0.8)
    px = np.nonzero(idx == mirror)[0]
    p = int(px[len(px) // 2])
    row, col = divmod(p, W)
    point = 0.9 * float(t[p]) * np.array([col - W / 2.0, (H - row) - H / 2.0, Z])
    cases["in front of a mirror"] = ("shade_and_reflect", [(hidden[3], transform(point, None, (0.4, 0.4, 0.4))), (mirror, R.transforms_of(objs[mirror:mirror + 1]))],
                                     [hidden[3]])
    # (d) coincident, for the tie rules: one object onto a static one that is in view, and two onto each other at a free place
    same = [i for i in hidden[5:] if objs["type"][i] == objs["type"][hidden[4]]]
    twin = next(i for i in vis if objs["type"][i] == objs["type"][same[0]])
    place = transform(FRONT[0], rotation((0.3, 1.0, 0.0), 0.6), (1.0, 0.8, 1.1))
    cases["coincident"] = ("shade_and_reflect", [(same[0], R.transforms_of(objs[twin:twin + 1])), (hidden[4], place), (same[1], place)], [])
    # (e) 64 objects at once
    cases["64 at once"] = ("shade_and_reflect", [(10, new_transforms(64, seed=31, centre=(0.0, 0.0, -36.0), spread=3.0))], [])
    return objs, cases


@pytest.mark.parametrize("name", ["far", "shadows from the last light", "shadows from a non-last light", "in front of a mirror", "coincident", "64 at once"])
def test_grid_path(name):
    objs, cases = grid_cases()
    kernel, moves, named = cases[name]
    lts = make_lights((0.0, 0.0, -27.0), POSITIONS["+y"]) if name == "shadows from a non-last light" else lights()
    expect = apply(objs, moves)
    ids = [i + k for i, t in moves for k in range(len(t))]
    with hip(objs, lts, None, DEPTH, camera=(W, H, Z), kernel=kernel) as rt:
        before = snapshot(rt)
        lt_before, tiles_before = rt.light_tiles_info(), rt.tiles_info()
        assert rt.geometry_info()["n_dynamic"] == 0 and rt.geometry_info()["dynamic_capacity"] == 64
        for i, t in moves:
            rt.set_transforms(t, i)
        info, lt_after, tiles_after = rt.geometry_info(), rt.light_tiles_info(), rt.tiles_info()
        got = snapshot(rt)
        seen = seen_objects(rt)
        assert same_records(rt.read_transforms(), R.transforms_of(expect))
    assert differs(got, before), name
    assert set(named) <= seen, name
    if name == "64 at once":
        assert len(seen & set(ids)) > 20
    assert info["grid_built"] == 1 and info["dynamic_ids"] == ids and info["n_dynamic"] == len(ids) and info["n_unbounded"] == 0
    assert lt_after["enabled"] == lt_before["enabled"] and lt_after["source"] == (2 if lt_after["enabled"] else 0)
    assert lt_before["enabled"] == (1 if kernel == "shade_and_reflect" else 0)
    assert info["light_tiles_rebuilt"] == lt_after["enabled"]
    assert tiles_after["enabled"] == tiles_before["enabled"] == 1
    assert got["wavefront"] == 1
    assert_same(got, fresh(("grid", name), expect, lts, kernel=kernel), f"{name}: fresh default")
    assert_same(got, fresh(("grid", name, "no grid"), expect, lts, kernel=kernel, grid=False), f"{name}: fresh no-grid")


# ---- 4. the registration spheres -----------------------------------------------------------------------------------------------
def test_registration_spheres_equal_a_fresh_grids():
    objs = cloud()
    s = first_of_type(objs, R.SPHERE, 7)
    t = transform((0.5, 0.3, -40.0), None, (0.8, 0.8, 0.8))   # interior, uniform scale: box, cell and K2 of build_grid stay
    expect = R.with_transforms(objs, t, s)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt, hip(expect, lights(), None, DEPTH, camera=(W, H, Z)) as ref:
        a, b = rt.rays_info(), ref.rays_info()
        assert np.array_equal(a["box_lo"], b["box_lo"]) and np.array_equal(a["box_hi"], b["box_hi"]) and a["grid_built"] == b["grid_built"] == 1
        spheres, pre = rt.grid_spheres(), rt.grid_pretest()
        rt.set_transforms(t, s)
        got_s, got_p, want_s, want_p = rt.grid_spheres(), rt.grid_pretest(), ref.grid_spheres(), ref.grid_pretest()
        assert rt.light_tiles_info()["pretest_alpha"] == ref.light_tiles_info()["pretest_alpha"]   # the same K2
    assert np.array_equal(got_s.view(np.uint64), want_s.view(np.uint64)), np.nonzero((got_s != want_s).any(axis=1))[0]
    assert np.array_equal(bits(got_p), bits(want_p)), np.nonzero(got_p != want_p)[0]
    changed = np.nonzero((got_s != spheres).any(axis=1))[0]
    assert list(changed) == [s] and got_p[s] > 0 and np.array_equal(np.delete(got_p, s), np.delete(pre, s))


def test_anisotropic_dynamic_object_takes_the_negative_form():
    objs = cloud()
    s = first_of_type(objs, R.SPHERE, 7)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_transforms(transform((0.5, 0.3, -40.0), None, (1.2, 0.3, 0.6)), s)   # kappa^2 = 16
        sphere, pre = rt.grid_spheres()[s], rt.grid_pretest()[s]
    assert pre < 0 and abs(pre) < sphere[3] < abs(pre) * 1.1 and np.allclose(sphere[:3], (0.5, 0.3, -40.0), rtol=0, atol=1e-4)


# ---- 5. history ----------------------------------------------------------------------------------------------------------------
def test_history():
    objs = cloud()
    a, b = first_of_type(objs, R.SPHERE, 3), first_of_type(objs, R.BOX, 2)
    steps = [(a, transform(FRONT[0], None, (0.9, 0.9, 0.9))), (b, transform(FRONT[1], rotation((1.0, 0.0, 1.0), 0.5), (0.8, 1.1, 0.7))),
             (a, transform(FRONT[2], rotation((0.0, 1.0, 0.0), 1.0), (0.5, 1.3, 0.9))), (a, R.transforms_of(objs[a:a + 1]))]
    expect = objs
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        last = snapshot(rt)
        for k, (i, t) in enumerate(steps):
            rt.set_transforms(t, i)
            expect = R.with_transforms(expect, t, i)
            got = snapshot(rt)
            assert differs(got, last), k
            assert_same(got, fresh(("history", k), expect), f"step {k}")
            assert rt.geometry_info()["dynamic_ids"] == [a, b][:max(1, min(k + 1, 2))]
            last = got
        assert rt.geometry_info()["n_dynamic"] == 2
        rt.set_transforms(R.transforms_of(objs[b:b + 1]), b)   # ... and B back too: the constructor's frame, both still dynamic
        assert_same(snapshot(rt), fresh(("history", "constructor"), objs), "everything back")
        assert rt.geometry_info()["n_dynamic"] == 2


# ---- 6. with the other setters, in both orders ---------------------------------------------------------------------------------
def test_with_the_other_setters(monkeypatch):
    for knob in ("RT_RENDER_PASSES", "RT_RENDER_SPLIT"):
        monkeypatch.delenv(knob, raising=False)
    objs = cloud()
    moves = three_moves(objs)
    changed = apply(objs, moves)
    dyn = moves[0][0]
    mats = new_materials(1, seed=41)
    M, origin = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0)   # (inside the grid's box: the pose's tiles are built)
    turned = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, -0.5))
    other_lights = make_lights(POSITIONS["-x"], (0.0, 0.0, -25.0), POSITIONS["+z"])
    acts = [("pose", lambda c: c.set_pose(W, H, Z, M, origin)), ("rays", lambda c: c.set_rays(turned)), ("camera", lambda c: c.set_camera(H, W, -120.0)),
            ("lights", lambda c: c.set_lights(other_lights)), ("camera back", lambda c: c.set_camera(W, H, Z)),
            ("materials on a dynamic object", lambda c: c.set_materials(mats, dyn)),
            ("supersampling", lambda c: c.set_supersampling(2)), ("supersampling off", lambda c: c.set_supersampling(1))]

    def move(c):
        for i, t in moves:
            c.set_transforms(t, i)

    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as after, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as before, \
            hip(changed, lights(), None, DEPTH, camera=(W, H, Z)) as ref:
        constructor = snapshot(before)
        move(after)                                    # `after`: the move first, every other call behind it
        assert differs(snapshot(after), constructor)
        for label, act in acts:
            act(after), act(ref), act(before)          # `before`: the other call first, the move behind it
            move(before)
            want = snapshot(ref)
            assert_same(snapshot(after), want, f"move, then {label}")
            assert_same(snapshot(before), want, f"{label}, then move")
            if label in ("pose", "camera", "lights"):
                # tables built AFTER a move list the objects where they are: as large as a fresh context's, from the same spheres
                assert after.tiles_info()["enabled"] == ref.tiles_info()["enabled"] and after.tiles_info()["n_entries"] > 0
                assert after.light_tiles_info()["enabled"] == ref.light_tiles_info()["enabled"] == 1
                assert after.light_tiles_info()["source"] == 2
            for i, _ in moves:                         # `before` goes back to the constructor's places for the next act
                before.set_transforms(objs[i:i + 1], i)
        want = ref.Render()
        assert np.array_equal(ppm.quantise_bytes(want), after.render_packed("rgba8"))
        pieces = []
        for rank in range(2):                          # two shards of 8-row tiles, stitched
            after.set_shard(8 * W, rank, 2)
            pieces.append(after.Render())
        after.set_shard(0, 0, 1)
        assert np.array_equal(bits(sharding.assemble_frame(pieces, 8 * W, W * H)), bits(want))
        before.set_shard(8 * W, 1, 2)                  # ... and the shard first, the move behind it
        move(before)
        assert np.array_equal(bits(before.Render()), bits(pieces[1]))


def test_multi_set_transforms_equals_the_single_frame():
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs = cloud()
    moves = three_moves(objs)
    want = fresh("multi", apply(objs, moves))
    far = transform((0.0, 0.0, -400.0))
    with MultiHIPRaytracer(objs, lights(), None, DEPTH, devices=(0, 0), camera=(W, H, Z)) as m:
        constructor = m.Render()
        for i, t in moves:
            m.set_transforms(t, i)
        got = m.Render()
        assert m._lib.rt_set_transforms_multi(m._m, far.ctypes.data_as(ctypes.c_void_p), 3, 1) == -1   # refused before any shard is touched
        assert m._lib.rt_set_transforms_multi(m._m, None, 0, 2) == -1
        assert np.array_equal(bits(m.Render()), bits(got))
        for i, _ in moves:
            m.set_transforms(objs[i:i + 1], i)
        assert np.array_equal(bits(m.Render()), bits(constructor))
    assert np.array_equal(bits(got[:W * H]), bits(want["frame"]))
    assert not np.array_equal(bits(got), bits(constructor))


# ---- 7. RT_FLAG_DEVICE_OPENCL --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_device_opencl_predicate_follows_the_objects(size):
    objs = cloud(SCENES[size])
    light = (0.0, 0.0, -25.0)
    lts = make_lights(light, POSITIONS["+y"])
    s = first_of_type(objs, R.SPHERE, 3)
    onto, away = transform(light, None, (0.7, 0.7, 0.7)), transform(FRONT[1], None, (0.7, 0.7, 0.7))
    with hip(objs, lts, None, DEPTH, camera=(W, H, Z), device_opencl=True) as rt:
        before = snapshot(rt)
        assert rt.rays_info()["literal"] == 0
        rt.set_transforms(onto, s)
        assert rt.rays_info()["literal"] == 1
        got = snapshot(rt)
        assert s in seen_objects(rt)
        rt.set_transforms(away, s)
        assert rt.rays_info()["literal"] == 0
        got_away = snapshot(rt)
    assert differs(got, before) and differs(got_away, got)
    assert_same(got, fresh(("opencl", size, "onto"), R.with_transforms(objs, onto, s), lts, device_opencl=True), f"{size}: onto the light")
    assert_same(got_away, fresh(("opencl", size, "away"), R.with_transforms(objs, away, s), lts, device_opencl=True), f"{size}: away again")


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    objs = cloud().copy()
    objs["type"][150] = 7                         # an unknown type: never hit, and no record that holds two matrices
    good = transform(FRONT[0], None, (0.9, 0.9, 0.9))
    not_affine, singular, nan, outside, grazing = good.copy(), good.copy(), good.copy(), transform((0.0, 0.0, -400.0)), transform((0.0, 0.0, -0.5))
    not_affine["mv"][0][3] = 0.5
    singular["mvInverse"][0][:12] = 0.0
    nan["mvInverse"][0][5] = np.nan
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(8, dtype=R.TRANSFORM_DTYPE)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        lib, ctx = rt._lib, rt._ctx
        rt.set_transforms(good, 20)               # one dynamic object to begin with: the state a refusal must leave alone is not the empty one
        before, records, info, lt = snapshot(rt), rt.read_transforms(0, 150), rt.geometry_info(), rt.light_tiles_info()
        box = rt.rays_info()
        assert box["box_hi"][2] < 1.0 and box["box_lo"][2] > -60.0
        pair = np.concatenate([good, outside])    # a range whose SECOND record is refused: the first must not be touched either
        refused = [(lambda: lib.rt_set_transforms(ctx, None, 0, 3), -1), (lambda: lib.rt_set_transforms(ctx, ptr(good), N, 1), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(pair), N - 1, 2), -1), (lambda: lib.rt_set_transforms(ctx, ptr(good), 0xffffffff, 2), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(good), 2, 0xffffffff), -1), (lambda: lib.rt_set_transforms(ctx, ptr(good), N + 1, 0), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(good), 150, 1), -1), (lambda: lib.rt_set_transforms(ctx, ptr(not_affine), 30, 1), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(singular), 30, 1), -1), (lambda: lib.rt_set_transforms(ctx, ptr(nan), 30, 1), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(outside), 30, 1), -1), (lambda: lib.rt_set_transforms(ctx, ptr(grazing), 30, 1), -1),
                   (lambda: lib.rt_set_transforms(ctx, ptr(pair), 30, 2), -1),
                   (lambda: lib.rt_read_transforms(ctx, ptr(out), N - 7, 8), -1), (lambda: lib.rt_read_transforms(ctx, None, 0, 3), -1),
                   (lambda: lib.rt_read_transforms(ctx, ptr(out), 149, 2), -1)]

        def unchanged(label):
            assert same_records(rt.read_transforms(0, 150), records), label
            now, lt_now = rt.geometry_info(), rt.light_tiles_info()
            assert {k: v for k, v in now.items() if k != "patch_device_ms"} == {k: v for k, v in info.items() if k != "patch_device_ms"}, label
            assert all(np.array_equal(np.asarray(lt_now[k]), np.asarray(lt[k])) for k in lt if k != "build_device_ms"), label
            assert_same(snapshot(rt), before, label)

        for k, (call, code) in enumerate(refused):
            assert call() == code, k
            assert lib.rt_last_error(ctx)
            unchanged(f"after refusal {k}")
        assert not out.view(np.uint32).any()
        # count == 0 is RT_OK, launches nothing and changes nothing
        for call in (lambda: lib.rt_set_transforms(ctx, None, 0, 0), lambda: lib.rt_set_transforms(ctx, ptr(good), N, 0),
                     lambda: lib.rt_set_transforms(ctx, ptr(outside), 5, 0), lambda: lib.rt_read_transforms(ctx, None, 0, 0)):
            assert call() == 0
        rt.set_transforms(good[:0])
        unchanged("after empty calls")
        # an unaligned HOST array is fine
        raw = np.zeros(128 + 1, dtype=np.uint8)
        raw[1:] = np.frombuffer(good.tobytes(), dtype=np.uint8)
        assert lib.rt_set_transforms(ctx, ctypes.c_void_p(raw.ctypes.data + 1), 20, 1) == 0
        unchanged("the same transform again, from an odd address")
        # capacity: 63 more distinct objects fill the set, the 65th is RT_ERR_STATE
        fill = new_transforms(63, seed=51, centre=(0.0, 0.0, -36.0), spread=3.0)
        rt.set_transforms(fill, 60)
        full = rt.geometry_info()
        assert full["n_dynamic"] == 64 and full["dynamic_capacity"] == 64 and full["dynamic_ids"] == [20] + list(range(60, 123))
        before, records, info, lt = snapshot(rt), rt.read_transforms(0, 150), full, rt.light_tiles_info()
        assert lib.rt_set_transforms(ctx, ptr(good), 5, 1) == -5
        assert b"dynamic" in lib.rt_last_error(ctx)
        unchanged("after the capacity refusal")
        assert lib.rt_set_transforms(ctx, ptr(np.concatenate([good, good])), 122, 2) == -5   # one dynamic, one new: all or none
        unchanged("after the mixed capacity refusal")
        elsewhere = transform(FRONT[1], None, (0.9, 0.9, 0.9))
        rt.set_transforms(elsewhere, 100)         # a dynamic object may still move
        assert rt.geometry_info()["n_dynamic"] == 64
        got = snapshot(rt)
    expect = R.with_transforms(R.with_transforms(R.with_transforms(objs, good, 20), fill, 60), elsewhere, 100)
    assert differs(got, before)
    assert_same(got, fresh("refusals", expect), "a full dynamic set")
    with pytest.raises(ValueError):
        R.with_transforms(objs, good, N)          # the definition refuses the same range


def test_contexts_without_a_grid_have_no_cap():
    objs = cloud()
    xf = new_transforms(130, seed=61)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), grid=False) as rt:
        before = snapshot(rt)
        rt.set_transforms(xf, 40)
        got = snapshot(rt)
        assert rt.geometry_info() == dict(grid_built=0, n_unbounded=0, n_dynamic=0, dynamic_capacity=0, light_tiles_rebuilt=0, dynamic_ids=[],
                                          patch_device_ms=rt.geometry_info()["patch_device_ms"])
    assert differs(got, before)
    assert_same(got, fresh("no cap", R.with_transforms(objs, xf, 40), grid=False), "130 objects of a no-grid context")


# ---- 9. a context that never calls the setter ----------------------------------------------------------------------------------
def test_a_context_that_never_calls_the_setter():
    """(Fails on a library from before the feature only because rt_get_geometry_info is missing: nothing else here is new.)"""
    objs = cloud()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as a, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as b:
        tables = []
        for c in (a, b):
            c.Render()
            info = c.geometry_info()
            assert info["n_dynamic"] == 0 and info["n_unbounded"] == 0 and info["grid_built"] == 1 and info["light_tiles_rebuilt"] == 0
            lt = c.light_tiles_info()
            assert lt["enabled"] == 1 and lt["source"] == 1
            tables.append(c.read_light_tiles())
            assert same_records(c.read_transforms(), R.transforms_of(objs)) and same_records(c.read_materials(), live_words(objs))
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
