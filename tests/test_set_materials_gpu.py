"""GPU: replaceable materials (rt_set_materials, rt_set_materials_device, rt_set_materials_multi, rt_read_materials) - the patched
records read back against records.with_materials, and the frames against a FRESH context created with that object array, on
uint32 words, with rays_reference and hit_pixels.

1. the patch kernel's boundaries (four lanes per material: 16 per wave, 64 per 256-thread group); 2. both copies of the
absorption; 3. every kernel and path; 4. history does not matter; 5. with the other live-context calls; 6. the device form
behind a torch kernel on another stream; 7. NaN and infinite values; 8. refusals; 9. several contexts; 10. the CPU oracle.
Depth 2, 64 x 48 frames."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import R, compare_frames, load_fixture, random_scene, rotation
from opencl_raytracer_amd import ppm, rays as RY, sharding
from test_frame_shapes_cpu import camera_z_for, scene
from test_primary_depth_order_gpu import bits, hip
from test_set_lights_cpu import CENTRE, POSITIONS, SPREAD, inside_point, make_lights
from test_set_materials_cpu import live_words, new_materials

pytestmark = pytest.mark.gpu
DEPTH = 2
W, H, Z = 64, 48, -160.0
F = np.float32
N = 200
_FRESH = {}


@functools.lru_cache(maxsize=None)
def cloud(n=N):
    """n (200) mixed spheres and boxes around (0, 0, -40) +- 6: the large-scene path (96 objects and more)."""
    objs, _ = random_scene(130, 70, 1, seed=47, spread=SPREAD, zrange=(CENTRE[2] - SPREAD, CENTRE[2] + SPREAD))
    assert len(objs) == N
    return objs[:n].copy()


def small():
    """The first 40 objects: the small-scene kernel."""
    return cloud(40)


def lights():
    return make_lights(inside_point(), POSITIONS["+y"])


def snapshot(rt):
    frame = rt.Render()
    st = rt.count_rays()
    return dict(frame=frame, rays_ref=int(st.rays_reference), hits=int(st.hit_pixels), wavefront=int(st.wavefront))


def fresh(key, objs, lts=None, **kw):
    """Snapshot of a fresh context created with these objects; remembered per key."""
    if key not in _FRESH:
        kw.setdefault("camera", (W, H, Z))
        with hip(objs, lights() if lts is None else lts, None, DEPTH, **kw) as rt:
            _FRESH[key] = snapshot(rt)
    return _FRESH[key]


def assert_same(got, want, label):
    a, b = bits(got["frame"]).reshape(-1), bits(want["frame"]).reshape(-1)
    assert a.shape == b.shape and np.array_equal(a, b), f"{label}: frame differs on {int((a != b).sum())} words"
    assert got["rays_ref"] == want["rays_ref"] and got["hits"] == want["hits"], label


def same_records(a, b):
    return np.array_equal(np.frombuffer(a.tobytes(), dtype=np.uint32), np.frombuffer(b.tobytes(), dtype=np.uint32))


# ---- 1. kernel boundaries ------------------------------------------------------------------------------------------------------
COUNTS = (1, 15, 16, 17, 63, 64, 65)       # one material, a wave of 16 and a group of 64 materials, each -1 / +1
FIRSTS = (0, 1, 3, 17)


@pytest.mark.parametrize("n_objs", [N, N - 1])
def test_kernel_boundaries(n_objs):
    objs = cloud(n_objs)
    ranges = [(f, c) for c in COUNTS for f in FIRSTS]
    ranges += [(n_objs - c, c) for c in COUNTS]                  # ending on the last object
    ranges += [(n_objs // 2, 1), (0, n_objs), (n_objs - 1, 1)]   # one object in the middle, every object, the last one alone
    expect = objs.copy()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), kernel="hittest") as ht, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        times = ht.Render()
        assert np.isfinite(times).sum() and (times < R.MAX_FLOAT).mean() > 0.2
        assert same_records(rt.read_materials(), live_words(objs)) and same_records(ht.read_materials(), live_words(objs))
        for k, (first, count) in enumerate(ranges):
            mats = new_materials(count, seed=100 + k)
            expect = R.with_materials(expect, mats, first)
            for c in (ht, rt):
                c.set_materials(mats, first)
                got = c.read_materials()                          # the WHOLE array: the range replaced, every neighbour untouched
                assert same_records(got, live_words(expect)), (first, count, np.nonzero(got != live_words(expect))[0][:8])
            assert same_records(rt.read_materials(first, count), live_words(mats))
            assert np.array_equal(bits(ht.Render()), bits(times)), (first, count)   # types and matrices survived
        got = snapshot(rt)
    assert_same(got, fresh(("boundaries", n_objs), expect), f"{n_objs} objects after {len(ranges)} patches")


# ---- 2. both copies of the absorption ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_both_copies_of_the_absorption(size):
    objs = (cloud() if size == "large" else small()).copy()
    objs["absorption"] = np.where(np.arange(len(objs)) % 2 == 0, F(1.0), F(0.5))
    flipped = R.materials_of(objs)
    flipped["absorption"] = np.where(np.arange(len(objs)) % 2 == 0, F(0.5), F(1.0))
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before = snapshot(rt)
        assert before["wavefront"] == (1 if size == "large" else 0)   # the round machine reads ObjectRecord, the small-scene kernel ColdObject
        rt.set_materials(flipped)
        after = snapshot(rt)
        rt.set_materials(flipped[5:9], 5)    # a part again: nothing changes
        again = snapshot(rt)
        rt.set_materials(objs)               # ... and back, from the object array
        back = snapshot(rt)
    want = fresh(("absorption", size), R.with_materials(objs, flipped))
    assert after["rays_ref"] != before["rays_ref"] and after["hits"] == before["hits"]
    assert_same(after, want, f"{size}: flipped")
    assert_same(again, want, f"{size}: flipped twice")
    assert_same(back, before, f"{size}: back")


# ---- 3. every kernel and path --------------------------------------------------------------------------------------------------
PATHS = [(f"{kernel} {path}", dict(kernel=kernel, path=path)) for kernel in ("hittest", "shade", "shade_and_reflect") for path in ("monolithic", "wavefront")]
PATHS += [("literal", dict(literal=True)), ("no grid", dict(grid=False)), ("brute force", dict(grid=False, path="wavefront")), ("unfused", dict(fused=False)), ("device_opencl", dict(device_opencl=True)),
          ("fast phong", dict(fast_phong=True)), ("fast phong unfused", dict(fast_phong=True, fused=False))]


@pytest.mark.parametrize("label,kw", PATHS, ids=[p[0] for p in PATHS])
def test_every_kernel_and_path(label, kw):
    objs = cloud()
    first, mats = 37, new_materials(101, seed=9)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z), **kw) as rt:
        before = snapshot(rt)
        rt.set_materials(mats, first)
        got = snapshot(rt)
    if "path" in kw:
        assert got["wavefront"] == (1 if kw["path"] == "wavefront" else 0)
    want = fresh(("paths", label), R.with_materials(objs, mats, first), **kw)
    assert_same(got, want, label)
    if kw.get("kernel") == "hittest":
        assert_same(got, before, f"{label}: nothing visible changes")
    else:
        assert not np.array_equal(bits(got["frame"]), bits(before["frame"])), label


def test_small_scene_kernel():
    objs = small()
    mats = new_materials(23, seed=10)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        rt.set_materials(mats, 11)
        got = snapshot(rt)
    assert got["wavefront"] == 0
    assert_same(got, fresh("small", R.with_materials(objs, mats, 11)), "small scene")


def test_triangles():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    assert (objs["type"] == 2).all() and len(objs) > 400
    mats = new_materials(len(objs) - 50, seed=11)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        before = snapshot(rt)
        rt.set_materials(mats, 25)
        got = snapshot(rt)
        assert same_records(rt.read_materials(), live_words(R.with_materials(objs, mats, 25)))
    with hip(R.with_materials(objs, mats, 25), lts, None, DEPTH, camera=(W, H, z)) as rt:
        want = snapshot(rt)
    assert want["hits"] > 100 and not np.array_equal(bits(got["frame"]), bits(before["frame"]))
    assert_same(got, want, "triangles")


# ---- 4. history does not matter ------------------------------------------------------------------------------------------------
def test_history_does_not_matter():
    objs = cloud()
    X, Y = new_materials(N, seed=12), new_materials(60, seed=13)
    end = R.with_materials(R.with_materials(objs, X), Y, 70)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as a, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as b:
        constructor = snapshot(a)
        a.set_materials(X)                    # everything, then the range on top
        a.Render()
        a.set_materials(Y, 70)
        b.set_materials(Y[::-1].copy(), 70)   # the range first (wrong way round), then its neighbours, then the range again, rendering in between
        b.set_materials(X[130:], 130)
        b.Render()
        b.set_materials(X[:70], 0)
        b.set_materials(Y[:1], 70)
        b.set_materials(Y[1:], 71)
        got_a, got_b = snapshot(a), snapshot(b)
        assert same_records(a.read_materials(), live_words(end)) and same_records(b.read_materials(), live_words(end))
        a.set_materials(R.materials_of(objs))
        back = snapshot(a)
    want = fresh("history", end)
    assert_same(got_a, want, "sequence a")
    assert_same(got_b, want, "sequence b")
    assert_same(back, constructor, "the originals put back")
    assert not np.array_equal(bits(got_a["frame"]), bits(constructor["frame"]))


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
    first, mats = 20, new_materials(150, seed=14)
    changed = R.with_materials(objs, mats, first)
    originals = R.materials_of(objs)
    M, origin = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, 1.0)
    turned = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    far = RY.posed_rays(W, H, Z, np.eye(3), (0.0, 0.0, 500.0))   # origins off the grid's box: a brute-force frame
    d_rays = torch.from_numpy(turned.view(np.float32).reshape(-1, 8).copy()).cuda()
    other_lights = make_lights(POSITIONS["-x"], inside_point(), POSITIONS["+z"])
    acts = [("pose", lambda c: c.set_pose(W, H, Z, M, origin)), ("rays (numpy, off the box)", lambda c: c.set_rays(far)),
            ("rays (torch)", lambda c: c.set_rays(d_rays)), ("camera", lambda c: c.set_camera(H, W, -120.0)),
            ("lights", lambda c: c.set_lights(other_lights)), ("camera back", lambda c: c.set_camera(W, H, Z)),
            ("supersampling", lambda c: c.set_supersampling(2)), ("supersampling off", lambda c: c.set_supersampling(1)),
            ("shard", lambda c: c.set_shard(8 * W, 1, 2)), ("shard off", lambda c: c.set_shard(0, 0, 1))]
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as after, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as before, \
            hip(changed, lights(), None, DEPTH, camera=(W, H, Z)) as ref:
        after.set_materials(mats, first)          # `after`: the materials first, every other call behind them
        for label, act in acts:
            act(after), act(ref), act(before)     # `before`: the other call first, the materials behind it
            infos = [(before.rays_info(), before.tiles_info(), before.light_tiles_info())]
            before.set_materials(mats, first)
            infos.append((before.rays_info(), before.tiles_info(), before.light_tiles_info()))
            for x, y in zip(*infos):
                same_info(x, y, label)
            want = snapshot(ref)
            assert_same(snapshot(after), want, f"{label}, then materials")
            assert_same(snapshot(before), want, f"materials, then {label}")
            if label == "rays (numpy, off the box)":
                assert before.rays_info()["grid_in_use"] == 0
            before.set_materials(originals)
        want = ref.Render()
        for c in (after, before):
            c.set_materials(mats, first)
            assert np.array_equal(ppm.quantise_bytes(want), c.render_packed("rgba8"))
            pieces = []
            for rank in range(2):   # two shards of 8-row tiles, stitched
                c.set_shard(8 * W, rank, 2)
                pieces.append(c.Render())
            c.set_shard(0, 0, 1)
            assert np.array_equal(bits(sharding.assemble_frame(pieces, 8 * W, W * H)), bits(want))
        monkeypatch.setenv("RT_RENDER_PASSES", "3")
        assert np.array_equal(bits(after.Render()), bits(want))


# ---- 6. the device form --------------------------------------------------------------------------------------------------------
def test_device_form_behind_a_torch_kernel_on_another_stream():
    import torch
    from opencl_raytracer_amd.hip_raytracer import RTError
    objs = cloud()
    first, mats = 13, new_materials(170, seed=15)
    want = fresh("device form", R.with_materials(objs, mats, first))
    src = torch.from_numpy(mats.view(np.float32).reshape(-1, 16).copy()).cuda()
    d_mats = torch.zeros_like(src)
    work = torch.full((2048, 2048), 1.0 / 2048.0, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as dev, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as host:
        with torch.cuda.stream(side):
            for _ in range(8):               # the stream is busy for a while ...
                work = work @ work
            torch.mul(src, 1.0, out=d_mats)  # ... then a torch kernel fills the array (until then it holds zeros) ...
            dev.set_materials(d_mats, first) # ... immediately before the call, which is ordered behind it on that stream
        got = snapshot(dev)
        assert same_records(dev.read_materials(), live_words(R.with_materials(objs, mats, first)))
        host.set_materials(mats, first)
        assert_same(got, snapshot(host), "device form vs host form")
        assert_same(got, want, "device form vs fresh")
        # the legacy default stream, and a one-material array
        dev.set_materials(src[3:4].contiguous(), 0)
        assert same_records(dev.read_materials(0, 1), live_words(mats[3:4]))
        # a misaligned device pointer is refused and touches nothing
        flat = torch.zeros(16 * len(mats) + 4, dtype=torch.float32, device="cuda")
        records = dev.read_materials()
        for shift in (1, 2, 3):
            with pytest.raises(RTError) as err:
                dev.set_materials(flat[shift:shift + 16 * len(mats)], first)
            assert err.value.code == -1
        assert same_records(dev.read_materials(), records)
        with pytest.raises(ValueError):
            dev.set_materials(flat[:17])
        with pytest.raises(ValueError):
            dev.set_materials(flat[:32].double())


# ---- 7. non-finite values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["large", "small"])
def test_non_finite_values(size):
    objs = cloud() if size == "large" else small()
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        _, idx = rt.render_aux()
        seen = [int(i) for i in np.argsort(-np.bincount(idx[idx >= 0], minlength=len(objs)))[:3]]   # the three objects with most pixels
        cases = []
        for label, field, value, obj in (("NaN absorption", "absorption", np.nan, seen[0]), ("infinite shininess", "shininess", np.inf, seen[1]),
                                         ("NaN colour", "diffuse", np.nan, seen[2])):
            m = R.materials_of(objs[obj:obj + 1])
            if field == "diffuse":
                m[field][0, 1] = value
            else:
                m[field] = value
            cases.append((label, obj, m))
        for label, obj, m in cases:
            rt.set_materials(m, obj)
            got = snapshot(rt)
            assert same_records(rt.read_materials(obj, 1), live_words(m))
            assert_same(got, fresh(("non-finite", size, label), R.with_materials(objs, m, obj)), f"{size}: {label}")
            rt.set_materials(objs[obj:obj + 1], obj)
        # ... and all three at once
        expect = objs
        for _, obj, m in cases:
            rt.set_materials(m, obj)
            expect = R.with_materials(expect, m, obj)
        got = snapshot(rt)
    want = fresh(("non-finite", size, "all"), expect)
    assert_same(got, want, f"{size}: all three")
    assert np.isnan(got["frame"]).any()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    objs = cloud()
    mats = new_materials(8, seed=16)
    buf = np.ascontiguousarray(mats)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    d_buf = torch.from_numpy(mats.view(np.float32).reshape(-1, 16).copy()).cuda()
    d_ptr = ctypes.c_void_p(d_buf.data_ptr())
    out = np.zeros(8, dtype=R.MATERIAL_DTYPE)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        before, records = snapshot(rt), rt.read_materials()
        lib, ctx = rt._lib, rt._ctx
        refused = [lambda: lib.rt_set_materials(ctx, ptr, N - 7, 8), lambda: lib.rt_set_materials(ctx, ptr, N, 1),
                   lambda: lib.rt_set_materials(ctx, ptr, 0xffffffff, 2), lambda: lib.rt_set_materials(ctx, ptr, 2, 0xffffffff),
                   lambda: lib.rt_set_materials(ctx, None, 0, 3), lambda: lib.rt_set_materials(ctx, ptr, N + 1, 0),
                   lambda: lib.rt_set_materials_device(ctx, d_ptr, N - 7, 8, None), lambda: lib.rt_set_materials_device(ctx, d_ptr, 0xffffffff, 2, None),
                   lambda: lib.rt_set_materials_device(ctx, None, 0, 3, None),
                   lambda: lib.rt_set_materials_device(ctx, ctypes.c_void_p(d_buf.data_ptr() + 4), 0, 4, None),
                   lambda: lib.rt_read_materials(ctx, out.ctypes.data_as(ctypes.c_void_p), N - 7, 8),
                   lambda: lib.rt_read_materials(ctx, out.ctypes.data_as(ctypes.c_void_p), 0xffffffff, 2), lambda: lib.rt_read_materials(ctx, None, 0, 3)]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert rt._lib.rt_last_error(ctx)
            assert same_records(rt.read_materials(), records), k
            assert_same(snapshot(rt), before, f"after refusal {k}")
        assert not out.view(np.uint32).any()
        # count == 0 is RT_OK and changes nothing
        for call in (lambda: lib.rt_set_materials(ctx, None, 0, 0), lambda: lib.rt_set_materials(ctx, ptr, N, 0), lambda: lib.rt_set_materials(ctx, ptr, 5, 0),
                     lambda: lib.rt_set_materials_device(ctx, None, 0, 0, None), lambda: lib.rt_set_materials_device(ctx, d_ptr, N, 0, None),
                     lambda: lib.rt_read_materials(ctx, None, 0, 0)):
            assert call() == 0
        rt.set_materials(mats[:0])
        assert same_records(rt.read_materials(), records)
        assert_same(snapshot(rt), before, "after empty calls")
        with pytest.raises(ValueError):
            R.with_materials(objs, mats, N - 7)   # the definition refuses the same range
        # an unaligned HOST array is fine
        raw = np.zeros(64 * 8 + 1, dtype=np.uint8)
        raw[1:] = np.frombuffer(mats.tobytes(), dtype=np.uint8)
        assert lib.rt_set_materials(ctx, ctypes.c_void_p(raw.ctypes.data + 1), N - 8, 8) == 0
        assert same_records(rt.read_materials(N - 8, 8), live_words(mats))


# ---- 9. several contexts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_multi_set_materials_equals_the_single_frame(shards):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs = cloud()
    first, mats = 3, new_materials(190, seed=17)
    want = fresh("multi", R.with_materials(objs, mats, first))
    with MultiHIPRaytracer(objs, lights(), None, DEPTH, devices=(0,) * shards, camera=(W, H, Z)) as m:
        constructor = m.Render()
        m.set_materials(mats, first)
        got = m.Render()
        buf = np.ascontiguousarray(mats)
        assert m._lib.rt_set_materials_multi(m._m, buf.ctypes.data_as(ctypes.c_void_p), N - 1, 2) == -1   # refused before any shard is touched
        assert m._lib.rt_set_materials_multi(m._m, None, 0, 2) == -1
        assert np.array_equal(bits(m.Render()), bits(got))
        m.set_materials(objs)
        assert np.array_equal(bits(m.Render()), bits(constructor))
    assert np.array_equal(bits(got[:W * H]), bits(want["frame"]))
    assert not np.array_equal(bits(got), bits(constructor))


def test_two_contexts_do_not_see_each_others_materials():
    objs = cloud()
    mats = new_materials(N, seed=18)
    with hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as a, hip(objs, lights(), None, DEPTH, camera=(W, H, Z)) as b:
        constructor = snapshot(b)
        a.set_materials(mats)
        got_a, got_b = snapshot(a), snapshot(b)
        assert same_records(b.read_materials(), live_words(objs)) and same_records(a.read_materials(), live_words(mats))
    assert_same(got_b, constructor, "the other context")
    assert_same(got_a, fresh("two contexts", R.with_materials(objs, mats)), "the patched context")


# ---- 10. against the oracle ----------------------------------------------------------------------------------------------------
def test_against_the_cpu_oracle():
    from oracle import oracle
    fx = load_fixture("random_mixed100_shade_and_reflect")   # 100 objects: the large-scene path
    objs, lts, rays, depth = fx["objs"], fx["lights"], fx["rays"], fx["max_bounces"]
    first, mats = 10, new_materials(80, seed=19, absorption=(1.0, 0.9995, 0.999, 0.7, 0.4))
    changed = R.with_materials(objs, mats, first)
    want = oracle.Restatement(True).render("shade_and_reflect", changed, lts, rays, depth)
    with hip(objs, lts, rays, depth, path="wavefront") as rt:
        old = rt.Render()
        rt.set_materials(mats, first)
        out = rt.Render()
        t, idx = rt.render_aux()
        st = rt.count_rays()
    assert st.wavefront == 1
    assert np.array_equal(idx, want["hit_index"]), "primary hit index differs from the oracle"
    assert st.rays_reference == want["rays_ref"]
    err = compare_frames(out, want["out"])
    print(f"max |dRGB| against the oracle: {err:.3e}")
    assert err <= 1e-5, f"max |dRGB| = {err}"
    assert compare_frames(old, want["out"]) > 1e-2   # (the materials do change the picture)
