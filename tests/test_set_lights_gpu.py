"""GPU: replaceable lights (rt_set_lights) and the light tiles rebuilt on the device (csrc/rt_light_tiles.hip) - the table against
light_tiles.py, the frames against a fresh context created with the same lights and against brute force, bit for bit.

1. the table for six light positions; 2. frames in the three arithmetic modes, and with RT_LIGHT_TILES_DEVICE=0; 3. list lengths
on both sides of every limit (chain boundaries 3 / 4 and 6 / 7, wave sort / LDS sort 64 / 65, 1024 accepted / 1025 refused);
4. history does not matter; 5. with the other live-context calls; 6. the other kernels and paths; 7. device_opencl turning
literal and back; 8. large coordinates; 9. triangles; 10. refused arguments; 11. two contexts of one GPU.
Depth 2, 64 x 48 frames. Brute force is a fresh context with grid=False."""
import ctypes

import numpy as np
import pytest

from helpers import R, instance, rotation
from opencl_raytracer_amd import light_tiles as LT
from opencl_raytracer_amd import ppm, rays as RY, sharding
from test_frame_shapes_cpu import camera_z_for, scene
from test_primary_depth_order_gpu import MODES, bits, hip
from test_set_lights_cpu import CENTRE, LINE_LIGHT, POSITIONS, cloud, inside_point, lights_for, line_scene, line_tile_lengths, make_lights

pytestmark = pytest.mark.gpu
DEPTH = 2
W, H, Z = 64, 48, -160.0
F = np.float32
_FRESH = {}


def snapshot(rt):
    frame = rt.Render()
    st = rt.count_rays()
    return dict(frame=frame, rays_ref=int(st.rays_reference), hits=int(st.hit_pixels), literal=int(rt.rays_info()["literal"]),
                wavefront=int(st.wavefront), tests=int(st.object_tests))


def fresh(key, objs, lts, **kw):
    """Snapshot (and light-tile info) of a fresh context created with these lights; remembered per key."""
    if key not in _FRESH:
        kw.setdefault("camera", (W, H, Z))
        with hip(objs, lts, None, DEPTH, **kw) as rt:
            snap = snapshot(rt)
            snap["info"] = rt.light_tiles_info()
        _FRESH[key] = snap
    return _FRESH[key]


def assert_same(got, want, label, literal=True):
    assert np.array_equal(bits(got["frame"]), bits(want["frame"])), f"{label}: frame differs on {int((bits(got['frame']) != bits(want['frame'])).sum())} words"
    assert got["rays_ref"] == want["rays_ref"] and got["hits"] == want["hits"], label
    if literal:
        assert got["literal"] == want["literal"], label


def start_lights():
    return make_lights(inside_point(), (5.0, 30.0, -10.0))


# ---- 1. the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(POSITIONS))
def test_table_lies_between_must_and_may(name):
    objs = cloud()
    with hip(objs, start_lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        assert rt.light_tiles_info()["source"] == 1   # never called rt_set_lights: rt_create's table
        rt.set_lights(lights_for(name))
        info = rt.light_tiles_info()
        start, entries = rt.read_light_tiles()
        spheres, pre = rt.grid_spheres(), rt.grid_pretest()
        rt.set_lights(lights_for(name))
        info2 = rt.light_tiles_info()
        start2, entries2 = rt.read_light_tiles()
    assert info["enabled"] == 1 and info["source"] == 2 and info["refused"] == 0 and info["light"] == 1
    assert info["axis"] == "xyz".index(name[1]) and info["sign"] == (1 if name[0] == "-" else -1)
    T = info["tiles_u"]
    assert info["tiles_v"] == T and len(start) == T * T + 1 and int(start[-1]) == info["n_entries"] == len(entries)
    lens = np.diff(start).astype(np.int64)
    assert info["n_blocks"] == T * T + int(np.where(lens > 3, (lens - 1) // 3, 0).sum())
    assert info["max_list"] == int(np.diff(start).max()) and info["build_device_ms"] > 0
    # two builds, the same bytes
    assert np.array_equal(start, start2) and np.array_equal(entries, entries2)
    assert {k: v for k, v in info.items() if k not in ("build_device_ms", "lat_lo")} == {k: v for k, v in info2.items() if k not in ("build_device_ms", "lat_lo")}

    k = LT.light_constants(spheres, POSITIONS[name])
    assert k["axis"] == info["axis"] and k["sign"] == info["sign"]
    assert abs(info["k_pad"] - k["k_pad"]) <= 1e-12 * k["k_pad"] and abs(info["cut_pad"] - k["cut_pad"]) <= 1e-12 * k["cut_pad"]
    rc = LT.rectangles(spheres, k, info["u0"], info["v0"], info["inv_du"], info["inv_dv"], T)
    n = len(objs)
    member = np.zeros((n, T * T), dtype=bool)
    tile_of_entry = np.repeat(np.arange(T * T), np.diff(start).astype(np.int64))
    member[entries[:, 0].astype(np.int64), tile_of_entry] = True
    cols, rows = np.arange(T * T) % T, np.arange(T * T) // T
    for i in range(n):
        assert rc["listed"][i] == member[i].any(), i
        if not rc["listed"][i]:
            continue
        a0, a1, b0, b1 = rc["must"][i]
        must = (cols >= a0) & (cols <= a1) & (rows >= b0) & (rows <= b1)
        a0, a1, b0, b1 = rc["may"][i]
        may = (cols >= a0) & (cols <= a1) & (rows >= b0) & (rows <= b1)
        assert not (must & ~member[i]).any(), f"object {i}: a MUST tile is missing"
        assert not (member[i] & ~may).any(), f"object {i}: a tile outside MAY"
    # T is the rule's for some pair total between the MUST and the MAY totals
    b = LT.spans(spheres, k, 1e-5)
    on = b["listed"] & b["ok"]
    bounds = (b["u0"][on].min(), b["u1"][on].max(), b["v0"][on].min(), b["v1"][on].max())

    def total_of(kind):
        def f(Tc):
            r = LT.rectangles(spheres, k, *LT.tile_frame(*bounds, Tc), Tc)
            return LT.pair_total(r[kind], r["listed"])
        return f
    assert LT.tile_rule(n, total_of("may")) <= T <= LT.tile_rule(n, total_of("must"))
    assert LT.pair_total(rc["must"], rc["listed"]) <= info["n_entries"] <= LT.pair_total(rc["may"], rc["listed"])

    # the entries: order, keys, radii, centres
    key = LT.keys(spheres, k)
    dec = LT.unpack_entries(entries, info)
    idx = dec["index"]
    for t in range(T * T):
        lst = idx[start[t]:start[t + 1]]
        ks = [(float(key[i]), int(i)) for i in lst]
        assert ks == sorted(ks), f"tile {t}"
    kstep, rstep = float(info["kstep"]), float(info["rstep"])
    assert np.all(dec["key"].astype(np.float64) <= key[idx].astype(np.float64))
    assert np.all(dec["key"].astype(np.float64) >= key[idx].astype(np.float64) - kstep)
    wq = LT.block_radius(spheres, pre, info["lat_lo"], info["lat_step"], info["pretest_alpha"], info["box_diagonal"])
    assert np.all(dec["radius"].astype(np.float64) >= wq[idx]) and np.all(dec["radius"].astype(np.float64) <= wq[idx] + rstep)
    off = np.sqrt(((dec["centre"].astype(np.float64) - spheres[idx, :3]) ** 2).sum(axis=1))
    assert np.all(off <= np.sqrt(3.0) / 2.0 * float(info["lat_step"]) * (1.0 + 1e-6))


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_frames_equal_fresh_and_brute_force(mode, monkeypatch):
    objs = cloud()
    with hip(objs, start_lights(), None, DEPTH, camera=(W, H, Z), **MODES[mode]) as rt:
        for name in sorted(POSITIONS):
            lts = lights_for(name)
            rt.set_lights(lts)
            got = snapshot(rt)
            info = rt.light_tiles_info()
            assert info["enabled"] == 1 and info["source"] == 2, (mode, name, info)
            want = fresh(("cloud", mode, name), objs, lts, **MODES[mode])
            brute = fresh(("cloud brute", mode, name), objs, lts, grid=False, path="wavefront", **MODES[mode])
            assert want["info"]["enabled"] == 1 and want["info"]["source"] == 1 and got["literal"] == 0
            assert_same(got, want, f"{mode} {name} vs fresh")
            assert_same(got, brute, f"{mode} {name} vs brute force")
            assert got["tests"] < brute["tests"]
        # the knob: nothing is built, the grid walk serves the last light, same bits
        monkeypatch.setenv("RT_LIGHT_TILES_DEVICE", "0")
        rt.set_lights(lights_for("+y"))
        info = rt.light_tiles_info()
        assert info["enabled"] == 0 and info["source"] == 0 and info["refused"] == LT.REFUSED_KNOB
        assert_same(snapshot(rt), fresh(("cloud", mode, "+y"), objs, lights_for("+y"), **MODES[mode]), f"{mode} knob")


# ---- 3. list lengths on both sides of every limit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 6, 7, 64, 65, 1024, 1025])
def test_list_lengths_around_the_limits(n):
    objs = line_scene(n, LINE_LIGHT)
    lts = make_lights((-4.0, 5.0, -33.0), LINE_LIGHT)
    with hip(objs, make_lights((0.0, 9.0, -20.0)), None, DEPTH, camera=(W, H, Z), path="wavefront") as rt:
        must, may, refused = line_tile_lengths(objs, LINE_LIGHT, rt.grid_spheres())
        assert must == may == n   # (the line-up is what this case needs, by the definition, on the context's own spheres)
        rt.set_lights(lts)
        info = rt.light_tiles_info()
        got = snapshot(rt)
        if n <= 1024:
            assert info["enabled"] == 1 and info["source"] == 2 and info["max_list"] == n, info
            start, entries = rt.read_light_tiles()
            assert int(np.diff(start).max()) == n
        else:
            assert info["enabled"] == 0 and info["refused"] == LT.REFUSED_LIST and info["max_list"] == n, info
    assert_same(got, fresh(("line brute", n), objs, lts, grid=False, path="wavefront"), f"line {n}")


# ---- 4. history does not matter ------------------------------------------------------------------------------------------------
def test_history_does_not_matter():
    objs = cloud()
    A = lights_for("-z")
    steps = [("A", A), ("inside", make_lights(POSITIONS["+x"], tuple(CENTRE))), ("directional", make_lights(inside_point(), (0.3, 1.0, 0.2, 0.0))),
             ("none", make_lights()), ("five", make_lights(inside_point(), POSITIONS["-x"], (0.0, 1.0, 0.5, 0.0), POSITIONS["+z"], POSITIONS["-y"])),
             ("A", A)]
    expect = {"A": (1, 0), "inside": (0, LT.REFUSED_PLANE), "directional": (0, LT.REFUSED_LIGHT), "none": (0, LT.REFUSED_NO_GRID), "five": (1, 0)}
    frames = []
    with hip(objs, start_lights(), None, DEPTH, camera=(W, H, Z)) as rt:
        for label, lts in steps:
            rt.set_lights(lts)
            got, info = snapshot(rt), rt.light_tiles_info()
            want = fresh(("history", label), objs, lts)
            assert_same(got, want, label)
            for f in ("enabled", "refused", "light", "axis", "sign"):
                assert info[f] == want["info"][f], (label, f, info, want["info"])
            assert (info["enabled"], info["refused"]) == expect[label], (label, info)
            frames.append(got["frame"])
    assert np.array_equal(bits(frames[0]), bits(frames[-1]))
    assert not np.array_equal(bits(frames[0]), bits(frames[1]))


# ---- 5. with the other live-context calls --------------------------------------------------------------------------------------
def test_with_the_other_live_context_calls(monkeypatch):
    for knob in ("RT_RENDER_PASSES", "RT_RENDER_SPLIT"):
        monkeypatch.delenv(knob, raising=False)
    objs, lts = cloud(), lights_for("+x")
    M, origin = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, 1.0)
    far = RY.posed_rays(W, H, Z, np.eye(3), (0.0, 0.0, 500.0))   # origins off the grid's box: a brute-force frame
    with hip(objs, start_lights(), None, DEPTH, camera=(W, H, Z)) as rt, hip(objs, lts, None, DEPTH, camera=(W, H, Z)) as ref:
        rt.set_lights(lts)
        assert rt.light_tiles_info()["source"] == 2 and ref.light_tiles_info()["source"] == 1
        for label, act in (("pose", lambda c: c.set_pose(W, H, Z, M, origin)), ("rays off the box", lambda c: c.set_rays(far)),
                           ("camera", lambda c: c.set_camera(H, W, -120.0))):
            act(rt), act(ref)
            assert_same(snapshot(rt), snapshot(ref), label)
            if label == "rays off the box":
                assert rt.rays_info()["grid_in_use"] == 0
        rt.set_camera(W, H, Z), ref.set_camera(W, H, Z)
        want = ref.Render()
        assert np.array_equal(ppm.quantise_bytes(want), rt.render_packed("rgba8"))
        pieces = []
        for rank in range(2):   # two shards of 8-row tiles, stitched
            rt.set_shard(8 * W, rank, 2)
            pieces.append(rt.Render())
        rt.set_shard(0, 0, 1)
        assert np.array_equal(bits(sharding.assemble_frame(pieces, 8 * W, W * H)), bits(want))
        monkeypatch.setenv("RT_RENDER_PASSES", "3")
        assert np.array_equal(bits(rt.Render()), bits(want))
    with hip(objs, start_lights(), None, DEPTH, camera=(W // 2, H // 2, Z / 2), supersample=2) as rt:
        rt.set_lights(lts)
        got = rt.Render()
    with hip(objs, lts, None, DEPTH, camera=(W // 2, H // 2, Z / 2), supersample=2) as ref:
        assert np.array_equal(bits(got), bits(ref.Render()))


# ---- 6. the other kernels and paths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,kw", [("hittest", dict(kernel="hittest")), ("shade", dict(kernel="shade")), ("literal", dict(literal=True)),
                                      ("no grid", dict(grid=False)), ("small scene", dict())])
def test_other_kernels_and_paths(label, kw):
    objs = cloud()[:10] if label == "small scene" else cloud()
    lts = lights_for("-x")
    with hip(objs, start_lights(), None, DEPTH, camera=(W, H, Z), **kw) as rt:
        rt.set_lights(lts)
        got, info = snapshot(rt), rt.light_tiles_info()
    assert info["enabled"] == 0 and info["source"] == 0 and info["refused"] == LT.REFUSED_NO_GRID
    if label == "small scene":
        assert got["wavefront"] == 0
    got2 = dict(got, frame=got["frame"].reshape(-1))
    want = fresh(("paths", label), objs, lts, **kw)
    assert_same(got2, dict(want, frame=want["frame"].reshape(-1)), label)


# ---- 7. device_opencl ----------------------------------------------------------------------------------------------------------
def test_device_opencl_turns_literal_and_back():
    objs = cloud()
    centre = objs["mv"][0].reshape(4, 4)[3, :3].astype(np.float64)   # (column-major: the translation)
    on_surface = make_lights(inside_point(), tuple(centre))           # inside object 0's bound: a light "on an object"
    away = lights_for("+z")
    with hip(objs, away, None, DEPTH, camera=(W, H, Z), device_opencl=True) as rt:
        assert rt.rays_info()["literal"] == 0
        for label, lts, literal in (("on", on_surface, 1), ("away", away, 0), ("on", on_surface, 1), ("away", away, 0)):
            rt.set_lights(lts)
            got = snapshot(rt)
            assert got["literal"] == literal, label
            assert rt.light_tiles_info()["enabled"] == (0 if literal else 1)
            assert_same(got, fresh(("opencl", label), objs, lts, device_opencl=True), label)


# ---- 8. scale of coordinates ---------------------------------------------------------------------------------------------------
def test_large_coordinates_and_a_far_light():
    rng = np.random.default_rng(811)
    centre = np.array([3000.0, -2000.0, -7000.0])
    objs = []
    for k in range(300):
        pos = centre + rng.uniform(-60, 60, 3)
        mv, inv = instance(pos, rotation(rng.normal(size=3), rng.uniform(0, 6)), np.full(3, rng.uniform(3.0, 9.0)))
        mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                         absorption=float(rng.choice([1.0, 0.5])), reflection=0.0, shininess=float(rng.choice([1.0, 12.0])))
        objs.append(R.make_object(R.BOX if k % 9 == 0 else R.SPHERE, mat, mv, inv))
    objs = R.objects_array(objs)
    lts = make_lights(tuple(centre + rng.uniform(-20, 20, 3)), tuple(centre + np.array([9000.0, 14000.0, 11000.0])))
    d0 = centre / np.linalg.norm(centre)
    ex = np.cross(d0, (0.0, 1.0, 0.0)); ex /= np.linalg.norm(ex)
    ey = np.cross(ex, d0)
    rays = np.zeros(W * H, dtype=R.RAY_DTYPE)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs = d0[None, :] + ((ii.ravel() - W / 2) / (W / 2) * 0.0085)[:, None] * ex[None, :] + ((jj.ravel() - H / 2) / (H / 2) * 0.0065)[:, None] * ey[None, :]
    rays["start"] = np.array([0, 0, 0, 1], dtype=F)
    rays["direction"][:, :3] = dirs.astype(F)
    with hip(objs, make_lights(tuple(centre)), rays, DEPTH, raygen=False) as rt:
        rt.set_lights(lts)
        info, got = rt.light_tiles_info(), snapshot(rt)
    assert info["enabled"] == 1 and info["source"] == 2 and info["k_pad"] > 1e-3
    with hip(objs, lts, rays, DEPTH, raygen=False, grid=False, path="wavefront") as rt:
        want = snapshot(rt)
    assert want["hits"] > 200
    assert_same(got, want, "far cloud")


# ---- 9. triangles --------------------------------------------------------------------------------------------------------------
def test_triangles_equal_a_fresh_context():
    objs, lts = scene("tri")
    z = camera_z_for("tri", W, H)
    moved = lts.copy()
    moved["position"][-1][:3] += (2.0, 3.0, 1.0)
    with hip(objs, lts, None, DEPTH, camera=(W, H, z)) as rt:
        first = rt.light_tiles_info()
        rt.set_lights(moved)
        got, info = snapshot(rt), rt.light_tiles_info()
    with hip(objs, moved, None, DEPTH, camera=(W, H, z)) as rt:
        want, winfo = snapshot(rt), rt.light_tiles_info()
    assert first["source"] == 1 and winfo["source"] == 1 and winfo["enabled"] == 1   # the fresh context has a host-built table
    assert info["enabled"] == 1 and info["source"] == 2
    assert_same(got, want, "triangles")


# ---- 10. refused arguments -----------------------------------------------------------------------------------------------------
def test_refused_arguments_change_nothing():
    objs, lts = cloud(), lights_for("-y")
    with hip(objs, lts, None, DEPTH, camera=(W, H, Z)) as rt:
        before, info = snapshot(rt), rt.light_tiles_info()
        buf = np.ascontiguousarray(lts)
        assert rt._lib.rt_set_lights(rt._ctx, None, 3) == -1
        assert rt._lib.rt_set_lights(rt._ctx, buf.ctypes.data_as(ctypes.c_void_p), 1 << 22) == -1
        assert_same(snapshot(rt), before, "after refused calls")
        after = rt.light_tiles_info()
        assert {k: v for k, v in after.items() if k != "lat_lo"} == {k: v for k, v in info.items() if k != "lat_lo"}
        assert rt._lib.rt_set_lights(rt._ctx, None, 0) == 0   # zero lights are allowed


# ---- 11. several contexts of one GPU -------------------------------------------------------------------------------------------
def test_multi_set_lights_equals_the_single_frame():
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    objs, lts = cloud(), lights_for("+z")
    want = fresh(("cloud", "fused", "+z"), objs, lts)
    with MultiHIPRaytracer(objs, start_lights(), None, DEPTH, devices=(0, 0), camera=(W, H, Z)) as m:
        m.set_lights(lts)
        got = m.Render()
        assert m._lib.rt_set_lights_multi(m._m, None, 2) == -1
        assert np.array_equal(bits(m.Render()), bits(got))
    assert np.array_equal(bits(got[:W * H]), bits(want["frame"]))
