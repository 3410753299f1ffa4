"""GPU: a posed camera whose origin lies OUTSIDE the grid's box keeps the grid (hip_raytracer.h, "outside the box"): registration
spheres made for the pose's own origin on the device (csrc/rt_tiles.hip: pose_spheres), the pose's screen tiles built from them, a
primary round that never enters the grid walk (rt_wavefront.hip: wf_trace_primary_tiles<AM, true>), the grid for every later ray.

Two seeded scenes, clouds in front of the world's origin (the create-time camera's eye, a corner of the grid's box) - 300 objects,
the count of the scene the pose tests render on the default path (s300): from 96 to 511 objects the round machine is the default
only while the grid serves the frame, so the path choice itself is under test; small objects (scales 0.4 .. 0.8 in a cloud 12 wide),
so that at 128 x 64 a rectangle covers about 2.5 of the 16 tiles - and 2 000, so that lists have depth - under shade_and_reflect,
depth 3, with two positional lights (the last one's shadow rays go through the light tiles). Frames of 128 x 64 and 192 x 64. Poses: 1.5 and 4 box
diagonals outside each of three faces, looking at the box's centre (z lets the box span the frame's longer side: the scene fills the
frame), and one looking away from the scene.
(Why not 96 objects, the threshold itself: check 2 asks for fewer than n_objs / 10 object tests per ray. A ray of the grid walk
tests 6 to 8 objects whatever the scene's size, and a primary ray of a 128 x 64 frame walks one of only 16 tile lists - k / 16 of the
objects for rectangles of k tiles; at 96 objects a tenth is 9.6 tests per ray, which the grid walk alone costs.) Every frame is compared bit for bit - frame, primary t and index,
rays_reference, hit_pixels - against two FRESH contexts: one created with rays.posed_rays(...) under RT_FLAG_NO_RAYGEN (its grid is
built around its own origin) and one created with RT_FLAG_NO_GRID.

1. rays_info / tiles_info report the route (grid_in_use 1, primary_outside_box 1, source 3);   2. object_tests is below a tenth of
n_objs * rays_traced;   3. frame identity, also under device_opencl;   4. read_pose_spheres against tiles.pose_registration_spheres
(1e-12 relative: host and device double need not agree to the last bit);   5. read_tiles lists every primary hit with a key <= t;
6. waves that straddle tiles - shards of 96 rays, supersampling - take the brute-force branch: same frames;   7. refusals (W = 96,
a frame of fewer than 16 tiles, RT_POSE_TILES=0 in a child process, an origin at 1e9) leave the frame with RT_FLAG_NO_GRID's route, same pixels;   8. history does
not matter;   9. nor do rt_set_transforms and rt_set_lights."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import R, ROOT, instance, random_scene, rotation
from opencl_raytracer_amd import camera, rays as RY, resolve
from test_context_lifecycle_gpu import clean_env
from test_frame_shapes_gpu import same_bits, stitched
from test_pose_tiles_cpu import assert_hits_are_listed, assert_lists_ascend
from test_pose_tiles_gpu import boundary_slack
from test_primary_depth_order_gpu import bits, hip

pytestmark = pytest.mark.gpu
DEPTH = 3
KERNEL = "shade_and_reflect"
SHAPES = ((128, 64), (192, 64))
SCENE_NAMES = ("n300", "n2000")
MODES = {"fused": {}, "device_opencl": dict(device_opencl=True)}
REFUSED_FAR = 0x400
REFUSED_SMALL = 0x800


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "n300":
        _, lts = random_scene(2, 2, 2, seed=41)
        rng = np.random.default_rng(41)
        recs = []
        for k in range(300):   # 200 spheres and 100 boxes, scales 0.4 .. 0.8, in 12 x 12 x 12 from z = -16 to -4
            mv, inv = instance((rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-16, -4)), rotation(rng.normal(size=3), rng.uniform(0, 6.28)),
                               rng.uniform(0.4, 0.8, size=3))
            a = float(rng.choice([0.9, 0.7, 0.5, 0.3]))
            mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3), absorption=a,
                             reflection=1 - a, shininess=5.0)
            recs.append(R.make_object(R.SPHERE if k % 3 else R.BOX, mat, mv, inv))
        return R.objects_array(recs), lts
    return random_scene(1300, 700, 2, seed=43, spread=14.0, zrange=(-32.0, -4.0))


@functools.lru_cache(maxsize=None)
def box_of(name):
    """(box_lo, box_hi, diagonal) of the grid a camera context builds for the scene."""
    objs, lts = scene(name)
    with hip(objs, lts, None, DEPTH, camera=(64, 64, -64.0), kernel=KERNEL) as rt:
        info = rt.rays_info()
        assert (info["grid_built"], info["grid_in_use"]) == (1, 1)
        return info["box_lo"].copy(), info["box_hi"].copy(), float(np.linalg.norm(info["box_hi"] - info["box_lo"]))


POSE_NAMES = tuple(f"{face} {d}" for face in ("x.hi", "y.lo", "z.hi") for d in ("1.5", "4")) + ("away",)


def pose(name, which, W, H=64):
    """(z, M, origin): outside a face by 1.5 or 4 diagonals, a little off the face's centre, looking at the box's centre with a z
    that lets the box's circumscribed sphere span the frame's longer side - the scene fills the frame, as for a viewer that orbits
    it; "away": from 1.5 diagonals outside x.hi, looking along +x - nothing there."""
    lo, hi, diag = box_of(name)
    centre = (lo + hi) / 2.0
    face, d = ("x.hi", "1.5") if which == "away" else which.split(" ")
    axis, side = "xyz".index(face[0]), face[2:]
    o = centre + np.array([0.07, -0.05, 0.06]) * diag
    o[axis] = hi[axis] + float(d) * diag if side == "hi" else lo[axis] - float(d) * diag
    o = o.astype(np.float32)
    target = centre if which != "away" else o.astype(np.float64) + np.array([1.0, 0.0, 0.0])
    z = float(np.float32(-0.5 * max(W, H) * np.linalg.norm(o - centre) / (0.5 * diag)))
    return z, camera.look_at(o, target), o


def snapshot(rt):
    frame = rt.Render()
    t, idx = rt.render_aux()
    st = rt.count_rays()
    return dict(frame=frame, t=t, idx=idx, rays_ref=int(st.rays_reference), hits=int(st.hit_pixels), tests=int(st.object_tests),
                traced=int(st.rays_traced), wavefront=int(st.wavefront))


_FRESH = {}


def fresh(objs, lts, W, H, z, M, o, key=None, **flags):
    """The two fresh contexts of one pose: created with its rays (NO_RAYGEN, grid around its own origin) and with NO_GRID."""
    if key is not None and key in _FRESH:
        return _FRESH[key]
    rays = RY.posed_rays(W, H, z, M, o)
    with hip(objs, lts, rays, DEPTH, kernel=KERNEL, raygen=False, **flags) as rt:
        own = snapshot(rt)
    with hip(objs, lts, rays, DEPTH, kernel=KERNEL, raygen=False, grid=False, **flags) as rt:
        brute = snapshot(rt)
    if key is not None:
        _FRESH[key] = (own, brute)
    return own, brute


def assert_same(got, want, label):
    for k in ("frame", "t", "idx"):
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{label}: {k} differs on {int((a != b).sum())} words"
    assert (got["rays_ref"], got["hits"]) == (want["rays_ref"], want["hits"]), f"{label}: rays_reference / hit_pixels differ"


def assert_both(got, pair, label):
    assert_same(got, pair[0], f"{label}: against the fresh context created with the pose's rays")
    assert_same(got, pair[1], f"{label}: against the fresh RT_FLAG_NO_GRID context")


def live(objs, lts, W, H, **flags):
    return hip(objs, lts, None, DEPTH, camera=(W, H, -float(W)), kernel=KERNEL, **flags)


def assert_outside_route(rt, label):
    info, ti = rt.rays_info(), rt.tiles_info()
    assert (info["source"], info["grid_built"], info["grid_in_use"], info["primary_outside_box"], info["literal"]) == (3, 1, 1, 1, 0), f"{label}: {info}"
    assert (ti["enabled"], ti["source"], ti["refused"], ti["col_shift"]) == (1, 3, 0, 6), f"{label}: {ti}"
    return ti


# ---- 1 - 5: the route, the counts, the frames, the spheres, the table -----------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", POSE_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_pose_outside_the_box_keeps_the_grid(name, shape, which, mode, monkeypatch):
    from opencl_raytracer_amd import tiles
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene(name)
    W, H = shape
    z, M, o = pose(name, which, W)
    label = f"{name} {W}x{H} {which} {mode}"
    want = fresh(objs, lts, W, H, z, M, o, key=(name, shape, which, mode), **MODES[mode])
    with live(objs, lts, W, H, **MODES[mode]) as rt:
        rt.set_pose(W, H, z, M, o)
        info = rt.rays_info()
        assert bool(((o < info["box_lo"]) | (o > info["box_hi"])).any()), f"{label}: the origin is inside the box"
        ti = assert_outside_route(rt, label)
        got = snapshot(rt)
        assert_both(got, want, label)
        assert got["wavefront"] == 1, label
        share = got["tests"] / (len(objs) * got["traced"])
        print(f"\n[pose offbox] {label}: hit share {(got['idx'] >= 0).mean():.3f}, object_tests / (n_objs rays_traced) = {share:.4f}, "
              f"pairs {ti['n_entries']}, global {ti['n_global']}, longest list {ti['max_list']}, build {ti['build_device_ms']:.3f} ms")
        # 2. (a primary ray walks its tile's list, k / T of the objects for rectangles of k tiles; the rest of the frame's rays are served
        # by the grid with a handful of tests each)
        bound = 0.1
        assert got["tests"] < bound * len(objs) * got["traced"], f"{label}: {got['tests']} object tests for {got['traced']} rays - did every ray test every object?"
        if which == "away":
            assert (got["idx"] >= 0).sum() == 0, "the pose looking away sees nothing"
        elif which.endswith("1.5"):
            assert (got["idx"] >= 0).mean() > 0.05, f"{label}: the pose sees too little"
        if mode != "fused":
            return
        # 4. the spheres
        g, b, base = rt.grid_constants(), rt.object_bounds(), rt.grid_spheres()
        spheres = rt.read_pose_spheres()
        expect = tiles.pose_registration_spheres(b, g, o, grid_spheres=base)
        assert np.array_equal(spheres[:, :3], base[:, :3])
        finite = np.isfinite(expect[:, 3])
        assert np.array_equal(spheres[~finite, 3], expect[~finite, 3])
        assert np.all(np.abs(spheres[finite, 3] - expect[finite, 3]) <= 1e-12 * np.abs(expect[finite, 3])), f"{label}: the device's spheres are not the definition's"
        listed = (base[:, 3] >= 0) & np.isfinite(base[:, 3])
        assert np.all(spheres[listed, 3] >= base[listed, 3]), "a per-pose sphere is never smaller than the grid's"
        inside = tiles.pose_registration_spheres(b, g, (0.0, 0.0, 0.0), grid_spheres=base)
        assert inside.tobytes() == base.tobytes(), "the definition with an origin inside the box is the context's spheres, bit for bit"
        # 5. the table
        start, entries = rt.read_tiles()
        assert int(start[-1]) == ti["n_entries"] and len(entries) == ti["n_entries"] + ti["n_global"]
        assert_lists_ascend(start, entries, ti["n_entries"], label)
        table = dict(tiles_x=ti["tiles_x"], tiles_y=ti["tiles_y"], col_shift=ti["col_shift"], tile_start=start, entries=entries,
                     n_entries=ti["n_entries"], n_global=ti["n_global"], global_begin=ti["n_entries"], always=np.nonzero(np.isposinf(base[:, 3]))[0])
        assert_hits_are_listed(table, len(objs), W, H, got["idx"], got["t"], label)
        definition = tiles.pose_screen_tiles(expect, W, H, z, M, o, whole_r=0.25 * g["diag"])
        slack = boundary_slack(definition["rects"], W, H)   # pairs whose rectangle has an edge within 1e-6 of a tile boundary
        assert definition["enabled"] and abs(definition["n_entries"] - ti["n_entries"]) <= slack and definition["n_global"] == ti["n_global"], \
            f"{label}: the definition lists {definition['n_entries']} pairs (+- {slack}), the device {ti['n_entries']}"


# ---- 6. straddling waves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", POSE_NAMES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_waves_that_straddle_tiles_test_every_object(name, which, monkeypatch):
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene(name)
    W, H = 128, 64
    n = W * H
    z, M, o = pose(name, which, W)
    want = fresh(objs, lts, W, H, z, M, o, key=(name, (W, H), which, "fused"))
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, z, M, o)
        whole = snapshot(rt)
        assert_both(whole, want, f"{name} {which}")
        pieces, ts, idxs, tests = [], [], [], 0
        for rank in range(2):   # tiles of 96 rays: every second wave holds pixels of two screen tiles
            rt.set_shard(96, rank, 2)
            assert_outside_route(rt, f"{name} {which} rank {rank}")
            pieces.append(rt.Render())
            t, idx = rt.render_aux()
            ts.append(t)
            idxs.append(idx)
            tests += int(rt.count_rays().object_tests)
        assert same_bits(stitched(pieces, 96, n), want[1]["frame"]), f"{name} {which}: the stitched frame of 96-ray shards"
        assert same_bits(stitched(ts, 96, n), want[1]["t"]) and np.array_equal(stitched(idxs, 96, n), want[1]["idx"])
        assert tests > whole["tests"], "the shards' straddling waves tested more objects than the whole frame's: the brute-force branch ran"
        rt.set_shard(0, 0, 1)
        rt.set_supersampling(2)   # 128 x 64 samples -> 64 x 32 pixels
        assert_outside_route(rt, f"{name} {which} s = 2")
        assert same_bits(rt.Render(), resolve.box_filter(want[1]["frame"], W, 2)), f"{name} {which}: s = 2"


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def assert_brute_route(rt, label, bit):
    info, ti = rt.rays_info(), rt.tiles_info()
    assert (info["source"], info["grid_built"], info["grid_in_use"], info["primary_outside_box"]) == (3, 1, 0, 0), f"{label}: {info}"
    assert (ti["enabled"], ti["source"]) == (0, 0) and ti["refused"] & bit and ti["refused"] & 0x1, f"{label}: {ti}"


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_refused_tables_leave_the_frame_to_brute_force(name, monkeypatch):
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene(name)
    # W = 96: tiles are 64 columns wide
    W, H = 96, 64
    z, M, o = pose(name, "y.lo 1.5", W)
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, z, M, o)
        assert_brute_route(rt, f"{name} W = 96", 0x10)
        got = snapshot(rt)
    assert_both(got, fresh(objs, lts, W, H, z, M, o), f"{name} W = 96")
    assert (got["idx"] >= 0).mean() > 0.05
    # 64 x 64, 8 tiles: a scene of fewer than 512 objects stays with the small-scene kernel (one launch), a larger one is served
    W, H = 64, 64
    z, M, o = pose(name, "z.hi 1.5", W)
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, z, M, o)
        if len(objs) < 512:
            assert_brute_route(rt, f"{name} 64 x 64", REFUSED_SMALL)
        else:
            assert_outside_route(rt, f"{name} 64 x 64")
        got = snapshot(rt)
        assert got["wavefront"] == (0 if len(objs) < 512 else 1)
    assert_both(got, fresh(objs, lts, W, H, z, M, o), f"{name} 64 x 64")
    assert (got["idx"] >= 0).mean() > 0.05
    # an origin at 1e9: FAR
    W, H = 64, 64
    o = np.array([1e9, 0.0, -20.0], dtype=np.float32)
    M = camera.look_at(o, (0.0, 0.0, -20.0))
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, -64.0, M, o)
        assert_brute_route(rt, f"{name} 1e9", REFUSED_FAR)
        got = snapshot(rt)
    assert_both(got, fresh(objs, lts, W, H, -64.0, M, o), f"{name} origin at 1e9")
    # ... and at 128 x 64, where nothing else refuses: FAR alone sends the frame to brute force
    W, H = 128, 64
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, -128.0, M, o)
        assert_brute_route(rt, f"{name} 1e9 at 128 x 64", REFUSED_FAR)
        assert rt.tiles_info()["refused"] == REFUSED_FAR | 0x1, "FAR (and the NO_GRID bit every refusal from outside carries), nothing else"
        got = snapshot(rt)
    assert_both(got, fresh(objs, lts, W, H, -128.0, M, o), f"{name} origin at 1e9, 128 x 64")


CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import helpers
import test_pose_offbox_gpu as T
objs, lts = T.scene({name!r})
W, H = 128, 64
z, M, o = T.pose({name!r}, "x.hi 1.5", W)
with T.live(objs, lts, W, H) as rt:
    rt.set_pose(W, H, z, M, o)
    info, ti = rt.rays_info(), rt.tiles_info()
    snap = T.snapshot(rt)
np.savez({out!r}, frame=snap["frame"], t=snap["t"], idx=snap["idx"])
print(json.dumps(dict(grid_in_use=info["grid_in_use"], outside=info["primary_outside_box"], enabled=ti["enabled"], refused=ti["refused"],
                      rays_ref=snap["rays_ref"], hits=snap["hits"], wavefront=snap["wavefront"])))
"""


def test_the_knob_in_a_child_process(tmp_path, monkeypatch):
    clean_env(monkeypatch)
    name = "n300"
    objs, lts = scene(name)
    W, H = 128, 64
    z, M, o = pose(name, "x.hi 1.5", W)
    out = str(tmp_path / "knob.npz")
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), name=name, out=out))
    env = dict(os.environ, RT_POSE_TILES="0")
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    said = json.loads(res.stdout.strip().splitlines()[-1])
    assert (said["grid_in_use"], said["outside"], said["enabled"]) == (0, 0, 0) and said["refused"] & 0x200, said
    assert said["wavefront"] == 0, "300 objects without the grid: the small-scene kernel, as before"
    child = np.load(out)
    want = fresh(objs, lts, W, H, z, M, o, key=(name, (W, H), "x.hi 1.5", "fused"))
    for w in want:
        assert_same(dict(frame=child["frame"], t=child["t"], idx=child["idx"], rays_ref=said["rays_ref"], hits=said["hits"]), w, "RT_POSE_TILES=0")


# ---- 8. history ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_history_does_not_matter(name, monkeypatch):
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene(name)
    W, H = 128, 64
    lo, hi, diag = box_of(name)
    centre = (lo + hi) / 2.0
    # (both near the world's origin, in front of the cloud, looking into it: no object reaches the camera plane)
    inside_a = tuple(np.array([0.5, -0.5, -0.5], dtype=np.float32))
    inside_b = tuple(np.array([1.0, 0.5, -0.2], dtype=np.float32))
    Ma, Mb = camera.look_at(inside_a, centre + np.array([0.0, 0.0, -0.2 * diag])), camera.look_at(inside_b, lo + 0.3 * (hi - lo))
    for p in (inside_a, inside_b):
        assert all(lo[a] <= p[a] <= hi[a] for a in range(3))
    z_out, M_out, o_out = pose(name, "z.hi 1.5", W)
    zc = -float(W)
    with live(objs, lts, W, H) as rt:
        cam = snapshot(rt)
        cam_source = rt.tiles_info()["source"]
        assert cam_source == 1
        rt.set_pose(W, H, zc, Ma, inside_a)
        assert (rt.rays_info()["grid_in_use"], rt.rays_info()["primary_outside_box"]) == (1, 0)
        assert (rt.tiles_info()["source"], rt.tiles_info()["refused"]) == (2, 0)   # as before this route
        assert_both(snapshot(rt), fresh(objs, lts, W, H, zc, Ma, inside_a), f"{name}: an in-box pose")
        rt.set_pose(W, H, z_out, M_out, o_out)
        assert_outside_route(rt, f"{name}: in-box, outside")
        assert_both(snapshot(rt), fresh(objs, lts, W, H, z_out, M_out, o_out, key=(name, (W, H), "z.hi 1.5", "fused")), f"{name}: in-box, outside")
        rt.set_pose(W, H, zc, Mb, inside_b)
        assert (rt.rays_info()["grid_in_use"], rt.rays_info()["primary_outside_box"]) == (1, 0)
        assert (rt.tiles_info()["source"], rt.tiles_info()["refused"]) == (2, 0)
        assert_both(snapshot(rt), fresh(objs, lts, W, H, zc, Mb, inside_b), f"{name}: ..., in-box again")
        rt.set_camera(W, H, zc)
        assert (rt.rays_info()["source"], rt.rays_info()["primary_outside_box"], rt.tiles_info()["source"]) == (1, 0, cam_source)
        assert_same(snapshot(rt), cam, f"{name}: ..., rt_set_camera")
        rt.set_pose(W, H, z_out, M_out, o_out)   # and from a camera straight to the outside pose
        assert_outside_route(rt, f"{name}: camera, outside")
        rt.set_rays(RY.posed_rays(W, H, z_out, M_out, o_out))   # the same rays as a buffer: no common origin, no table
        info = rt.rays_info()
        assert (info["source"], info["grid_in_use"], info["primary_outside_box"]) == (2, 0, 0)
        assert_both(snapshot(rt), fresh(objs, lts, W, H, z_out, M_out, o_out, key=(name, (W, H), "z.hi 1.5", "fused")), f"{name}: the buffer")


# ---- 9. transforms and lights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_after_set_transforms_and_set_lights(name, monkeypatch):
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene(name)
    W, H = 128, 64
    lo, hi, diag = box_of(name)
    centre = (lo + hi) / 2.0
    z, M, o = pose(name, "x.hi 1.5", W)
    # one object moved to just inside the face the pose looks at: in front of the scene for this pose
    moved = objs.copy()
    k = len(objs) // 3
    mv, inv = instance((float(hi[0]) - 3.0, 0.5, float(centre[2])), None, (1.5, 1.5, 1.5))
    rec = R.objects_array([R.make_object(int(objs[k]["type"]), R.Material(), mv, inv)])
    moved[k]["mv"], moved[k]["mvInverse"] = rec[0]["mv"], rec[0]["mvInverse"]
    new_lts = lts.copy()
    new_lts["position"][-1][:3] = (centre + np.array([0.0, 0.9, 0.3]) * diag).astype(np.float32)
    with live(objs, lts, W, H) as rt:
        rt.set_pose(W, H, z, M, o)
        first = snapshot(rt)
        rt.set_transforms(moved[k:k + 1], first=k)
        assert rt.geometry_info()["n_dynamic"] == 1
        assert_outside_route(rt, f"{name}: after set_transforms")
        got = snapshot(rt)
        assert_both(got, fresh(moved, lts, W, H, z, M, o), f"{name}: after set_transforms")
        assert not same_bits(got["frame"], first["frame"]) and (got["idx"] == k).sum() > 0, "the moved object is seen"
        rt.set_pose(W, H, z, M, o)   # the same pose again: its spheres are made from the moved object's new bound
        assert_outside_route(rt, f"{name}: set_transforms, then the pose again")
        assert_both(snapshot(rt), fresh(moved, lts, W, H, z, M, o), f"{name}: set_transforms, then the pose again")
        rt.set_lights(new_lts)
        assert_outside_route(rt, f"{name}: after set_lights")
        assert_both(snapshot(rt), fresh(moved, new_lts, W, H, z, M, o), f"{name}: after set_lights")


# ---- 10. several contexts ------------------------------------------------------------------------------------------------------------------
def test_rt_set_pose_multi_takes_the_route(monkeypatch):
    """rt_set_pose_multi needs no new argument: every shard settles its own table, and the stitched frame is the fresh context's."""
    import ctypes
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer, RTRaysInfo, RTTilesInfo
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    name = "n2000"
    objs, lts = scene(name)
    W, H = 128, 64
    z, M, o = pose(name, "y.lo 1.5", W)
    want = fresh(objs, lts, W, H, z, M, o, key=(name, (W, H), "y.lo 1.5", "fused"))
    with MultiHIPRaytracer(objs, lts, None, DEPTH, devices=(0, 0), camera=(W, H, -float(W)), kernel=KERNEL) as multi:
        multi.set_pose(W, H, z, M, o)
        for shard in range(2):
            ctx = multi._lib.rt_multi_context(multi._m, shard)
            info, ti = RTRaysInfo(), RTTilesInfo()
            assert multi._lib.rt_get_rays_info(ctx, ctypes.byref(info)) == 0 and multi._lib.rt_get_tiles_info(ctx, ctypes.byref(ti)) == 0
            assert (info.source, info.grid_in_use, info.primary_outside_box, ti.enabled, ti.source) == (3, 1, 1, 1, 3), f"shard {shard}"
        assert same_bits(multi.Render(), want[1]["frame"]), "rt_set_pose_multi: the frame"
