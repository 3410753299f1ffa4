"""GPU: the screen tiles of a posed camera, built on the device (csrc/rt_tiles.hip), and the frames traced through them
(rt_wavefront.hip: wf_trace_primary_tiles with ScreenTiles::posed) - against tiles.pose_screen_tiles, against brute force and
against the same context with RT_POSE_TILES=0, bit for bit.

1. the table: enabled, ascending, every primary hit of a brute-force context listed with a key <= its t, two builds the same
   bytes, the pair count the definition's; 2. frames in the three arithmetic modes; 3. frame shapes; 4. list lengths on both
   sides of the two sort kernels' limits; 5. objects behind and at the camera plane; 6. a live context walked through cameras,
   poses and a ray buffer; 7. shards, passes, 8-bit frames, supersampling, several contexts; 8. an origin off the grid.
The brute-force context is created with rays.posed_rays(...) and grid=False: every ray against every object."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import R
from opencl_raytracer_amd import camera, rays as RY, resolve, sharding
from test_context_lifecycle_gpu import clean_env
from test_frame_shapes_cpu import camera_z_for, scene
from test_frame_shapes_gpu import packed_of, same_bits, stitched
from test_pose_tiles_cpu import TILE_POSES, TILE_SCENES, assert_hits_are_listed, assert_lists_ascend, scene_objects
from test_primary_depth_order_gpu import MODES, bits, hip, lights, scene_global, sphere
from test_set_rays_cpu import POSES

pytestmark = pytest.mark.gpu
DEPTH = 2
F = np.float32


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (objects, lights, W, H, z, M, origin): the depth-order scenes under the four poses, and s300 moved."""
    if name == "s300 moved":
        objs, lts = scene("s300")
        W, H = 64, 48
        return objs, lts, W, H, camera_z_for("s300", W, H), POSES["moved"][0], POSES["moved"][1]
    sc, pose = name.split(" ")
    objs, (W, H, z) = scene_objects(sc)
    return (objs, lights(), W, H, z) + TILE_POSES[pose]


CASES = [f"{s} {p}" for s in TILE_SCENES for p in TILE_POSES] + ["s300 moved"]
_BRUTE = {}


def snapshot(rt):
    frame = rt.Render()
    t, idx = rt.render_aux()
    st = rt.count_rays()
    return dict(frame=frame, t=t, idx=idx, rays_ref=int(st.rays_reference), hits=int(st.hit_pixels), tests=int(st.object_tests),
                wavefront=int(st.wavefront))


def brute_force(objs, lts, W, H, z, M, origin, kernel="shade_and_reflect", key=None, **flags):
    """A fresh context created with the pose's rays, every ray against every object; remembered per `key`."""
    if key is not None and key in _BRUTE:
        return _BRUTE[key]
    with hip(objs, lts, RY.posed_rays(W, H, z, M, origin), DEPTH, kernel=kernel, raygen=False, path="wavefront", grid=False, **flags) as rt:
        snap = snapshot(rt)
    if key is not None:
        _BRUTE[key] = snap
    return snap


def posed(objs, lts, W, H, z, M, origin, kernel="shade_and_reflect", **flags):
    rt = hip(objs, lts, None, DEPTH, camera=(W, H, z), kernel=kernel, path="wavefront", **flags)
    rt.set_pose(W, H, z, M, origin)
    return rt


def assert_same(got, want, label):
    for k in ("frame", "t", "idx"):
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{label}: {k} differs on {int((a != b).sum())} words"
    assert (got["rays_ref"], got["hits"]) == (want["rays_ref"], want["hits"]), f"{label}: rays_reference / hit_pixels differ"


def as_table(info, start, entries, spheres):
    """(objects registered with an infinite radius are in the grid's always-list: the kernel tests them for every ray, no list holds them)"""
    return dict(tiles_x=info["tiles_x"], tiles_y=info["tiles_y"], col_shift=info["col_shift"], tile_start=start, entries=entries,
                n_entries=info["n_entries"], n_global=info["n_global"], global_begin=info["n_entries"],
                always=np.nonzero(np.isposinf(spheres[:, 3]))[0])


def boundary_slack(rects, W, H):
    """(object, tile) pairs of listed objects one of whose rectangle edges lies within 1e-6 relative of the value at which its
    tile index changes - floor(c0) and floor(r0) at multiples of 64 and 8, ceil(c1) and ceil(r1) one below them - or at which the
    object leaves the screen: the pairs by which a builder that rounds differently in the last bits may differ."""
    e, slack = rects["edges"], 0
    for i in np.nonzero(rects["cls"] > 0)[0]:
        near = False
        for v, step, off, last in ((e["c0"][i], 64, 0, W), (e["c1"][i], 64, -1, W), (e["r0"][i], 8, 0, H), (e["r1"][i], 8, -1, H)):
            if not np.isfinite(v):
                continue
            targets = [round((v - off) / step) * step + off, -1.0, 0.0, last - 1.0, float(last)]
            near = near or any(abs(v - t) <= 1e-6 * max(1.0, abs(v)) for t in targets)
        if near:
            slack += int((rects["x1"][i] - rects["x0"][i] + 2) * (rects["y1"][i] - rects["y0"][i] + 2))
    return slack


# ---- 1. the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_table(name, monkeypatch):
    from opencl_raytracer_amd import tiles
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts, W, H, z, M, origin = case(name)
    want = brute_force(objs, lts, W, H, z, M, origin, kernel="hittest", key=(name, "hittest"))
    with posed(objs, lts, W, H, z, M, origin, kernel="hittest") as rt:
        info = rt.tiles_info()
        assert (info["enabled"], info["source"], info["col_shift"], info["refused"]) == (1, 2, 6, 0), info
        assert (info["tiles_x"], info["tiles_y"]) == (W // 64, (H + 7) // 8)
        start, entries = rt.read_tiles()
        assert int(start[0]) == 0 and int(start[-1]) == info["n_entries"] and len(entries) == info["n_entries"] + info["n_global"]
        assert info["max_list"] == int(np.diff(start.astype(np.int64)).max())
        assert_lists_ascend(start, entries, info["n_entries"], name)
        glob = entries[info["n_entries"]:, 0]
        assert np.all(np.diff(glob.astype(np.int64)) > 0) and not entries[info["n_entries"]:, 1].any(), "the global list: by index, no key"
        assert_hits_are_listed(as_table(info, start, entries, rt.grid_spheres()), len(objs), W, H, want["idx"], want["t"], name)
        rt.set_pose(W, H, z, M, origin)   # the same pose again: built again (a new pose marks the tiles dirty), the same bytes
        start2, entries2 = rt.read_tiles()
        assert start2.tobytes() == start.tobytes() and entries2.tobytes() == entries.tobytes(), "two builds of one pose differ"
        definition = tiles.pose_screen_tiles(rt.grid_spheres(), W, H, z, M, origin)
        slack = boundary_slack(definition["rects"], W, H)
        print(f"\n[pose tiles] {name}: device {info['n_entries']} pairs, definition {definition['n_entries']} (+- {slack}); global "
              f"{info['n_global']} / {definition['n_global']}; longest list {info['max_list']}; eps {info['eps']:.3g} pad {info['pad']:.3g}; "
              f"build {info['build_device_ms']:.3f} ms on the device")
        assert definition["enabled"] and abs(info["n_entries"] - definition["n_entries"]) <= slack
        assert info["eps"] == pytest.approx(definition["eps"], rel=1e-12) and info["pad"] == pytest.approx(definition["pad"], rel=1e-12)
        if slack == 0:
            assert info["n_global"] == definition["n_global"] and np.array_equal(start, definition["tile_start"])
            assert np.array_equal(entries, definition["entries"][:len(entries)]), "no edge near a boundary: the device's table is the definition's"


# ---- 2. frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASES)
def test_frames_are_brute_forces_and_the_grid_walks(name, mode, monkeypatch):
    objs, lts, W, H, z, M, origin = case(name)
    want = brute_force(objs, lts, W, H, z, M, origin, key=(name, mode), **MODES[mode])
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    with posed(objs, lts, W, H, z, M, origin, **MODES[mode]) as rt:
        assert rt.tiles_info()["source"] == 2
        got = snapshot(rt)
    monkeypatch.setenv("RT_POSE_TILES", "0")
    with posed(objs, lts, W, H, z, M, origin, **MODES[mode]) as rt:
        info = rt.tiles_info()
        assert (info["enabled"], info["source"]) == (0, 0) and info["refused"] & 0x200
        walk = snapshot(rt)
    assert got["wavefront"] == 1 and walk["wavefront"] == 1 and want["wavefront"] == 1
    assert_same(got, want, f"{name} {mode}: tiles against brute force")
    assert_same(got, walk, f"{name} {mode}: tiles against RT_POSE_TILES=0")
    assert got["tests"] < want["tests"], f"{name} {mode}: the tile path tested no fewer objects than brute force - did the tile kernel run?"


# ---- 3. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 8), (128, 16), (192, 40), (128, 20), (96, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_shapes(shape, monkeypatch):
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    W, H = shape
    objs = scene_objects("boxes")[0]
    z = float(-W)   # the scenes' horizontal field of view
    M, origin = TILE_POSES["moved"]
    want = brute_force(objs, lights(), W, H, z, M, origin, kernel="hittest")
    with posed(objs, lights(), W, H, z, M, origin, kernel="hittest") as rt:
        info = rt.tiles_info()
        if W % 64:
            assert (info["enabled"], info["source"]) == (0, 0) and info["refused"] == 0x10, "tiles of 64 columns: refused, not an error"
        else:
            assert (info["enabled"], info["source"], info["tiles_x"], info["tiles_y"]) == (1, 2, W // 64, (H + 7) // 8)
        got = snapshot(rt)
    assert_same(got, want, f"{W} x {H}")
    assert (want["idx"] >= 0).mean() >= 0.05, "the shape sees too little"
    if W % 64 == 0:
        assert got["tests"] < want["tests"]


# ---- 4. list lengths ------------------------------------------------------------------------------------------------------------
LIST_SHAPE = (192, 16, -192.0)            # 3 x 2 tiles
LIST_LENGTHS = (0, 1, 64, 65, 100, 3)     # per tile, row-major: none; one wave (1, 64, 3); one workgroup (65, 100)


def cluster(n, tile_x, tile_y, M, origin, seed, z=LIST_SHAPE[2], W=LIST_SHAPE[0], H=LIST_SHAPE[1], spread=20.0):
    """n spheres of radius 0.08 whose images lie inside tile (tile_x, tile_y): within +-spread columns of column 32 and +-1 row of
    row 3.5 of the tile, 50 .. 60 deep in the camera's frame (a world position is origin + M x camera position). With the
    rectangle's pixel of pad a registration radius of up to 0.39 (1.5 rows at depth 50) keeps floor(r0) and ceil(r1) inside the tile."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        col, row = 64 * tile_x + 32 + rng.uniform(-spread, spread), 8 * tile_y + 3.5 + rng.uniform(-1.0, 1.0)
        v = np.array([col - W / 2, (H - row) - H / 2, z])
        p = np.asarray(origin) + np.asarray(M, dtype=np.float64) @ (v * (rng.uniform(50.0, 60.0) / -z))
        out.append(sphere(700 + 97 * seed + k, tuple(p), 0.08))
    return out


def list_scene(lengths=LIST_LENGTHS):
    M, origin = TILE_POSES["moved"]
    recs = []
    for t, n in enumerate(lengths):
        recs += cluster(n, t % 3, t // 3, M, origin, seed=t)
    return R.objects_array(recs)


def test_list_lengths_on_both_sides_of_the_sort_kernels(monkeypatch):
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    W, H, z = LIST_SHAPE
    M, origin = TILE_POSES["moved"]
    objs = list_scene()
    assert len(objs) >= 96
    want = brute_force(objs, lights(), W, H, z, M, origin, kernel="hittest")
    with posed(objs, lights(), W, H, z, M, origin, kernel="hittest") as rt:
        info = rt.tiles_info()
        start, entries = rt.read_tiles()
        assert tuple(np.diff(start.astype(np.int64))) == LIST_LENGTHS, "the clusters do not fill the lists they were made for"
        assert (info["enabled"], info["max_list"], info["n_entries"], info["n_global"]) == (1, 100, sum(LIST_LENGTHS), 0)
        assert_lists_ascend(start, entries, info["n_entries"], "lists")
        for t in range(6):   # every list holds its own cluster, each object once
            first = sum(LIST_LENGTHS[:t])
            assert sorted(entries[start[t]:start[t + 1], 0]) == list(range(first, first + LIST_LENGTHS[t])), f"tile {t}"
        assert_hits_are_listed(as_table(info, start, entries, rt.grid_spheres()), len(objs), W, H, want["idx"], want["t"], "lists")
        got = snapshot(rt)
    assert_same(got, want, "lists of 0, 1, 64, 65, 100 and 3 entries")
    assert (want["idx"] >= 0).sum() >= 20, "the clusters are seen"


def test_a_list_beyond_the_cap_is_refused_and_the_frame_still_right(monkeypatch):
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    W, H, z = LIST_SHAPE
    M, origin = TILE_POSES["moved"]
    objs = R.objects_array(cluster(1100, 1, 0, M, origin, seed=9) + cluster(5, 2, 1, M, origin, seed=10))
    want = brute_force(objs, lights(), W, H, z, M, origin, kernel="hittest")
    with posed(objs, lights(), W, H, z, M, origin, kernel="hittest") as rt:
        info = rt.tiles_info()
        assert (info["enabled"], info["source"]) == (0, 0) and info["refused"] == 0x80 and info["max_list"] == 1100, info
        got = snapshot(rt)
    assert_same(got, want, "1 100 entries in one tile")


# ---- 5. behind the camera ---------------------------------------------------------------------------------------------------------
def test_objects_behind_and_at_the_camera_plane(monkeypatch):
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    M, origin = TILE_POSES["moved"]
    behind = np.asarray(origin) + np.asarray(M) @ np.array([1.0, 2.0, 20.0])   # 20 behind the posed camera
    objs = np.concatenate([scene_global(), R.objects_array([sphere(90, tuple(behind), 5.0)])])
    W, H, z = 128, 64, -128.0
    want = brute_force(objs, lights(), W, H, z, M, origin)
    with posed(objs, lights(), W, H, z, M, origin) as rt:
        info = rt.tiles_info()
        start, entries = rt.read_tiles()
        spheres = rt.grid_spheres()
        assert spheres[100, 2] + spheres[100, 3] > 0, "the sphere reaches the camera plane"
        assert info["enabled"]
        if np.isfinite(spheres[100, 3]):   # (registered with an infinite radius it is in the grid's always-list instead)
            assert info["n_global"] >= 1 and 100 in set(entries[info["n_entries"]:, 0]), "the sphere at the camera plane: global"
        assert_hits_are_listed(as_table(info, start, entries, spheres), len(objs), W, H, want["idx"], want["t"], "behind")
        assert np.isfinite(spheres[-1, 3]) and len(objs) - 1 not in set(entries[:, 0]), "the sphere behind the camera is in no list"
        got = snapshot(rt)
    assert_same(got, want, "behind and at the camera plane")
    assert 100 in set(np.unique(want["idx"])) and len(objs) - 1 not in set(np.unique(want["idx"]))


# ---- 6. a live context ---------------------------------------------------------------------------------------------------------
def test_a_live_context_through_cameras_poses_and_a_buffer(monkeypatch):
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts, W, H, z, A, oA = case("boxes turned")
    B, oB = TILE_POSES["sheared"]
    want_a = brute_force(objs, lts, W, H, z, A, oA, key=("boxes turned", "fused"))
    want_b = brute_force(objs, lts, W, H, z, B, oB, key=("boxes sheared", "fused"))
    with hip(objs, lts, None, DEPTH, camera=(W, H, z), path="wavefront") as rt:
        cam = snapshot(rt)
        assert (rt.tiles_info()["source"], rt.tiles_info()["col_shift"]) == (1, 3)
        rt.set_pose(W, H, z, A, oA)
        assert rt.tiles_info()["source"] == 2
        assert_same(snapshot(rt), want_a, "camera, pose A")
        table_a = rt.read_tiles()
        rt.set_camera(W, H, z)
        assert rt.tiles_info()["source"] == 1
        assert_same(snapshot(rt), cam, "camera, pose A, camera")
        rt.set_pose(W, H, z, B, oB)
        info = rt.tiles_info()
        assert info["source"] == 2 and rt.read_tiles()[1].tobytes() != table_a[1].tobytes()
        assert_same(snapshot(rt), want_b, "..., pose B")
        rt.set_rays(RY.posed_rays(W, H, z, A, oA))
        info = rt.tiles_info()
        assert (info["enabled"], info["source"]) == (0, 0), "a ray buffer has no tiles"
        assert_same(snapshot(rt), want_a, "..., set_rays(A)")
        rt.set_pose(W, H, z, A, oA)
        assert rt.tiles_info()["source"] == 2
        again = rt.read_tiles()
        assert again[0].tobytes() == table_a[0].tobytes() and again[1].tobytes() == table_a[1].tobytes()
        assert_same(snapshot(rt), want_a, "..., pose A")


# ---- 7. partitions ---------------------------------------------------------------------------------------------------------------
def test_partitions_of_a_posed_frame(monkeypatch):
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer, RTTilesInfo
    clean_env(monkeypatch)
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts, W, H, z, M, origin = case("boxes moved")
    n = W * H
    want = brute_force(objs, lts, W, H, z, M, origin, key=("boxes moved", "fused"))
    with posed(objs, lts, W, H, z, M, origin) as rt:
        for label, tr in (("16-row tiles", sharding.tile_rays_for_rows(W, 16)), ("tiles of 50 rays", 50)):
            pieces, ts, idxs = [], [], []
            for rank in range(2):
                rt.set_shard(tr, rank, 2)
                assert rt.tiles_info()["source"] == 2
                pieces.append(rt.Render())
                t, idx = rt.render_aux()
                ts.append(t)
                idxs.append(idx)
            assert same_bits(stitched(pieces, tr, n), want["frame"]), f"{label}: the stitched frame"
            assert same_bits(stitched(ts, tr, n), want["t"]) and np.array_equal(stitched(idxs, tr, n), want["idx"]), label
        rt.set_shard(0, 0, 1)
        assert np.array_equal(rt.render_packed("rgba8"), packed_of(want["frame"], "rgba8")), "rgba8"
        monkeypatch.setenv("RT_RENDER_PASSES", "2")
        assert same_bits(rt.Render(), want["frame"]), "two passes"
        clean_env(monkeypatch)
    # s = 2 over a sample grid of 128 x 32
    sw, sh, sz = camera.supersampled(64, 16, -64.0, 2)
    assert (sw, sh) == (128, 32)
    samples = brute_force(objs, lts, sw, sh, float(sz), M, origin)
    with posed(objs, lts, sw, sh, float(sz), M, origin) as rt:
        rt.set_supersampling(2)
        assert rt.tiles_info()["source"] == 2
        assert same_bits(rt.Render(), resolve.box_filter(samples["frame"], sw, 2)), "s = 2"
    # two contexts on one GPU, posed twice
    with MultiHIPRaytracer(objs, lts, None, DEPTH, devices=(0, 0), camera=(W, H, z)) as multi:
        for k in range(2):
            multi.set_pose(W, H, z, M, origin)
            assert same_bits(multi.Render(), want["frame"]), f"rt_set_pose_multi, call {k}"
        info = RTTilesInfo()
        assert multi._lib.rt_get_tiles_info(multi._lib.rt_multi_context(multi._m, 1), ctypes.byref(info)) == 0
        assert info.source in (0, 2)   # (a shard of the small-scene path has no tiles)


# ---- 8. off the grid -------------------------------------------------------------------------------------------------------------
def test_an_origin_outside_the_grids_box(monkeypatch):
    monkeypatch.delenv("RT_POSE_TILES", raising=False)
    objs, lts = scene("s300")
    W, H = 64, 48
    M, origin, zs = POSES["far"]
    z = camera_z_for("s300", W, H, zs)
    want = brute_force(objs, lts, W, H, z, M, origin)
    with posed(objs, lts, W, H, z, M, origin) as rt:
        assert rt.rays_info()["grid_in_use"] == 0
        info = rt.tiles_info()
        assert (info["enabled"], info["source"]) == (0, 0) and info["refused"] & 0x1
        got = snapshot(rt)
    assert_same(got, want, "an origin outside the box")
    assert (want["idx"] >= 0).mean() > 0.05
