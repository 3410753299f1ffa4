"""No GPU: the screen tiles of a posed camera as tiles.pose_screen_tiles defines them (csrc/rt_grid.h: ScreenTiles, "posed
cameras"; the device builder csrc/rt_tiles.hip is held against this definition in test_pose_tiles_gpu.py).

1. the header, the wrappers and the kernels' table carry the new names;
2. the definition against the oracle on the depth-order scenes under four poses: every primary hit's object is in its tile's
   list (or the global list) with a key not above the hit's t, the lists ascend by (key, index), and every case sees enough;
3. the refusal rules, one case each; 4. the identity pose keeps every membership of the camera's rule.

The registration spheres of a context need the library; here tiles.bounding_spheres(objs, reach) stands in for them: the bound
at the top of rt_grid.h evaluated as build_grid does, for ray origins within REACH of the world's origin (every pose below is).
(A plain 1e-4 relative inflation of the geometric radius is NOT enough: the sphere of radius 0.4 at distance 30 in scene_boxes
reports a t whose point lies 1.05e-4 outside its surface - fp32 error of t scales with the distance, not the radius - and its
key then came out 2.7e-7 above that t under the "moved" pose.) As everywhere, a test can show a margin wrong,
never sufficient: the margins rest on the argument in rt_grid.h."""
import ctypes
import functools
import re

import numpy as np
import pytest

from helpers import ROOT
from opencl_raytracer_amd import rays as RY
from test_primary_depth_order_gpu import SCENES, lights
from test_set_rays_cpu import euler

F = np.float32
NON_ORTHONORMAL = np.array([[1.1, 0.05, 0.0], [0.0, 0.9, 0.02], [0.03, 0.0, 1.2]])
# name -> (matrix, origin)
TILE_POSES = {"identity": (np.eye(3), (0.0, 0.0, 0.0)),
              "turned": (euler(2, -1.5, 3), (0.0, 0.0, 0.0)),
              "moved": (euler(-1, 1, 0), (0.5, -0.5, -1.0)),
              "sheared": (NON_ORTHONORMAL, (0.25, 0.25, -0.5))}
TILE_SCENES = ("stack", "ties", "partial", "boxes")
MIN_HIT_SHARE = 0.05
REACH = 2.0   # every origin of TILE_POSES lies within this distance of the world's origin


def T():
    from opencl_raytracer_amd import tiles
    return tiles


@functools.lru_cache(maxsize=None)
def scene_objects(name):
    make, cam = SCENES[name]
    return make(), cam


def key_matrix(table, n_objs):
    """tiles x objects: the key an object has in a tile's list (+inf: not in the list; the global list: -inf, it has no bound;
    so have the objects of table["always"], if given - the grid's always-list, which the kernel tests for every ray)."""
    n_tiles = table["tiles_x"] * table["tiles_y"]
    start, entries = table["tile_start"], table["entries"]
    keys = np.full((n_tiles, n_objs), np.inf, dtype=np.float32)
    tile_of = np.repeat(np.arange(n_tiles), np.diff(start.astype(np.int64)))
    keys[tile_of, entries[:table["n_entries"], 0]] = entries[:table["n_entries"], 1].copy().view(np.float32)
    g0 = table["global_begin"]
    keys[:, entries[g0:g0 + table["n_global"], 0]] = -np.inf
    keys[:, list(table.get("always", ()))] = -np.inf
    return keys


def assert_lists_ascend(start, entries, n_entries, label):
    idx = entries[:n_entries, 0].astype(np.int64)
    key = entries[:n_entries, 1].copy().view(np.float32).astype(np.float64)
    assert not np.isnan(key).any(), f"{label}: a NaN key"
    tile_of = np.repeat(np.arange(len(start) - 1), np.diff(start.astype(np.int64)))
    same = tile_of[1:] == tile_of[:-1]
    ordered = (key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (idx[1:] > idx[:-1]))
    assert bool(np.all(ordered | ~same)), f"{label}: {int((~ordered & same).sum())} neighbours out of (key, index) order"


def assert_hits_are_listed(table, n_objs, W, H, hit_index, hit_t, label):
    keys = key_matrix(table, n_objs)
    px = np.nonzero(hit_index >= 0)[0]
    row, col = px // W, px % W
    tile = (row >> 3) * table["tiles_x"] + (col >> table["col_shift"])
    k = keys[tile, hit_index[px]]
    missing = np.isposinf(k)
    assert not missing.any(), f"{label}: {int(missing.sum())} hits whose object is not in the tile's list (first: pixel {int(px[missing][0])}, object {int(hit_index[px][missing][0])})"
    above = k > hit_t[px]
    assert not above.any(), f"{label}: {int(above.sum())} keys above their hit's t (worst by {float((k - hit_t[px])[above].max()):.3g})"


# ---- 1. the names -----------------------------------------------------------------------------------------------------------
def test_the_header_and_the_wrappers_carry_the_new_names():
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    for name in ("rt_get_tiles_info", "rt_read_tiles", "rt_tiles_info_t", "build_device_ms", "RT_TILES_REFUSED_LIST"):
        assert name in header, name
    assert re.search(r"#define RT_ABI_VERSION 3\b", header), "the ABI version stays: the new functions are additive"
    grid_h = (ROOT / "opencl-raytracer_amd" / "csrc" / "rt_grid.h").read_text()
    body = grid_h[grid_h.index("struct ScreenTiles {"):]
    body = body[:body.index("};")]
    assert "posed" in body and "width" in body
    assert "TilesInfo" in (ROOT / "opencl-raytracer_amd" / "host" / "HIPRaytracer.hpp").read_text()
    makefile = (ROOT / "opencl-raytracer_amd" / "csrc" / "Makefile").read_text()
    assert "rt_tiles.hip" in makefile and "rt_tiles.o" in makefile
    from opencl_raytracer_amd import hip_raytracer as hr
    for name in ("rt_get_tiles_info", "rt_read_tiles"):
        assert name in hr.EXPORTS
    assert callable(hr.HIPRaytracer.tiles_info) and callable(hr.HIPRaytracer.read_tiles)
    assert ctypes.sizeof(hr.RTTilesInfo) == 64   # 8 x uint32, uint64, 3 x double
    tiles = T()
    flags = {n: getattr(tiles, n) for n in dir(tiles) if n.startswith("REFUSED_")}
    for n, v in flags.items():   # the definition's bits are the header's
        m = re.search(rf"#define RT_TILES_{n}\s+0x([0-9a-fA-F]+)u", header)
        assert m and int(m.group(1), 16) == v, n


# ---- 2. the definition against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", list(TILE_POSES))
@pytest.mark.parametrize("name", TILE_SCENES)
def test_every_hit_is_in_its_tiles_list_with_a_key_below_its_t(restatement, name, pose):
    tiles = T()
    objs, (W, H, z) = scene_objects(name)
    M, origin = TILE_POSES[pose]
    want = restatement[True].render("hittest", objs, lights(), RY.posed_rays(W, H, z, M, origin), 0)
    share = float((want["hit_index"] >= 0).mean())
    table = tiles.pose_screen_tiles(tiles.bounding_spheres(objs, REACH), W, H, z, M, origin)
    label = f"{name} {pose}"
    print(f"\n[pose tiles] {label}: hit share {share:.3f}, entries {table['n_entries']}, global {table['n_global']}, longest list "
          f"{table['max_list']}, eps {table['eps']:.3g}, pad {table['pad']:.3g}")
    assert share >= MIN_HIT_SHARE, f"{label}: the case sees too little ({share:.3f})"
    assert table["enabled"] and table["refused"] == 0 and table["col_shift"] == 6, label
    assert (table["tiles_x"], table["tiles_y"]) == (W // 64, (H + 7) // 8)
    assert 0 < table["pad"] < 1e-3 and table["eps"] < table["pad"], "the pad of these poses is a small fraction of a pixel"
    assert int(table["tile_start"][-1]) == table["n_entries"] == table["global_begin"]
    assert not table["entries"][-1].any(), "one zeroed entry behind the last"
    assert_lists_ascend(table["tile_start"], table["entries"], table["n_entries"], label)
    assert_hits_are_listed(table, len(objs), W, H, want["hit_index"], want["hit_t"], label)


# ---- 3. the refusals -------------------------------------------------------------------------------------------------------------
def some_spheres(n=100, seed=5):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(-60, -20, n), rng.uniform(0.2, 1.0, n)])


def test_refusals_one_case_each():
    tiles = T()
    s, I, o = some_spheres(), np.eye(3), (0.0, 0.0, 0.0)
    ok = tiles.pose_screen_tiles(s, 128, 64, -128.0, I, o)
    assert ok["enabled"] and ok["refused"] == 0
    cases = {
        "W = 96": (tiles.pose_screen_tiles(s, 96, 64, -128.0, I, o), tiles.REFUSED_WIDTH),
        "z > 0": (tiles.pose_screen_tiles(s, 128, 64, 128.0, I, o), tiles.REFUSED_Z),
        "singular M": (tiles.pose_screen_tiles(s, 128, 64, -128.0, [[1, 0, 0], [0, 1, 0], [1, 1, 0]], o), tiles.REFUSED_MATRIX),
        "M not finite": (tiles.pose_screen_tiles(s, 128, 64, -128.0, [[1, 0, 0], [0, np.inf, 0], [0, 0, 1]], o), tiles.REFUSED_MATRIX),
        "ill-conditioned M": (tiles.pose_screen_tiles(s, 128, 64, -128.0, [[1, 0, 0], [0, 1, 0], [1, 1, 1e-6]], o), tiles.REFUSED_EPS),
        "off the grid": (tiles.pose_screen_tiles(s, 128, 64, -128.0, I, o, grid_in_use=False), tiles.REFUSED_NO_GRID),
    }
    # 65 spheres that reach the camera plane: the whole screen each
    whole = np.tile(np.array([[0.0, 0.0, -1.0, 5.0]]), (65, 1))
    cases["65 whole-screen spheres"] = (tiles.pose_screen_tiles(np.concatenate([s, whole]), 128, 64, -128.0, I, o), tiles.REFUSED_GLOBAL)
    assert tiles.pose_screen_tiles(np.concatenate([s, whole[:64]]), 128, 64, -128.0, I, o)["enabled"], "64 of them are served"
    # 1 100 tiny spheres along the ray of pixel (32, 4): one tile's list (the cap is a condition of the sort, not a measurement)
    v = np.array([32 - 64.0, (64 - 4) - 32.0, -128.0])
    scale = np.linspace(0.5, 1.5, 1100)
    tiny = np.column_stack([scale[:, None] * v[None, :], 0.001 * scale])
    long_list = tiles.pose_screen_tiles(tiny, 128, 64, -128.0, I, o)
    assert long_list["max_list"] == 1100 and long_list["n_entries"] == 1100, "all of them sit in one tile"
    cases["1 100 in one tile"] = (long_list, tiles.REFUSED_LIST)
    assert tiles.pose_screen_tiles(tiny[:1024], 128, 64, -128.0, I, o)["enabled"], "1 024 are sorted"
    # more pairs than 256 n + 4096: every sphere over most of a frame of many tiles
    wide = np.tile(np.array([[0.0, 0.0, -10.0, 9.7]]), (8, 1))   # 13 x 64 of the 16 x 64 tiles each
    cases["over the pair budget"] = (tiles.pose_screen_tiles(wide, 1024, 512, -100.0, I, o), tiles.REFUSED_BUDGET)
    for label, (table, bit) in cases.items():
        assert not table["enabled"] and table["refused"] & bit, f"{label}: refused = {table['refused']:#x}"


def test_spheres_behind_the_camera_and_without_a_bound_are_in_no_list():
    tiles = T()
    s = np.array([[0.0, 0.0, 30.0, 5.0],          # entirely behind the camera
                  [0.0, 0.0, -30.0, np.inf],      # the always-list: the kernel tests it for every ray
                  [0.0, 0.0, -30.0, -np.inf],     # never hit
                  [0.0, 0.0, -30.0, np.nan],
                  [0.0, 0.0, -30.0, 5.0],         # listed
                  [0.0, 0.0, 3.0, 5.0]])          # reaches the camera plane: the whole screen
    table = tiles.pose_screen_tiles(s, 128, 64, -128.0, np.eye(3))
    assert list(table["rects"]["cls"]) == [0, 0, 0, 0, 1, 2]
    assert table["n_global"] == 1 and int(table["entries"][table["global_begin"], 0]) == 5
    assert set(table["entries"][:table["n_entries"], 0]) == {4}
    key = table["entries"][:table["n_entries"], 1].copy().view(np.float32)
    assert np.all(key < 25.0 / 128.0) and np.all(key > 24.9 / 128.0), "t >= (c.z + R) / z = 25 / 128, rounded down"


# ---- 4. the identity pose against the camera's rule ----------------------------------------------------------------------------
def camera_memberships(spheres, W, H, z, col_shift=6):
    """rt_camera_tiles.cpp: screen_rect and build_screen_tiles' tile ranges, per object (x0, x1, y0, y1) or None."""
    out = []
    half_w, half_h = float(F(W) / F(2)), float(F(H) / F(2))
    for cx, cy, cz, r in spheres:
        if not (r >= 0) or r == np.inf or cz - r >= 0:
            out.append(None)
            continue
        rect = []
        for cu in (cx, cy):
            lo, hi = -np.inf, np.inf
            if not cz + r >= 0:
                a, b, c = cz * cz - r * r, -2.0 * z * cu * cz, z * z * (cu * cu - r * r)
                disc = b * b - 4.0 * a * c
                if a > 0 and disc >= 0:
                    u0, u1 = sorted(((-b - np.sqrt(disc)) / (2.0 * a), (-b + np.sqrt(disc)) / (2.0 * a)))
                    u0 -= 1.0 + 1e-6 * abs(u0)
                    u1 += 1.0 + 1e-6 * abs(u1)
                    lo, hi = float(np.nextafter(F(u0), F(-np.inf))), float(np.nextafter(F(u1), F(np.inf)))
            rect += [lo, hi]
        c0, c1, r0, r1 = rect[0] + half_w, rect[1] + half_w, H - half_h - rect[3], H - half_h - rect[2]
        cx0, cx1 = max(0.0, np.floor(c0)), min(W - 1.0, np.ceil(c1))
        ry0, ry1 = max(0.0, np.floor(r0)), min(H - 1.0, np.ceil(r1))
        out.append(None if cx0 > cx1 or ry0 > ry1 else (int(cx0) >> col_shift, int(cx1) >> col_shift, int(ry0) >> 3, int(ry1) >> 3))
    return out


@pytest.mark.parametrize("name", TILE_SCENES)
def test_the_identity_pose_keeps_every_membership_of_the_camera_rule(name):
    tiles = T()
    objs, (W, H, z) = scene_objects(name)
    s = tiles.bounding_spheres(objs, REACH)
    table = tiles.pose_screen_tiles(s, W, H, z, np.eye(3))
    r = table["rects"]
    listed = 0
    for i, m in enumerate(camera_memberships(s, W, H, z)):
        if m is None:
            continue
        listed += 1
        assert r["cls"][i] in (1, 2), f"object {i} is in the camera's lists and in none of the pose's"
        if r["cls"][i] == 1:
            assert r["x0"][i] <= m[0] and r["x1"][i] >= m[1] and r["y0"][i] <= m[2] and r["y1"][i] >= m[3], f"object {i}: {m} is not inside the pose's rectangle"
    assert listed >= 8
