"""No GPU: a pose whose origin lies outside the grid's box - the registration spheres made for its own origin
(tiles.pose_registration_spheres; csrc/rt_grid_radii.h holds the expressions, csrc/rt_tiles.hip: pose_spheres evaluates them per pose)
and the screen tiles built from them (tiles.pose_screen_tiles), against the oracle.

Per scene (the generators test_pose_tiles_cpu.py and test_pose_tiles_gpu.py use: the depth-order scenes and s300), with tiles.object_bounds and tiles.grid_constants standing in
for a context's bounds and constants:
1. an origin inside the box reproduces the grid's own spheres (tiles.grid_registration_spheres, grid_radii's formula) bit for bit;
2. an origin outside never shrinks a sphere;
3. for 20 seeded poses outside the box, 1.5 to 4 box diagonals from a face and looking at the box's centre, every primary hit of
   the CPU restatement on rays.posed_rays(...) is in its tile's list, or among the whole-screen entries, with a key <= the hit's t
   (the oracle is oracle.Restatement, as in test_pose_tiles_cpu.py: the tile check needs the hit's INDEX, which cpu_raytracer's
   hittest frame does not carry);
4. the FAR condition accepts those poses and refuses an origin at 1e9.
As everywhere a test can show a margin wrong, never sufficient."""
import functools

import numpy as np
import pytest

from helpers import ROOT
from opencl_raytracer_amd import camera, rays as RY
from test_frame_shapes_cpu import scene
from test_pose_tiles_cpu import TILE_SCENES, T, assert_hits_are_listed, assert_lists_ascend
from test_pose_tiles_cpu import scene_objects as depth_order_scene
from test_primary_depth_order_gpu import lights

N_POSES = 20
OFFBOX_SCENES = TILE_SCENES + ("s300",)   # the depth-order scenes (a few objects, padding far behind) and the dense cloud of s300


def scene_objects(name):
    return (scene("s300")[0], (128, 64, -128.0)) if name == "s300" else depth_order_scene(name)


@functools.lru_cache(maxsize=None)
def bounds_and_constants(name):
    tiles = T()
    objs, _ = scene_objects(name)
    b = tiles.object_bounds(objs)
    return b, tiles.grid_constants(b)


def outside_poses(g, n, seed, W=128):
    """n seeded (M, origin, z): 1.5 .. 4 box diagonals outside one of the six faces (off the face's centre by up to a fifth of a
    diagonal), looking at the box's centre; float32 origins. z zooms in so that the box's circumscribed sphere spans the frame's
    width W, whatever the distance."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(g["box_lo"]), np.asarray(g["box_hi"])
    centre = (lo + hi) / 2.0
    out = []
    for k in range(n):
        axis, side = k % 3, (k // 3) % 2
        o = centre + rng.uniform(-0.2, 0.2, 3) * g["diag"]
        dist = rng.uniform(1.5, 4.0) * g["diag"]
        o[axis] = (hi[axis] + dist) if side else (lo[axis] - dist)
        o = o.astype(np.float32)
        z = -0.5 * W * float(np.linalg.norm(o - centre)) / (0.5 * g["diag"])
        out.append((camera.look_at(o, centre), o, float(np.float32(z))))
    return out


def is_outside(g, o):
    o = np.asarray(o, dtype=np.float64)
    return bool(((o < g["box_lo"]) | (o > g["box_hi"])).any())


def grid_formula(b, g):
    """grid_radii (csrc/rt_scene.cpp, csrc/rt_grid_radii.h) written out once more, object by object in plain Python floats and in its
    order of operations - independent of tiles.py's vectorised helper, which both definitions under test share."""
    import math
    out = []
    for x, y, z, r, k2, ty in b:
        if r == -math.inf:
            out.append(-1.0)
            continue
        if not math.isfinite(r):
            out.append(math.inf)
            continue
        D2 = 0.0
        for c, lo, hi in zip((x, y, z), g["box_lo"], g["box_hi"]):
            d = max(abs(c - float(lo)), abs(float(hi) - c))
            D2 += d * d
        kap, cl = math.sqrt(k2), math.sqrt(x * x + y * y + z * z)
        a2 = r * r * (1.0 + 2e-6)
        L = 2.2e-6 * kap * (g["S_max"] + cl) + 2e-6 * k2 * math.sqrt(D2)
        reg = math.sqrt(a2 + 3e-6 * k2 * D2) + L
        rg = reg * (1.0 + 1e-6) + 0.01 * g["cell"]
        out.append(math.inf if (not math.isfinite(rg) or rg > 0.25 * g["diag"]) else rg)
    return np.array(out)


@pytest.mark.parametrize("name", OFFBOX_SCENES)
def test_an_origin_inside_the_box_reproduces_the_grids_spheres_bit_for_bit(name):
    tiles = T()
    b, g = bounds_and_constants(name)
    want = tiles.grid_registration_spheres(b, g)
    assert want[:, 3].tobytes() == grid_formula(b, g).tobytes(), f"{name}: tiles.grid_registration_spheres is not grid_radii's formula"
    assert np.isfinite(want[:, 3]).sum() >= 96, "the scene's objects have finite registration radii"
    rng = np.random.default_rng(17)
    corners = [g["box_lo"], g["box_hi"], (g["box_lo"] + g["box_hi"]) / 2.0, (0.0, 0.0, 0.0)]
    inside = corners + [g["box_lo"] + rng.uniform(0, 1, 3) * (g["box_hi"] - g["box_lo"]) for _ in range(8)]
    for o in inside:
        o32 = np.asarray(o, dtype=np.float64).astype(np.float32)
        if is_outside(g, o32):   # (the float32 rounding of a corner may leave the box)
            continue
        got = tiles.pose_registration_spheres(b, g, o32)
        assert got.tobytes() == want.tobytes(), f"{name}: origin {o32} inside the box changes a sphere"


@pytest.mark.parametrize("name", OFFBOX_SCENES)
def test_an_origin_outside_never_shrinks_a_sphere(name):
    tiles = T()
    b, g = bounds_and_constants(name)
    base = tiles.grid_registration_spheres(b, g)
    grew = 0
    for M, o, _ in outside_poses(g, N_POSES, seed=23):
        assert is_outside(g, o)
        got = tiles.pose_registration_spheres(b, g, o)
        assert np.array_equal(got[:, :3], base[:, :3])
        assert np.all(got[:, 3] >= base[:, 3]), f"{name}: origin {o}: a sphere shrank"
        grew += int((got[:, 3] > base[:, 3]).sum())
    assert grew > 0, "the poses are far enough for the distance terms to show"


@pytest.mark.parametrize("name", OFFBOX_SCENES)
def test_every_hit_of_an_outside_pose_is_listed_with_a_key_below_its_t(restatement, name):
    tiles = T()
    objs, (W, H, _) = scene_objects(name)
    b, g = bounds_and_constants(name)
    seen = []
    for k, (M, o, z) in enumerate(outside_poses(g, N_POSES, seed=29, W=W)):
        label = f"{name} pose {k} at {o}"
        assert tiles.pose_within_reach(g, o), f"{label}: the FAR condition refuses a test pose"
        spheres = tiles.pose_registration_spheres(b, g, o)
        table = tiles.pose_screen_tiles(spheres, W, H, z, M, o, whole_r=0.25 * g["diag"])
        assert table["enabled"] and table["refused"] == 0, f"{label}: refused {table['refused']:#x}"
        want = restatement[True].render("hittest", objs, lights(), RY.posed_rays(W, H, z, M, o), 0)
        seen.append(float((want["hit_index"] >= 0).mean()))
        assert_lists_ascend(table["tile_start"], table["entries"], table["n_entries"], label)
        table["always"] = np.nonzero(np.isposinf(spheres[:, 3]))[0]
        assert_hits_are_listed(table, len(objs), W, H, want["hit_index"], want["hit_t"], label)
    print(f"\n[pose offbox] {name}: hit shares {min(seen):.4f} .. {max(seen):.4f}")
    assert max(seen) > 0.0 and sum(s > 0 for s in seen) >= N_POSES // 2, f"{name}: the poses see too little: {seen}"


def test_the_far_condition():
    tiles = T()
    b, g = bounds_and_constants("boxes")
    for M, o, _ in outside_poses(g, N_POSES, seed=31):
        assert tiles.pose_within_reach(g, o)
    assert tiles.pose_within_reach(g, (0.0, 0.0, 0.0))
    assert not tiles.pose_within_reach(g, (1e9, 0.0, 0.0)) and not tiles.pose_within_reach(g, (0.0, -1e9, 1e9))
    assert not tiles.pose_within_reach(g, (np.inf, 0.0, 0.0)) and not tiles.pose_within_reach(g, (np.nan, 0.0, 0.0))
    # tiles.pose_growth_ok (a stated limit of the argument, not enforced): true for s300's poses, false for an ill-conditioned object
    b3, g3 = bounds_and_constants("s300")
    for M, o, _ in outside_poses(g3, N_POSES, seed=31):
        assert tiles.pose_growth_ok(b3, g3, o)
    assert b[:, 4].max() > 100 and not all(tiles.pose_growth_ok(b, g, o) for M, o, _ in outside_poses(g, N_POSES, seed=31)), \
        "the boxes scene holds a box of kappa^2 = 900: from a few diagonals out its sphere grows by more than a cell"
    thin = b.copy()
    thin[0, 3:5] = (0.05, 400.0)
    assert tiles.pose_growth_ok(thin, g, (0.0, 0.0, 0.0)) and not tiles.pose_growth_ok(thin, g, (0.0, 0.0, 0.3 * 0.01 * g["cell"] / 3e-6))
    # the limit itself: |o| + far = 0.01 cell / 3e-6
    reach = 0.01 * g["cell"] / 3e-6
    assert tiles.pose_within_reach(g, (0.0, 0.0, 0.3 * reach)) and not tiles.pose_within_reach(g, (0.0, 0.0, 0.6 * reach))


def test_a_sphere_above_a_quarter_of_the_diagonal_is_a_whole_screen_entry():
    tiles = T()
    s = np.array([[0.0, 0.0, -30.0, 5.0], [3.0, 0.0, -30.0, 2.0]])
    plain = tiles.pose_screen_tiles(s, 128, 64, -128.0, np.eye(3))
    assert list(plain["rects"]["cls"]) == [1, 1]
    table = tiles.pose_screen_tiles(s, 128, 64, -128.0, np.eye(3), whole_r=4.0)
    assert list(table["rects"]["cls"]) == [2, 1] and table["n_global"] == 1 and int(table["entries"][table["global_begin"], 0]) == 0


def test_the_names():
    import re
    from opencl_raytracer_amd import hip_raytracer as hr
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    for name in ("RT_TILES_REFUSED_FAR", "primary_outside_box", "rt_read_pose_spheres"):
        assert name in header, name
    assert re.search(r"#define RT_TILES_REFUSED_FAR\s+0x400u", header) and T().REFUSED_FAR == 0x400
    assert re.search(r"#define RT_TILES_REFUSED_SMALL\s+0x800u", header) and T().REFUSED_SMALL == 0x800
    tiles_h = (ROOT / "opencl-raytracer_amd" / "csrc" / "rt_tiles.h").read_text()
    assert re.search(r"kPoseOutsideMinTiles = 16\b", tiles_h) and T().OUTSIDE_MIN_TILES == 16
    assert re.search(r"#define RT_ABI_VERSION 3\b", header)
    assert "rt_read_pose_spheres" in hr.EXPORTS and callable(hr.HIPRaytracer.read_pose_spheres)
    assert "primary_outside_box" in [n for n, _ in hr.RTRaysInfo._fields_]
    assert "RaysInfo" in (ROOT / "opencl-raytracer_amd" / "host" / "HIPRaytracer.hpp").read_text()
