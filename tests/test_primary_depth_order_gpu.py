"""GPU: the primary round's depth-ordered screen-tile lists and their wave-wide early exit (rt_grid.h: ScreenTiles;
rt_wavefront.hip: wf_trace_primary_tiles) against brute force, bit for bit.

Every scene holds >= 96 objects and is rendered on the large-scene path, once through the tiles (the default) and once with
grid=False (every ray against every object). Frame, primary t and hit index are compared as 32-bit words, rays_traced and
hit_pixels for equality. Each scene is built around one way the exit could go wrong; the frames are 128 x 64 or 256 x 128.

Reading of the first case: a table sorted by key is the same table whatever the objects' indices are, so "fewer tests than
with the index order reversed" cannot hold for a correct build - with either index order the lists come out near first.
What is asserted instead is what that sentence is after: with the spheres indexed near-first and far-first the tile path
(1) gives equal frames, (2) executes the SAME number of tests - the order is by depth, not by index - and (3) executes fewer
tests than any walk of the whole lists must: a sphere that the ray of some pixel of a tile geometrically hits is in that
tile's list, and a whole-list walk runs every entry on all 64 lanes, so it executes at least 64 x the number of (tile, sphere)
pairs with such a pixel. (A first form of (3) counted (pixel, sphere) pairs instead. No build can meet that in a frame of
256 x 128: the eight silhouettes coincide, a disc of radius r = 54 pixels; the lists are made from bounding RECTANGLES, so
the tiles of the rectangle that the disc does not fill, (2r + 16)^2 - pi (r - 8)^2 = 8 700 pixels, walk all eight entries
with or without the exit, and 6 650 + 8 x 8 700 = 76 000 already exceeds the 8 x pi r^2 = 73 000 pairs. Counted by tiles the
whole-list walk needs >= 8 x (6 650 + the ~6 500 pixels of the rim's tiles) = 105 000.)"""
import numpy as np
import pytest

from helpers import R, instance, light_in_reach, rotation
from opencl_raytracer_amd import sharding, tessellate as T
from test_frame_shapes_cpu import launch_form, pinhole_rays

pytestmark = pytest.mark.gpu
DEPTH = 2
CAM = (128, 64, -128.0)
MODES = {"fused": {}, "unfused": dict(fused=False), "device_opencl": dict(device_opencl=True)}
_REFERENCE = {}


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def material(k):
    rng = np.random.default_rng(1000 + k)
    return R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                      absorption=float(rng.choice([1.0, 0.7, 0.4])), reflection=0.0, shininess=float(rng.choice([1.0, 5.0, 30.0])))


def sphere(k, centre, r):
    return R.make_object(R.SPHERE, material(k), *instance(centre, None, (r, r, r)))


def box(k, centre, scale, rot=None):
    return R.make_object(R.BOX, material(k), *instance(centre, rot, scale))


def padding(n, depth, at=(0.44, 0.21), seed=3):
    """n spheres of radius 0.05 far off, in a small patch of the frame around direction (at.x, at.y, -1): they bring a scene
    over the 96 objects of the large-scene path without sitting in many tile lists."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        d = depth * rng.uniform(1.0, 1.1)
        out.append(sphere(500 + k, ((at[0] + rng.uniform(-0.03, 0.03)) * d, (at[1] + rng.uniform(-0.02, 0.02)) * d, -d), 0.05))
    return out


def lights():
    props = [R.LightProperties(ambient=(0.1, 0.1, 0.1), diffuse=(0.5, 0.4, 0.3), specular=(0.3, 0.3, 0.3)),
             R.LightProperties(ambient=(0.0, 0.1, 0.1), diffuse=(0.3, 0.4, 0.5), specular=(0.2, 0.3, 0.4))]
    return R.lights_array([R.make_light(props[0], position=(-50.0, 40.0, 30.0, 1.0)), R.make_light(props[1], position=(30.0, 60.0, 40.0, 1.0))])


# ---- the scenes -------------------------------------------------------------------------------------------------------------
STACK_DEPTHS = [20.0 * 1.4 ** k for k in range(8)]   # disjoint: sphere k spans depths 0.79 d .. 1.21 d
STACK_TAN = 0.21                                     # radius / depth: 54 pixels of the 256 x 128 frame's 64 above the axis
STACK_CAM = (256, 128, -256.0)


def stack_spheres(far_first):
    recs = [sphere(k, (0.0, 0.0, -d), STACK_TAN * d) for k, d in enumerate(STACK_DEPTHS)]
    return recs[::-1] if far_first else recs


def scene_stack(far_first=False):
    """1: spheres behind one another on the axis, every one covering whole tiles - the exit fires after the first entry. (The
    padding sits behind the stack: in a patch of its own its ~4 tiles, whose lanes mostly miss, would walk 100 entries each.)"""
    return R.objects_array(padding(100, 400.0, at=(0.0, 0.0)) + stack_spheres(far_first))


def scene_ties():
    """2: coincident objects at different indices with other objects between them in index order: sphere + sphere and box + box
    (equal keys: both must be tested, the tie rules pick the winner), and a sphere inside a box whose front face touches it (the
    same near t on the axis ray, different keys)."""
    pad = padding(96, 200.0)
    recs = pad[:3] + [sphere(1, (-8.0, 0.0, -30.0), 3.0)] + pad[3:10]
    recs += [box(2, (8.0, 0.0, -30.0), (4.0, 4.0, 4.0), rotation((0, 1, 0), 0.3))] + pad[10:20]
    recs += [sphere(3, (0.0, 0.0, -30.0), 2.0)] + pad[20:50]
    recs += [sphere(4, (-8.0, 0.0, -30.0), 3.0)] + pad[50:60]
    recs += [box(5, (8.0, 0.0, -30.0), (4.0, 4.0, 4.0), rotation((0, 1, 0), 0.3))] + pad[60:70]
    recs += [box(6, (0.0, 0.0, -30.0), (4.0, 4.0, 4.0))] + pad[70:]
    return R.objects_array(recs)


GAP_PIXEL = (67, 29)   # direction (3, 3, -128): through (1.5, 1.5) at depth 64


def scene_partial():
    """3: a near sphere over part of a few tiles with far objects behind the uncovered lanes (those lanes miss until late: no
    early exit), and a far wall of four boxes that leaves a hole of one pixel: a tile in which one lane hits nothing at all."""
    recs = padding(100, 300.0)
    recs += [sphere(1, (0.75, 0.2, -16.0), 0.3), sphere(2, (-2.0, 1.0, -16.0), 0.9), sphere(9, (3.5, 1.0, -100.0), 1.2)]
    recs += [box(3, (-18.7, 0.0, -64.0), (40.0, 60.0, 1.0)), box(4, (21.7, 0.0, -64.0), (40.0, 60.0, 1.0)),      # x < 1.3, x > 1.7
             box(5, (0.0, 21.7, -64.0), (100.0, 40.0, 1.0)), box(6, (0.0, -18.7, -64.0), (100.0, 40.0, 1.0))]   # y > 1.7, y < 1.3
    recs += [sphere(7, (-20.0, 5.0, -100.0), 6.0), sphere(8, (15.0, -10.0, -100.0), 8.0)]
    return R.objects_array(recs)


def scene_boxes():
    """4: rotated, non-uniformly scaled boxes seen edge-on - the near face lies well inside the registration sphere, the key is far
    from tight - with small spheres inside those spheres; and a cube that turns a corner to the camera: the corner is the hit."""
    diag = rotation(np.cross((1, 1, 1), (0, 0, 1)), np.arccos(1 / np.sqrt(3)))   # (1, 1, 1) / sqrt 3  ->  +z
    recs = padding(100, 300.0)
    recs += [box(1, (0.0, -1.0, -40.0), (10.0, 0.05, 10.0), rotation((1, 0, 0), 0.035)),
             box(2, (6.0, 1.0, -45.0), (0.3, 6.0, 9.0), rotation((1, 2, 3), 0.8)),
             box(3, (-7.0, 0.0, -35.0), (4.0, 4.0, 4.0), diag),
             sphere(4, (0.0, 0.5, -38.0), 1.0), sphere(5, (0.0, -2.5, -36.0), 0.8),
             sphere(6, (-7.0, 0.0, -45.0), 2.5), sphere(7, (-7.0, 0.0, -30.0), 0.4), sphere(8, (6.5, 1.0, -41.0), 0.7)]
    return R.objects_array(recs)


def scene_overlap():
    """5: overlapping depth ranges. A large sphere (key depth 40) in front of which, at the tiles where it counts, sits a small
    one with the LARGER key (43); a small one (key 51) behind the large sphere's surface (depth ~43); and a pair whose winner
    changes from lane to lane: small sphere key 42, front 42 .. 45, large sphere key 43.6 with its surface at 43.6 .. 44."""
    recs = padding(100, 300.0)
    recs += [sphere(1, (15.0, 0.0, -60.0), 20.0), sphere(2, (0.0, 0.0, -44.0), 1.0),
             sphere(3, (-15.0, 0.0, -60.0), 20.0), sphere(4, (-6.0, 0.0, -52.0), 1.0),
             sphere(5, (0.0, 6.0, -45.0), 3.0), sphere(6, (0.0, 6.0, -63.6), 20.0)]
    return R.objects_array(recs)


def scene_global():
    """6: a sphere whose registration sphere reaches the camera plane (the per-camera global list, tested first, without a key) in
    front of tiled objects."""
    recs = padding(100, 300.0)
    recs += [sphere(1, (0.0, -12.0, -8.0), 10.0)]
    recs += [sphere(10 + k, (0.0, -3.0 + 1.5 * k, -d), 0.12 * d) for k, d in enumerate((25.0, 35.0, 50.0, 70.0))]
    return R.objects_array(recs)


SCENES = {"stack": (scene_stack, STACK_CAM), "ties": (scene_ties, CAM), "partial": (scene_partial, CAM), "boxes": (scene_boxes, CAM),
          "overlap": (scene_overlap, CAM), "global": (scene_global, CAM)}


# ---- rendering and comparing -------------------------------------------------------------------------------------------------
def snapshot(rt):
    frame = rt.Render()
    t, idx = rt.render_aux()
    st = rt.count_rays()
    return dict(frame=frame, t=t, idx=idx, traced=int(st.rays_traced), hits=int(st.hit_pixels), tests=int(st.object_tests),
                wavefront=int(st.wavefront))


def render(objs, cam, kernel="shade_and_reflect", **flags):
    with hip(objs, lights(), None, DEPTH, camera=cam, kernel=kernel, path="wavefront", **flags) as rt:
        return snapshot(rt)


def assert_same(got, want, label):
    for key in ("frame", "t", "idx"):
        a, b = bits(got[key]), bits(want[key])
        assert a.shape == b.shape and np.array_equal(a, b), f"{label}: {key} differs on {int((a != b).sum())} words"
    assert (got["traced"], got["hits"]) == (want["traced"], want["hits"]), f"{label}: rays_traced / hit_pixels differ"


def tiles_against_brute_force(name, mode):
    make, cam = SCENES[name]
    objs = make()
    assert len(objs) >= 96
    if mode == "device_opencl":
        assert not any(light_in_reach(objs, l["position"], 1e-3) for l in lights()), "a light in reach: the scene would leave the default path"
    key = (name, mode)
    if key not in _REFERENCE:
        _REFERENCE[key] = render(objs, cam, grid=False, **MODES[mode])
    want = _REFERENCE[key]
    got = render(objs, cam, **MODES[mode])
    assert got["wavefront"] == 1 and want["wavefront"] == 1
    assert_same(got, want, f"{name} {mode}")
    assert got["tests"] < want["tests"], f"{name} {mode}: the tile path tested no fewer objects than brute force - were the tiles built?"
    return objs, cam, got, want


@pytest.mark.parametrize("name", list(SCENES))
def test_tiles_equal_brute_force(name):
    objs, cam, got, want = tiles_against_brute_force(name, "fused")
    if name == "partial":   # the scene does what its docstring says: in the tile of GAP_PIXEL exactly that lane misses
        W = cam[0]
        idx = want["idx"].reshape(cam[1], W)
        c0, r0 = GAP_PIXEL[0] // 8 * 8, GAP_PIXEL[1] // 8 * 8
        block = idx[r0:r0 + 8, c0:c0 + 8]
        assert block[GAP_PIXEL[1] - r0, GAP_PIXEL[0] - c0] == -1 and int((block == -1).sum()) == 1
    if name == "ties":      # ... and its coincident pairs do tie: the later sphere wins, the earlier box wins
        seen = {int(i) for i in np.unique(want["idx"])}   # (positions in scene_ties' list: spheres 3 and 53, boxes 11 and 64)
        assert 53 in seen and 3 not in seen, "sphere + sphere: the highest index wins a tie"
        assert 11 in seen and 64 not in seen, "box + box: the lowest index wins a tie"
    if name == "global":
        assert 100 in {int(i) for i in np.unique(want["idx"])}, "the sphere at the camera plane is visible"


@pytest.mark.parametrize("mode", ["unfused", "device_opencl"])
@pytest.mark.parametrize("name", ["stack", "ties", "partial", "boxes", "overlap"])
def test_tiles_equal_brute_force_in_the_other_arithmetic_modes(name, mode):
    tiles_against_brute_force(name, mode)


def test_the_order_is_by_depth_not_by_index():
    """Case 1 (see the module docstring for the reading): near-first and far-first indices give the same frame and the same number
    of executed tests, below what a walk of the whole lists executes at the least."""
    W, H, z = STACK_CAM
    near, far = scene_stack(False), scene_stack(True)
    n, K = len(near), len(STACK_DEPTHS)
    runs = {}
    for label, objs in (("near first", near), ("far first", far)):
        runs[label] = render(objs, STACK_CAM, kernel="hittest")
        assert_same(runs[label], render(objs, STACK_CAM, kernel="hittest", grid=False), f"stack {label}")
    a, b = runs["near first"], runs["far first"]
    assert np.array_equal(bits(a["frame"]), bits(b["frame"])) and np.array_equal(bits(a["t"]), bits(b["t"]))
    flip = np.where(a["idx"] >= n - K, 2 * n - K - 1 - a["idx"], a["idx"])   # stack sphere j of one scene is sphere K - 1 - j of the other
    assert np.array_equal(flip, b["idx"])
    # (tile, sphere) pairs in which the ray of some pixel of the 8 x 8 tile passes the centre within 0.999 r, in float64
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([col - W / 2, (H - row) - H / 2, np.full_like(col, z)], -1)
    pairs = 0
    for depth in STACK_DEPTHS:
        c = np.array([0.0, 0.0, -depth])
        hit = (np.cross(d, c) ** 2).sum(-1) / (d ** 2).sum(-1) < (0.999 * STACK_TAN * depth) ** 2
        pairs += int(hit.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3)).sum())
    print(f"\n[depth order] executed tests: near first {a['tests']}, far first {b['tests']}; a walk of the whole lists: >= {64 * pairs}; "
          f"pixels {W * H}")
    assert a["tests"] == b["tests"], "the number of executed tests depends on the index order"
    assert a["tests"] < 64 * pairs, "no early exit: the tile path executed as many tests as a walk of the whole lists"


def test_both_tile_shapes():
    """7: the frame in 8 x 8 work-item order (8 x 8 tiles) and the same frame from two shards of 4-row tiles, whose work-items run in
    linear order over 64 x 8 tiles (do_launch: col_shift = wf_tile_order ? 3 : 6; tests/test_frame_shapes_cpu.py: launch_form)."""
    W, H, z = CAM
    tile_rays, world = sharding.tile_rays_for_rows(W, 4), 2
    objs = np.concatenate([scene_overlap(), scene_boxes()[100:]])
    assert launch_form(W, H, z, len(objs))["screen_tiles"] == 3
    whole = render(objs, CAM)
    assert_same(whole, render(objs, CAM, grid=False), "8 x 8 tiles")
    frames, ts, idxs = [], [], []
    with hip(objs, lights(), None, DEPTH, camera=CAM, path="wavefront") as rt:
        for rank in range(world):
            form = launch_form(W, H, z, len(objs), tile_rays, rank, world)
            assert form["screen_tiles"] == 6 and not form["straddle"] and not form["tile_order"]
            rt.set_shard(tile_rays, rank, world)
            frames.append(rt.Render())
            t, idx = rt.render_aux()
            ts.append(t)
            idxs.append(idx)
    n = W * H
    assert np.array_equal(bits(sharding.assemble_frame(frames, tile_rays, n)), bits(whole["frame"])), "64 x 8 tiles: frame"
    assert np.array_equal(bits(sharding.assemble_frame(ts, tile_rays, n)), bits(whole["t"])), "64 x 8 tiles: primary t"
    assert np.array_equal(sharding.assemble_frame(idxs, tile_rays, n), whole["idx"]), "64 x 8 tiles: hit index"


def test_keys_follow_the_camera():
    """8: rt_set_camera on a live context to another z and another frame shape, then back: every frame is the one a fresh
    brute-force context renders for that camera."""
    objs = np.concatenate([scene_overlap(), scene_boxes()[100:], scene_stack()[100:]])
    cams = [CAM, (64, 128, -70.0), (128, 64, -300.0), CAM, (64, 128, -70.0)]
    want = {cam: render(objs, cam, grid=False) for cam in set(cams)}
    with hip(objs, lights(), None, DEPTH, camera=cams[0], path="wavefront") as rt:
        for k, cam in enumerate(cams):
            if k:
                rt.set_camera(*cam)
            assert_same(snapshot(rt), want[cam], f"camera {k} {cam}")


def test_triangles_in_the_tile_lists():
    """10: a tessellated sphere in front of and behind analytic spheres. Triangles have no brute-force loop here: the tile kernel
    (in-kernel pinhole rays) against the grid walk (the same rays uploaded, which never use the screen tiles)."""
    W, H, z = CAM
    analytic = R.objects_array([sphere(1, (0.5, 0.3, -26.0), 0.7), sphere(2, (1.0, 0.0, -40.0), 4.0), sphere(3, (-3.0, 1.0, -33.0), 1.0)])
    mesh = T.tessellate(R.objects_array([sphere(4, (0.0, 0.0, -30.0), 2.0)]), 8, 12, 1)
    objs = np.concatenate([analytic, mesh])
    assert len(objs) >= 96
    with hip(objs, lights(), None, DEPTH, camera=CAM) as rt:
        tiles = snapshot(rt)
    with hip(objs, lights(), pinhole_rays(W, H, z), DEPTH, raygen=False) as rt:
        walk = snapshot(rt)
    assert tiles["wavefront"] == 1 and walk["wavefront"] == 1
    assert_same(tiles, walk, "triangles: tiles against the grid walk")
    seen = {int(i) for i in np.unique(tiles["idx"])}
    assert 0 in seen and 1 in seen and any(i >= 3 for i in seen), "the mesh and the spheres in front of and behind it are all visible"
