"""No GPU: the frame shapes, partitions, scenes and cameras that tests/test_frame_shapes_gpu.py and
tests/test_context_lifecycle_gpu.py render, and the proof that the list is worth rendering.

The host decides the FORM of a launch from a handful of predicates on width, height, shard and object count
(`launch_form` restates them). A frame shape only tests something if it reaches a combination of predicate values
that no other shape reaches, so this file enumerates every combination that a frame of up to 2304 x 1024 pixels can
reach under the listed partitions and asserts that the shared list reaches all of them. The input conditions (hit
share, miss share, rays per pixel) are checked with the oracle alone: they are conditions on the inputs, not
measurements of the HIP path."""
import functools

import numpy as np
import pytest

from helpers import ROOT, R, camera, instance, random_scene, rotation
from opencl_raytracer_amd import scene_loader, sharding, tessellate as T

# ---- the shared lists ---------------------------------------------------------------------------------------------------
FACTORS_9216 = [(96, 96), (128, 72), (72, 128), (64, 144), (36, 256), (18, 512), (9, 1024), (1024, 9), (2304, 4), (1, 9216), (9216, 1)]
FACTORS_1800 = [(36, 50), (50, 36), (72, 25), (120, 15), (200, 9), (8, 225), (40, 45), (24, 75), (1800, 1), (1, 1800)]
SHAPES = [(1, 1), (1, 97), (97, 1), (7, 5), (8, 8), (63, 65), (64, 8), (64, 9), (72, 40), (72, 41), (128, 72), (128, 75), (100, 100),
          (256, 8), (2049, 1), (520, 4), (64, 16), (64, 40), (128, 8), (64, 64), (64, 33), (1, 48), (13, 225), (43, 88), (48, 88)]
ALL_SHAPES = SHAPES + [s for s in FACTORS_9216 + FACTORS_1800 if s not in SHAPES]

# (name, tile rows | None, tile rays | None, world): tile j of `tile_rays` consecutive rays belongs to rank j % world
SHARDS = [("rows16x3", 16, None, 3), ("rows4x2", 4, None, 2), ("rays50x2", None, 50, 2), ("rows8x5", 8, None, 5)]
# RT_RENDER_SPLIT of a Render() forced through passes (RT_RENDER_PASSES=2); None: the default ("3,1" floats, "7,1" bytes)
SPLITS = [None, "1,1", "5,2,1"]
N_OBJS = (40, 80, 300)          # both sides of 64 (per-bundle rectangles) and of 96 (large-scene path)
KERNELS = ("hittest", "shade", "shade_and_reflect")
DEPTH = 3

# per scene: direction z of the pinhole grid = -factor * max(W, H) (camera.camera_z ties z to the height alone, and flat or
# tall frames then look past the scene); chosen so that every shape of >= 256 pixels meets the input conditions below
Z_FACTOR = {"s40": 1.5, "s80": 1.0, "s300": 0.8, "tri": 1.0}
MIN_HIT_SHARE, MIN_MISS_SHARE, MIN_RAYS_PER_PIXEL = 0.25, 0.02, 2.0


def shard_tile_rays(shard, W):
    _, rows, rays, _ = shard
    return sharding.tile_rays_for_rows(W, rows) if rows else rays


def camera_z_for(scene, W, H, scale=1.0):
    return float(np.float32(-Z_FACTOR[scene] * scale * max(W, H)))


def pinhole_rays(W, H, z):
    """The reference's pinhole grid with direction z replaced: what rt_set_camera(W, H, z) generates in-kernel."""
    rays = camera.primary_rays(W, H)
    rays["direction"][:, 2] = np.float32(z)
    return rays


def _behind_and_across(seed):
    """Six objects behind the camera plane (z in 3..14, one of them near the axis: what a camera with z > 0 looks at, however narrow) and two across the plane z = 0, off
    the axis so that none contains the origin."""
    rng = np.random.default_rng(seed)
    recs = []
    places = [(rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(3, 14)) for _ in range(5)] + [(0.4, -0.3, 8.0), (5.0, 4.0, 0.0), (-6.0, -3.0, 0.2)]
    for k, pos in enumerate(places):
        mv, inv = instance(pos, rotation(rng.normal(size=3), rng.uniform(0, 6.3)), rng.uniform(0.6, 1.6, size=3))
        mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                         absorption=float(rng.choice([1.0, 0.7, 0.4])), shininess=float(rng.choice([1.0, 5.0, 30.0])))
        recs.append(R.make_object(R.BOX if k % 3 == 0 else R.SPHERE, mat, mv, inv))
    return R.objects_array(recs)


@functools.lru_cache(maxsize=None)
def scene(name):
    """s40: per-bundle rectangles (tile_cull); s80: the small-scene kernel without them; s300: grid, block walk, light tiles
    (three lights, one of them well outside the cloud); tri: 432 triangles (only the grid path knows them)."""
    if name == "s40":
        objs, lights = random_scene(20, 12, 2, seed=11, spread=3.0, zrange=(-16, -6))
        objs = np.concatenate([objs, _behind_and_across(101)])
    elif name == "s80":
        objs, lights = random_scene(45, 27, 2, seed=13, spread=5.0, zrange=(-20, -6))
        objs = np.concatenate([objs, _behind_and_across(102)])
    elif name == "s300":
        objs, lights = random_scene(195, 97, 3, seed=7, spread=8.0, zrange=(-40, -8))
        objs = np.concatenate([objs, _behind_and_across(103)])
        lights["position"][2][:] = (30.0, 25.0, 10.0, 1.0)
    elif name == "tri":
        base, lights = scene_loader.load_scene(str(ROOT / "scenes" / "roundedCube.txt"))
        objs = T.tessellate(base, 4, 8, 2)
        second = lights[:1].copy()
        second["position"][0][:] = (-12.0, 6.0, 2.0, 1.0)
        lights = np.concatenate([lights, second])
    else:
        raise KeyError(name)
    return objs, lights


SCENES = ("s40", "s80", "s300", "tri")


# ---- the predicates -----------------------------------------------------------------------------------------------------
def local_count(n_rays, tile_rays, rank, world, span=1):
    """rt_render.cpp: local_count -work-items of ranks rank .. rank + span - 1 (whole tiles)."""
    if world <= 1:
        return n_rays
    tiles = -(-n_rays // tile_rays)
    rest = tiles % world
    return ((tiles // world) * span + (min(rest - rank, span) if rest > rank else 0)) * tile_rays


def launch_form(W, H, z, n_objs, tile_rays=0, rank=0, world=1, span=1, literal=False, triangles=False):
    """The form do_launch gives a pinhole frame, as a pure function. Mirrors csrc/rt_render.cpp: do_launch (row_tiles, tile2d,
    local_rows, wf_tile_order, tile_cull, bundles_x; the col_shift of the screen tiles and build_screen_tiles' own conditions),
    use_wavefront, local_count; csrc/rt_wavefront.hip: run_wavefront (`padded`, finish_threshold = max(2048, n / 128)) and
    wf_trace_primary_tiles (a wave of 64 work-items in one screen tile, or not). Two things are NOT restated because they
    depend on the scene, not the shape: whether the grid exists (assumed for >= 96 objects) and the 8x8 -> 64x8 fallback when
    the screen tiles exceed their pair budget."""
    n_rays = W * H
    n_local = local_count(n_rays, tile_rays, rank, world, span)
    form = dict(n_local=n_local, empty=n_local == 0, tile2d=False, local_rows=0, tile_order=False, tile_cull=False, partial_bundles=False,
                wavefront=False, screen_tiles=0, straddle=False, padded=False, small=n_local <= 2048)
    if n_local == 0:
        return form
    row_tiles = world <= 1 or (tile_rays % W == 0 and (tile_rays // W) % 8 == 0)
    tile2d = row_tiles and n_local % W == 0
    local_rows = n_local // W if tile2d else 0
    tile_order = tile2d and W % 8 == 0 and local_rows % 8 == 0
    wavefront = triangles or (n_objs >= 96 and not literal)
    col_shift = 3 if tile_order else 6
    screen = col_shift if (wavefront and not literal and z < 0 and W % (1 << col_shift) == 0) else 0
    run_rays = max(tile_rays, 1) * span
    last_run = (n_local - 1) // run_rays
    padded = world > 1 and (last_run * world + rank) * tile_rays + (n_local - last_run * run_rays) > n_rays
    form.update(tile2d=tile2d, local_rows=local_rows, tile_order=tile_order,
                tile_cull=tile2d and 0 < n_objs <= 64 and z < 0 and not literal,
                partial_bundles=tile2d and (W % 8 != 0 or local_rows % 8 != 0),
                wavefront=wavefront, screen_tiles=screen,
                # 64 x 8 tiles under the linear order: a wave is 64 consecutive work-items, in one tile unless a tile of the
                # partition ends inside it (tiles of whole rows of a width that is a multiple of 64 never do)
                straddle=screen == 6 and not tile2d and tile_rays % 64 != 0,
                padded=padded)
    return form


def form_key(form, n_objs):
    """What distinguishes two launches for the kernels that render them."""
    if form["empty"]:
        return ("empty",)
    if form["wavefront"]:
        return ("wavefront", form["tile2d"], form["tile_order"], form["screen_tiles"], form["straddle"], form["padded"], form["small"])
    return ("small-scene", n_objs <= 64, form["tile2d"], form["tile_cull"], form["partial_bundles"], form["padded"])


def pass_forms(W, H, z, n_objs, split, packed=False):
    """render_in_passes (rt_render.cpp): per pass its launch form and how its tiles travel - (form, strided copy, short last run)."""
    spans = [int(s) for s in split.split(",")] if split else ([7, 1] if packed else [3, 1])
    world, tile_rays = sum(spans), 16 * W
    tiles = -(-(W * H) // tile_rays)
    groups, rest = tiles // world, tiles % world
    out, rank = [], 0
    for span in spans:
        form = launch_form(W, H, z, n_objs, tile_rays, rank, world, span)
        out.append((form, groups > 0 and not form["empty"], rest > rank and not form["empty"]))
        rank += span
    return out


def keys_of(W, H, z=-1.0):
    """Every (partition, key) a W x H frame reaches: unsharded and every rank of every shard for each object count, every pass
    of every split for the large scene (only the large-scene path renders in passes)."""
    keys = set()
    for n in N_OBJS:
        keys.add(("whole", form_key(launch_form(W, H, z, n), n)))
        for shard in SHARDS:
            tr = shard_tile_rays(shard, W)
            for rank in range(shard[3]):
                keys.add((shard[0], form_key(launch_form(W, H, z, n, tr, rank, shard[3]), n)))
    for split in SPLITS:
        for packed in (False, True):
            for form, strided, short in pass_forms(W, H, z, 300, split, packed):
                keys.add(("passes", form_key(form, 300), strided, short))
    return keys


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_the_shared_list_reaches_every_reachable_combination():
    widths = sorted(set(range(1, 73)) | {96, 100, 120, 128, 136, 192, 200, 256, 520, 1024, 2049, 2304})
    heights = sorted(set(range(1, 73)) | {75, 88, 97, 100, 128, 144, 225, 256, 512, 1024})
    reachable = {}
    for W in widths:
        for H in heights:
            for k in keys_of(W, H):
                reachable.setdefault(k, (W, H))
    listed = set()
    for W, H in ALL_SHAPES:
        listed |= keys_of(W, H)
    missing = {k: wh for k, wh in reachable.items() if k not in listed}
    assert not missing, f"{len(missing)} of {len(reachable)} reachable combinations are rendered by no listed shape: {missing}"
    assert len(reachable) >= 20
    # both sides of every predicate, on both paths
    wf = [k[1] for k in listed if k[1][0] == "wavefront"]
    for pos, name in ((1, "tile2d"), (2, "tile order"), (4, "straddle"), (5, "padding"), (6, "<= 2048")):
        assert {k[pos] for k in wf} == {False, True}, name
    assert {k[3] for k in wf} == {0, 3, 6}
    small = [k[1] for k in listed if k[1][0] == "small-scene"]
    for pos in range(1, 6):
        assert {k[pos] for k in small} == {False, True}, pos
    assert any(k[1] == ("empty",) for k in listed)
    assert {(k[2], k[3]) for k in listed if k[0] == "passes"} == {(False, False), (True, False), (False, True), (True, True)}


def test_the_mirror_notices_a_flipped_predicate():
    """The coverage assertion is only as good as the mirror: with one predicate of launch_form flipped, forms differ."""
    assert launch_form(64, 9, -1.0, 300)["tile_order"] is False and launch_form(64, 8, -1.0, 300)["tile_order"] is True
    assert launch_form(64, 9, -1.0, 300)["screen_tiles"] == 6 and launch_form(64, 8, -1.0, 300)["screen_tiles"] == 3
    assert launch_form(72, 41, -1.0, 300)["screen_tiles"] == 0 and launch_form(72, 40, 1.0, 300)["screen_tiles"] == 0
    assert launch_form(256, 8, -1.0, 300)["small"] and not launch_form(2049, 1, -1.0, 300)["small"]
    assert launch_form(7, 5, -1.0, 40)["tile_cull"] and not launch_form(7, 5, -1.0, 80)["tile_cull"] and not launch_form(7, 5, 0.0, 40)["tile_cull"]
    assert launch_form(128, 72, -1.0, 300, 4 * 128, 0, 2)["tile2d"] is False and launch_form(128, 72, -1.0, 300, 16 * 128, 0, 3)["tile2d"] is True
    assert launch_form(128, 72, -1.0, 300, 50, 0, 2)["straddle"] and not launch_form(128, 72, -1.0, 300, 4 * 128, 0, 2)["straddle"]
    # 72 rows in tiles of 16: 4.5 tiles; tile 4 (ragged) belongs to rank 1 of 3
    assert [launch_form(128, 72, -1.0, 300, 16 * 128, r, 3)["padded"] for r in range(3)] == [False, True, False]
    assert [launch_form(64, 8, -1.0, 300, 8 * 64, r, 5)["empty"] for r in range(5)] == [False, True, True, True, True]
    for W, H in ALL_SHAPES:   # local_count is the library's rt_local_rays as sharding.py states it
        for shard in SHARDS:
            tr = shard_tile_rays(shard, W)
            for rank in range(shard[3]):
                assert local_count(W * H, tr, rank, shard[3]) == sharding.local_rays(W * H, tr, rank, shard[3])


def test_waves_of_the_linear_order_lie_in_one_screen_tile_or_straddle_two():
    """`straddle` by brute force on the listed frames. An unpadded shard's first-round waves are 64 consecutive work-items: with
    tiles of 4 rows none of them leaves its 64 x 8 screen tile; with tiles of 50 rays some do (unless the frame is one tile wide
    and one tile high), and the listed frames hold both kinds of wave."""
    seen = set()
    for W, H in ALL_SHAPES:
        for shard in SHARDS:
            tr, world = shard_tile_rays(shard, W), shard[3]
            for rank in range(world):
                form = launch_form(W, H, -1.0, 300, tr, rank, world)
                if form["empty"] or form["padded"] or form["screen_tiles"] != 6:
                    continue
                t = np.arange(form["n_local"])
                run = t // tr
                g = (run * world + rank) * tr + (t - run * tr)
                tile = (g // W // 8) * (W // 64) + (g % W) // 64
                kinds = {bool((tile[k:k + 64] != tile[k]).any()) for k in range(0, len(t), 64)}
                assert form["straddle"] or kinds == {False}, (W, H, shard[0], rank)
                if form["straddle"] and (W > 64 or H > 8):
                    assert True in kinds, (W, H, shard[0], rank)
                    seen |= kinds
    assert seen == {False, True}


def test_a_wrong_tile_size_fails_the_stitch():
    """sharding.assemble_frame is what the GPU tests stitch shards with: it must not be forgiving."""
    W, H, world = 64, 40, 3
    frame = np.arange(W * H * 4, dtype=np.float32).reshape(W * H, 4)
    tr = 16 * W
    tiles = sharding.n_tiles(W * H, tr)
    padded = np.concatenate([frame, np.zeros((tiles * tr - W * H, 4), np.float32)]).reshape(tiles, tr, 4)
    pieces = [padded[r::world].reshape(-1, 4) for r in range(world)]
    assert np.array_equal(sharding.assemble_frame(pieces, tr, W * H), frame)
    assert not np.array_equal(sharding.assemble_frame(pieces, 8 * W, W * H), frame)
    assert not np.array_equal(sharding.assemble_frame(pieces[::-1], tr, W * H), frame)


@pytest.mark.parametrize("name", SCENES)
def test_every_listed_frame_sees_the_scene(restatement, name):
    """Conditions on the inputs, from the oracle alone: a frame that misses the scene, or covers it entirely, tests little."""
    objs, lights = scene(name)
    assert {"s40": 0 < len(objs) <= 64, "s80": 64 < len(objs) < 96, "s300": len(objs) >= 96, "tri": 200 <= len(objs) <= 900}[name]
    worst = [1.0, 1.0, 1e9]
    for W, H in ALL_SHAPES:
        if W * H < 256:
            continue
        want = restatement[True].render("shade_and_reflect", objs, lights, pinhole_rays(W, H, camera_z_for(name, W, H)), DEPTH)
        hit = float((want["hit_index"] >= 0).mean())
        per_pixel = want["rays_ref"] / (W * H)
        worst = [min(worst[0], hit), min(worst[1], 1.0 - hit), min(worst[2], per_pixel)]
        assert hit >= MIN_HIT_SHARE and 1.0 - hit >= MIN_MISS_SHARE and per_pixel >= MIN_RAYS_PER_PIXEL, (W, H, hit, per_pixel)
    print(f"{name}: {len(objs)} objects, smallest hit share {worst[0]:.2f}, miss share {worst[1]:.2f}, rays per pixel {worst[2]:.2f}")


@pytest.mark.parametrize("name", ("s40", "s80", "s300"))
def test_a_camera_that_looks_away_still_sees_objects(restatement, name):
    """z > 0 (section C of the lifecycle tests): the objects behind the camera plane make it a frame, not a background."""
    objs, lights = scene(name)
    for W, H in ((96, 96), (36, 50), (9, 1024)):
        want = restatement[True].render("hittest", objs, lights, pinhole_rays(W, H, -camera_z_for(name, W, H)), 0)
        assert 0.02 <= float((want["hit_index"] >= 0).mean()) <= 0.98, (W, H)
