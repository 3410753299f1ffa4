"""GPU: the block walk's stash of prepared rays (rt_wavefront.hip: block_segment; rt_walk_stash.h) - rays are set up 64 queue
entries at a time into LDS and copied out by the lanes that fall idle. A ray's result must not depend on the way it reached its
lane, so every case here is the brute-force loop's (t, index) or frame, bit for bit:
 * queues that end inside, at and just after a batch of 64, and queues long enough for runs of 128 and 256 entries drawn from
   the ticket counters (several batches per run, a ragged last batch),
 * slots that start no walk between ones that do: NaN reflection rays in the later rounds of a frame (the one kind that
   reaches the prepare; a caller's buffer of such rays makes the whole frame literal, which is checked too),
 * an always-tested object (what it found travels with the slot's taker),
 * the later rounds of a reflecting frame, under the three arithmetics' flags,
 * triangles, whose instance keeps the hand-out by idle lanes."""
import numpy as np
import pytest

from helpers import R, camera, same_floats
from test_block_walk_gpu import _rays, _scene, hip

pytestmark = pytest.mark.gpu
_CACHE = {}


def awkward_scene():
    if "scene" not in _CACHE:
        _CACHE["scene"] = _scene(np.random.default_rng(5), 2500, 9, 60)
    return _CACHE["scene"]


def hittest(objs, lights, rays, grid, walked=True):
    """(t, index) of caller-made rays. With the grid, the frame must really go through the grid's walks (rays_info: the grid in
    use, the frame not switched to the literal loops by rt_create's scan of the rays) unless the caller says it does not."""
    with hip(objs, lights, rays, 0, kernel="hittest", grid=grid) as rt:
        t, idx = rt.render_aux()
        info = rt.rays_info()
        assert rt.stats().pinhole == 0 and (rt.stats().wavefront == 1 or not grid)  # (a small scene's brute force is the small-scene kernel)
        if grid:
            assert (info["grid_in_use"] == 1 and info["literal"] == 0) == walked, info
    return t, idx


def assert_same_hits(got, want, label):
    assert np.array_equal(got[1], want[1]), f"{label}: {(got[1] != want[1]).sum()} hit indices differ"
    assert same_floats(got[0], want[0]), label


def inside_rays(n, seed=17):
    rays = _rays(np.random.default_rng(seed), n, "inside")
    rays["direction"] = rays["direction"].astype(np.float32)
    return rays


def assert_hits_and_misses(idx, label):
    share = (idx >= 0).mean()
    print(f"{label}: hit share {share:.3f} of {len(idx)} rays")
    assert share >= 0.10 and 1.0 - share >= 0.10, f"{label}: hit share {share:.3f}"


def test_the_population_hits_and_misses():
    """8 192 `inside` rays on the awkward scene hit 15.9 % of the time on the CPU oracle: both outcomes are well represented."""
    objs, lights = awkward_scene()
    _, idx = hittest(objs, lights, inside_rays(8192), grid=False)
    assert_hits_and_misses(idx, "8192 inside rays, brute force")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_queues_around_a_batch_of_64(n):
    objs, lights = awkward_scene()
    rays = inside_rays(n, seed=100 + n)
    assert_same_hits(hittest(objs, lights, rays, True), hittest(objs, lights, rays, False), f"{n} rays")


@pytest.mark.parametrize("n", [16384 + 37, 32768 + 37])
def test_runs_of_128_and_256_entries_drawn_by_64_waves(monkeypatch, n):
    """With 64 launched waves these are the smallest queues cut in runs of 128 and of 256 entries (RunCursor::begin: n >= 2 x waves
    x run): several batches per run, runs drawn from the ticket counters, a ragged last batch."""
    objs, lights = awkward_scene()
    rays = inside_rays(n, seed=n)
    want = hittest(objs, lights, rays, False)
    assert_hits_and_misses(want[1], f"{n} rays, brute force")
    monkeypatch.setenv("RT_WAVES_CLOSEST", "64")
    assert_same_hits(hittest(objs, lights, rays, True), want, f"{n} rays, 64 waves")


def test_a_buffer_of_rays_the_walk_is_not_made_for_never_reaches_it(monkeypatch):
    """Every eighth ray with a NaN in it, every eighth past the grid box, every eighth a `scaled` ray of the block-walk tests (|d| of
    1e-20 ... 1e17), the rest `inside` rays: the results are brute force's - but NOT by way of the stash. rt_create's scan of a
    caller's buffer finds directions outside the walk's window and renders the whole frame with the literal loops; a NaN origin
    leaves no grid at all; and the origins of a buffer are united into the grid's box, so no first-round ray can miss it. Of the
    three kinds of slot that start no walk only one can therefore reach the prepare: a ray with a NaN in it, in a later round
    (test_nan_reflection_rays_between_ones_that_start). A miss of the grid box and the test-everything case would need a
    later-round ray that starts outside the box or whose |d|^2 left (1e-30, 1e30): hit points lie inside the box and a reflection
    keeps its ray's length. Those two branches stay as the parent had them, for a caller this scan does not know."""
    objs, lights = awkward_scene()
    n = 32768 + 37
    rng = np.random.default_rng(41)
    rays = inside_rays(n, seed=43)
    k = np.arange(n)
    nan = k % 8 == 1
    rays["direction"][nan, rng.integers(0, 3, nan.sum())] = np.nan
    rays["start"][k % 16 == 9, 1] = np.nan                     # (half of them in the origin as well)
    off = k % 8 == 3                                           # far from the cloud and pointing away from it
    rays["start"][off, :3] = rng.uniform([200, -30, -90], [400, 30, -25], (off.sum(), 3))
    rays["direction"][off, :3] = np.abs(rng.normal(size=(off.sum(), 3))) * [1, 0.1, 0.1] + [0.5, 0, 0]
    scaled = _rays(rng, n, "scaled")
    with np.errstate(all="ignore"):
        scaled["direction"] = scaled["direction"].astype(np.float32)
    sc = k % 8 == 5
    rays[sc] = scaled[sc]
    assert nan.sum() > 4000 and off.sum() > 4000 and sc.sum() > 4000
    want = hittest(objs, lights, rays, False)
    assert (want[1][off] == -1).all(), "the rays meant to miss the cloud hit something"
    monkeypatch.setenv("RT_WAVES_CLOSEST", "64")
    assert_same_hits(hittest(objs, lights, rays, True, walked=False), want, "mixed buffer")
    assert (want[1][~(nan | off | sc)] >= 0).mean() >= 0.10


@pytest.mark.parametrize("name", ["fuzz seed 45", "tiny far box"])
def test_nan_reflection_rays_between_ones_that_start(name):
    """Slots that start no walk, where they do occur: a box normal that comes out zero makes a NaN reflection ray under the default
    arithmetic (tests/test_device_opencl_fuzz_gpu.py: test_zero_box_normal, whose two scenes these are), so the closest-hit queues
    of rounds 2 and 3 hold rays with a NaN between rays that walk. walk_begin leaves such a ray's cell unset; its slot must say
    "does not start" whatever stands there, and the lane that takes it stores the miss and stays idle. The grid is in use and the
    frame is not literal; frame, t, index and ray counts are brute force's; and the NaN route is really taken (a sphere no ray
    can reach, appended to the scene, changes pixels: the reference shades a NaN ray with the LAST object)."""
    import test_device_opencl_fuzz_gpu as F
    from helpers import clear_lights
    if name == "fuzz seed 45":
        objs, lights, rays = F.fuzz_scene(np.random.default_rng(1000 + 45))
        lights, _ = clear_lights(objs, lights, np.random.default_rng(45))
    else:
        objs, lights, rays = F.tiny_far_box_scene()
    got = {}
    for grid in (True, False):
        with hip(objs, lights, rays, 3, kernel="shade_and_reflect", path="wavefront", grid=grid) as rt:
            frame = rt.Render().copy()
            t, idx = rt.render_aux()
            st = rt.count_rays()
            if grid:
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, info
        got[grid] = (frame.view(np.uint32), t.copy(), idx.copy(), st.rays_traced, st.rays_reference, st.hit_pixels)
    assert np.array_equal(got[True][0], got[False][0]), f"{name}: {(got[True][0] != got[False][0]).any(axis=1).sum()} pixels differ"
    assert np.array_equal(got[True][2], got[False][2]) and same_floats(got[True][1], got[False][1])
    assert got[True][3:] == got[False][3:]
    probe = F.obj(R.SPHERE, (0.0, 0.0, 5.0e4), 1.0, seed=99)
    with hip(R.objects_array(list(objs) + [probe]), lights, rays, 3, kernel="shade_and_reflect", path="wavefront") as rt:
        probed = rt.Render().view(np.uint32)
    routed = int((probed != got[True][0]).any(axis=1).sum())
    print(f"{name}: {routed} pixels take the NaN-ray route, {got[True][3]} rays traced")
    assert routed > 0


def test_an_always_tested_object_travels_with_the_slot():
    """scene_partial's far walls are far larger than any cell span the grid registers: every ray tests them before its walk,
    and what that test found (T, index, sphere bit) is the state the walk starts from."""
    from test_primary_depth_order_gpu import lights as wall_lights, scene_partial
    objs, lights = scene_partial(), wall_lights()
    rng = np.random.default_rng(3)
    n = 4096 + 19
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays["start"][:, 3] = 1.0
    rays["start"][:, :3] = rng.uniform([-6, -4, -20], [6, 4, 0], (n, 3))
    tgt = rng.uniform([-25, -15, -110], [25, 15, -14], (n, 3))
    near = np.arange(n) % 3 == 0                                # a third aimed into the sphere of radius 0.9 in front of the walls
    tgt[near] = np.array([-2.0, 1.0, -16.0]) + rng.uniform(-0.6, 0.6, (near.sum(), 3))
    rays["direction"][:, :3] = ((tgt - rays["start"][:, :3]) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    with hip(objs, lights, rays, 0, kernel="hittest") as rt:  # (registered with an infinite radius = on the always-list; as tests/test_pose_tiles_gpu.py reads it)
        n_always = int(np.isposinf(rt.grid_spheres()[:, 3]).sum())
    assert n_always > 0, "no object of this scene is tested by every ray"
    want = hittest(objs, lights, rays, False)
    walls = np.isin(want[1], np.arange(len(objs))[-6:-2])
    assert walls.sum() > 500 and (~walls & (want[1] >= 0)).sum() > 100
    assert_same_hits(hittest(objs, lights, rays, True), want, "always-list")


@pytest.mark.parametrize("mode", ["fused", "unfused", "device_opencl"])
def test_later_rounds_of_a_reflecting_frame(monkeypatch, mode):
    kw = {"fused": {}, "unfused": dict(fused=False), "device_opencl": dict(device_opencl=True)}[mode]
    if "frame_scene" not in _CACHE:
        _CACHE["frame_scene"] = _scene(np.random.default_rng(11), 1800, 4, 40, lights=3)
    objs, lights = _CACHE["frame_scene"]
    rays = camera.primary_rays(160, 120)
    got = {}
    for name, env, grid in (("blocks", {}, True), ("records", {"RT_WALK3": "0"}, True), ("brute", {}, False)):
        monkeypatch.delenv("RT_WALK3", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with hip(objs, lights, rays, 3, grid=grid, **kw) as rt:
            frame = rt.Render()
            t, idx = rt.render_aux()
            st = rt.count_rays()
        got[name] = (frame.view(np.uint32), t.view(np.uint32), idx, st.rays_traced, st.hit_pixels)
    monkeypatch.delenv("RT_WALK3", raising=False)
    print(f"{mode}: rays_traced {got['brute'][3]}, hit_pixels {got['brute'][4]}")
    assert got["brute"][3] > 160 * 120 + 2 * got["brute"][4], "the frame has no later rounds to speak of"
    for name in ("records", "brute"):
        for a, b, what in zip(got["blocks"], got[name], ("frame", "aux_t", "aux_index", "rays_traced", "hit_pixels")):
            assert np.array_equal(a, b), f"{mode}: {what} differs from {name}"


def test_triangles_keep_their_hand_out(monkeypatch):
    from test_frame_shapes_cpu import scene
    objs, lights = scene("tri")
    W, H = 96, 96
    z = float(camera.camera_z(H))
    got = {}
    for name, env in (("blocks", None), ("records", "0")):
        monkeypatch.delenv("RT_WALK3", raising=False)
        if env is not None:
            monkeypatch.setenv("RT_WALK3", env)
        with hip(objs, lights, None, 3, camera=(W, H, z)) as rt:
            frame = rt.Render()
            st = rt.count_rays()
            assert st.wavefront == 1
        got[name] = (frame.view(np.uint32), st.rays_traced, st.rays_reference, st.hit_pixels)
    monkeypatch.delenv("RT_WALK3", raising=False)
    assert got["blocks"][3] > 500
    for a, b in zip(got["blocks"], got["records"]):
        assert np.array_equal(a, b)
