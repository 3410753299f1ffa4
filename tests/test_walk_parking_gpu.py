"""GPU: the block walk's parked candidates (rt_wavefront.hip: block_segment). A lane parks a candidate that passed a block's
pre-test until the wave's next round of exact tests; at a further one it stalls and comes back to the same block, entry by entry
(`cur = b | back << 24`), until a round frees the slot. Written for a walk with a second slot (docs/LOG.md, "Block walk: a second
parking slot" - measured, slower, taken out) and kept for the walk as it is: rays that offer many more candidates in one block
than a lane can park, and remember (`done_k`, a reflection ray's note) only the last one. What a ray hits must not depend on how
its candidates waited, so every case here is, bit for bit, the record walk's (RT_WALK3=0) and the brute-force loop's (grid=False):
 * a cluster of 4 spheres, and of 10 (more than a block holds: the cell's chain), whose centres lie within a quarter radius of
   one point P in the middle of a block cell, in the 1 800-object scene of the block-walk tests: every ray through P offers
   at least 3 (at least 9) candidates in one block or one chain,
 * caller rays through P, queues of 1, 63, 64, 65 and 257 (`hittest`),
 * a depth-3 frame of 64 x 64 rays at the cluster: the later rounds' rays carry a note (the object they leave),
 * under the fused, the unfused and the device-OpenCL arithmetic,
 * and a mesh scene, whose instance has its own copy of the parking code."""
import numpy as np
import pytest

from helpers import R, camera, instance, same_floats
from test_block_walk_gpu import _scene, hip

pytestmark = pytest.mark.gpu
_CACHE = {}
MODES = {"fused": {}, "unfused": dict(fused=False), "device_opencl": dict(device_opencl=True)}
BLOCK_FACTOR = 1.67  # rt_scene.cpp: build_walk_blocks - a block cell's edge in cells of the fine grid; the two share their origin
GUESS = np.array([2.0, 3.0, -55.0])  # where to look for a block cell: the middle of the cloud


def _through(P, r, n, seed):
    """n rays whose lines pass through P (as exactly as float32 allows), from origins between 2 r and 4 r away: outside the cluster's
    spheres (they end 1.25 r from P), inside the cloud of objects, so they do not move the grid's box."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (P + u * rng.uniform(2.0 * r, 4.0 * r, (n, 1))).astype(np.float32).astype(np.float64)
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays["start"][:, 3] = 1.0
    rays["start"][:, :3] = o
    rays["direction"][:, :3] = (P - o) * rng.uniform(0.5, 2.0, (n, 1))
    return rays


def _block_cell(rt):
    gc = rt.grid_constants()
    return float(np.float32(gc["cell"] * BLOCK_FACTOR)), np.asarray(gc["box_lo"], dtype=np.float64)[:3]


def _with_cluster(base, n_cluster, P, r, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n_cluster, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centres = P + u * rng.uniform(0.0, 0.25 * r, (n_cluster, 1))
    recs = []
    for c in centres:
        mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                         absorption=float(rng.choice([1.0, 0.5])), reflection=0.0, shininess=8.0)
        recs.append(R.make_object(R.SPHERE, mat, *instance(c, None, np.full(3, r))))
    return np.concatenate([base, R.objects_array(recs)]), centres


def _free_block_cell(bc, lo, spheres):
    """the centre of the block cell nearest the guess that no other object comes near: nothing within 0.4 of a cell's edge of it (the
    cluster's radius is a twelfth of the edge and the rays start within four radii), so that the rays meet the cluster and nothing else first"""
    others = spheres[np.isfinite(spheres[:, 3]) & (spheres[:, 3] > 0)]
    i0 = np.floor((GUESS - lo) / bc)
    steps = sorted(((dx, dy, dz) for dx in range(-4, 5) for dy in range(-4, 5) for dz in range(-4, 5)), key=lambda s: (s[0] ** 2 + s[1] ** 2 + s[2] ** 2, s))
    for step in steps:
        P = lo + (i0 + np.array(step) + 0.5) * bc
        if (np.linalg.norm(others[:, :3] - P, axis=1) - others[:, 3]).min() >= 0.4 * bc:
            return P
    raise AssertionError("no free block cell near the middle of the cloud")


def cluster_scene(n_cluster):
    """The scene with its cluster, where the cluster is, and an eye for the frame. The grid's cell depends on the scene, so P is found
    in two passes: the cluster at a guess, the grid's constants read back, the cluster moved to the middle of a block cell - and
    the constants read again. Every render then checks that P is in the middle of a block cell of the scene as rendered."""
    if n_cluster in _CACHE:
        return _CACHE[n_cluster]
    if "base" not in _CACHE:
        _CACHE["base"] = _scene(np.random.default_rng(11), 1800, 4, 40, lights=3)
    base, lights = _CACHE["base"]
    P, r = GUESS, 0.3
    for _ in range(2):
        objs, centres = _with_cluster(base, n_cluster, P, r, seed=n_cluster)
        with hip(objs, lights, _through(P, r, 257, seed=1), 0, kernel="hittest") as rt:
            bc, lo = _block_cell(rt)
            spheres = rt.grid_spheres()[:len(base)]
        P = _free_block_cell(bc, lo, spheres)
        r = bc / 12.0
    objs, centres = _with_cluster(base, n_cluster, P, r, seed=n_cluster)
    eye = P + 4.0 * r * np.array([0.48, 0.6, 0.64])
    _CACHE[n_cluster] = dict(objs=objs, lights=lights, P=P, r=r, bc=bc, centres=centres, eye=eye, ids=np.arange(len(base), len(objs)))
    return _CACHE[n_cluster]


def assert_cluster_in_one_block_cell(rt, sc):
    """P within 0.2 of a cell's edge of a block cell's centre, and the spheres (1.25 r around P) within 0.4 of it"""
    bc, lo = _block_cell(rt)
    off = np.abs(((sc["P"] - lo) / bc) % 1.0 - 0.5)
    assert off.max() <= 0.2 and 1.25 * sc["r"] <= 0.2 * bc, (off, sc["r"], bc)


def lines_within_radius(rays, centres, r):
    """per ray: the number of cluster spheres whose centre its LINE passes within the true radius r of"""
    o = rays["start"][:, None, :3].astype(np.float64)
    d = rays["direction"][:, None, :3].astype(np.float64)
    oc = centres[None, :, :] - o
    dist = np.linalg.norm(np.cross(oc, np.broadcast_to(d, oc.shape)), axis=2) / np.linalg.norm(d, axis=2)
    return (dist < r).sum(axis=1)


def hittest(sc, rays, env, grid, kw, monkeypatch):
    monkeypatch.delenv("RT_WALK3", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with hip(sc["objs"], sc["lights"], rays, 0, kernel="hittest", grid=grid, **kw) as rt:
        t, idx = rt.render_aux()
        st = rt.count_rays()
        if grid:
            info = rt.rays_info()
            assert info["grid_in_use"] == 1 and info["literal"] == 0, info
            assert_cluster_in_one_block_cell(rt, sc)
    monkeypatch.delenv("RT_WALK3", raising=False)
    return t.view(np.uint32).copy(), idx.copy(), (st.rays_reference, st.rays_traced, st.hit_pixels)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_cluster,need", [(4, 3), (10, 9)])
def test_rays_through_a_cluster_offer_more_than_a_lane_can_park(monkeypatch, n_cluster, need, n, mode):
    sc = cluster_scene(n_cluster)
    rays = _through(sc["P"], sc["r"], n, seed=100 * n_cluster + n)
    near = lines_within_radius(rays, sc["centres"], sc["r"])
    assert near.min() >= need, f"a ray's line passes only {near.min()} of the {n_cluster} spheres"  # (a condition on the inputs)
    got = hittest(sc, rays, {}, True, MODES[mode], monkeypatch)
    records = hittest(sc, rays, {"RT_WALK3": "0"}, True, MODES[mode], monkeypatch)
    brute = hittest(sc, rays, {}, False, MODES[mode], monkeypatch)
    on_cluster = np.isin(got[1], sc["ids"]).sum()
    print(f"{n_cluster} spheres, {n} rays, {mode}: {on_cluster} hit the cluster, lines pass {near.min()} .. {near.max()} spheres, counters {got[2]}")
    for want, name in ((records, "RT_WALK3=0"), (brute, "grid=False")):
        assert np.array_equal(got[1], want[1]), f"{name}: {(got[1] != want[1]).sum()} hit indices differ"
        assert same_floats(got[0].view(np.float32), want[0].view(np.float32)), f"{name}: t differs"
        assert got[2] == want[2], f"{name}: counters {got[2]} against {want[2]}"
    assert on_cluster * 2 >= n, "the rays were meant to hit the cluster"


def frame_rays(sc, W=64, H=64):
    """W x H rays from the eye through a window of 3 r x 3 r around P"""
    d = sc["P"] - sc["eye"]
    a = np.cross(d, [0.3, 1.0, 0.2])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    b /= np.linalg.norm(b)
    x, y = np.meshgrid((np.arange(W) + 0.5) / W - 0.5, (np.arange(H) + 0.5) / H - 0.5)
    tgt = sc["P"] + 3.0 * sc["r"] * (x.reshape(-1, 1) * a + y.reshape(-1, 1) * b)
    rays = np.zeros(W * H, dtype=R.RAY_DTYPE)
    rays["start"][:, 3] = 1.0
    rays["start"][:, :3] = sc["eye"]
    rays["direction"][:, :3] = tgt - rays["start"][:, :3].astype(np.float64)
    return rays


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_cluster", [4, 10])
def test_a_reflecting_frame_at_the_cluster(monkeypatch, n_cluster, mode):
    sc = cluster_scene(n_cluster)
    rays = frame_rays(sc)
    got = {}
    for name, env, grid in (("blocks", {}, True), ("records", {"RT_WALK3": "0"}, True), ("brute", {}, False)):
        monkeypatch.delenv("RT_WALK3", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with hip(sc["objs"], sc["lights"], rays, 3, kernel="shade_and_reflect", grid=grid, **MODES[mode]) as rt:
            frame = rt.Render().view(np.uint32).copy()
            t, idx = rt.render_aux()
            st = rt.count_rays()
            if grid:
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, info
                assert_cluster_in_one_block_cell(rt, sc)
        got[name] = (frame, t.view(np.uint32).copy(), idx.copy(), st.rays_reference, st.rays_traced, st.hit_pixels)
    monkeypatch.delenv("RT_WALK3", raising=False)
    on_cluster = int(np.isin(got["brute"][2], sc["ids"]).sum())
    print(f"{n_cluster} spheres, {mode}: {on_cluster} of {len(rays)} primary rays hit the cluster, rays_traced {got['brute'][4]}, hit_pixels {got['brute'][5]}")
    assert on_cluster >= len(rays) // 4, "the frame was meant to look at the cluster"
    # (every primary hit sends a reflection ray, which carries a note, into round 2)
    assert got["brute"][4] >= len(rays) + on_cluster, "the frame has no later rounds to speak of"
    for name in ("records", "brute"):
        for a, b, what in zip(got["blocks"], got[name], ("frame", "aux_t", "aux_index", "rays_reference", "rays_traced", "hit_pixels")):
            assert np.array_equal(a, b), f"{mode}: {what} differs from {name}"


def test_a_mesh_scene_agrees_with_the_record_walk(monkeypatch):
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
            frame = rt.Render().view(np.uint32).copy()
            st = rt.count_rays()
            assert st.wavefront == 1
        got[name] = (frame, st.rays_traced, st.rays_reference, st.hit_pixels)
    monkeypatch.delenv("RT_WALK3", raising=False)
    assert got["blocks"][3] > 500
    for a, b in zip(got["blocks"], got["records"]):
        assert np.array_equal(a, b)
