"""GPU: the 16-byte reflection record (rt_wavefront.hip: reflection_rays_rebuilt). Where the block walk serves a frame without
triangles that has lights, a reflection ray in flight is stored as its direction and one word, and every reader - the walk's
prepare, wf_resume, wf_finish - rebuilds its start from the hit the pixel keeps in its F_PX block. Everywhere else (the record
walk under RT_WALK3=0, brute force, meshes, no lights, literal frames) the 32-byte ray is stored as before. Both forms live in
one library, chosen per frame, and a frame must not depend on the form: every case here is bit for bit - frame, t, index, ray
counts - the frame of a path that keeps the 32-byte record.

Every grid render asserts through rays_info() that the grid is in use and the frame is not literal. Frames are small, and a
small frame is handed to wf_finish after its first round (at most 2 048 live pixels); so that the rounds themselves - the walk's
prepare and wf_resume - read the records, most cases render with RT_WF_FINISH_THRESHOLD=0 ("rounds"), which keeps wf_finish out
of the frame, and the tail cases render with the default ("tail")."""
import numpy as np
import pytest

from helpers import R, camera, instance, same_floats
from test_block_walk_gpu import _scene, hip

pytestmark = pytest.mark.gpu
_CACHE = {}
MODES = {"fused": {}, "unfused": dict(fused=False), "device_opencl": dict(device_opencl=True)}
ENV = ("RT_WALK3", "RT_WF_FINISH_THRESHOLD")
W, H = 64, 64


def cloud(lights=3):
    """test_block_walk_gpu's 1 800-object scene: small spheres and boxes, four objects several cells across, one crowded cell"""
    if ("cloud", lights) not in _CACHE:
        objs, ls = _scene(np.random.default_rng(11), 1800, 4, 40, lights=max(lights, 1))
        _CACHE[("cloud", lights)] = (objs, ls[:lights])
    return _CACHE[("cloud", lights)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(monkeypatch, objs, lights, rays, depth, walk="blocks", tail=False, **kw):
    """One frame and its counted pass. walk: "blocks" (the 16-byte record where its conditions hold), "records" (RT_WALK3=0: the
    record walk and the 32-byte record) or "brute" (no grid)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = walk != "brute"
    if walk == "records":
        monkeypatch.setenv("RT_WALK3", "0")
    if grid and not tail:
        monkeypatch.setenv("RT_WF_FINISH_THRESHOLD", "0")
    kw.setdefault("path", "wavefront")
    try:
        with hip(objs, lights, rays, depth, grid=grid, **kw) as rt:
            frame = rt.Render().copy()
            t, idx = rt.render_aux()
            st = rt.count_rays()
            assert st.wavefront == 1
            if grid:
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, info
            return dict(frame=bits(frame), t=t.copy(), idx=idx.copy(), traced=int(st.rays_traced), reference=int(st.rays_reference),
                        hits=int(st.hit_pixels), rounds=int(st.rounds))
    finally:
        for k in ENV:
            monkeypatch.delenv(k, raising=False)


def assert_same(got, want, label):
    assert np.array_equal(got["idx"], want["idx"]), f"{label}: {(got['idx'] != want['idx']).sum()} hit indices differ"
    assert same_floats(got["t"], want["t"]), f"{label}: t"
    assert np.array_equal(got["frame"], want["frame"]), f"{label}: {(got['frame'] != want['frame']).reshape(len(got['idx']), -1).any(axis=1).sum()} pixels differ"
    for k in ("traced", "reference", "hits"):
        assert got[k] == want[k], f"{label}: {k} {got[k]} != {want[k]}"


def reflecting_hits(objs, res):
    """Primary hits that send a reflection ray at depth > 0: begin_shade_lit's condition is the hit object's absorption <= 0.999."""
    hit = res["idx"][res["idx"] >= 0]
    return int((objs["absorption"][hit] <= 0.999).sum())


# ---- both forms in one library ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_both_record_forms_and_brute_force_give_one_frame(monkeypatch, mode):
    objs, lights = cloud()
    rays = camera.primary_rays(W, H)
    got = {walk: render(monkeypatch, objs, lights, rays, 3, walk, **MODES[mode]) for walk in ("blocks", "records", "brute")}
    print(f"{mode}: traced {got['brute']['traced']}, hit pixels {got['brute']['hits']}, rounds {got['blocks']['rounds']}")
    assert reflecting_hits(objs, got["brute"]) > 200, "the frame has no reflection rays to speak of"
    assert got["blocks"]["rounds"] >= 5, "the frame's rounds did not run as rounds"  # (depth + 2)
    assert_same(got["blocks"], got["records"], f"{mode}: 16-byte against 32-byte records")
    assert_same(got["blocks"], got["brute"], f"{mode}: 16-byte records against brute force")


# ---- depth and lights ---------------------------------------------------------------------------------------------------------
def plates_scene():
    """The cloud with forty thin plates in front of it, facing the camera, and three lights of which the LAST stands behind the
    whole scene. A plate is thinner than the 0.01 a shadow ray starts off its hit, so the ray to the last light starts behind the
    plate: the hit is lit with nDotL <= 0, the backward light scan goes on to an earlier light - a stale-specular scan - and that
    takes further rounds while the hit's reflection record stays parked."""
    if "plates" not in _CACHE:
        objs, _ = cloud()
        rng = np.random.default_rng(29)
        plates = []
        for _k in range(40):
            mv, inv = instance(rng.uniform([-9, -9, -23], [9, 9, -17]), None, (2.5, 2.5, 0.001))
            mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3), absorption=0.5,
                             reflection=0.0, shininess=20.0)
            plates.append(R.make_object(R.BOX, mat, mv, inv))
        props = R.LightProperties((.1, .1, .1), (.5, .5, .5), (.5, .5, .5))
        ls = R.lights_array([R.make_light(props, position=p) for p in ((-30.0, 20.0, 10.0, 1.0), (25.0, -15.0, 5.0, 1.0), (3.0, 2.0, -200.0, 1.0))])
        _CACHE["plates"] = (np.concatenate([objs, R.objects_array(plates)]), ls)
    return _CACHE["plates"]


@pytest.mark.parametrize("kind", ["no lights", "one light", "three lights, scans"])
def test_depths_and_lights(monkeypatch, kind):
    """No lights: the hit starts no light loop and loop_step emits the reflection ray itself - the frame keeps the 32-byte record.
    One light, three lights: the ray leaves with its hit's first shadow ray, as a 16-byte record."""
    if kind == "three lights, scans":
        objs, lights = plates_scene()
    else:
        objs, lights = cloud(0 if kind == "no lights" else 1)
    rays = camera.primary_rays(W, H)
    for depth in (0, 1, 3, 5):
        got = render(monkeypatch, objs, lights, rays, depth)
        want = render(monkeypatch, objs, lights, rays, depth, "brute")
        assert_same(got, want, f"{kind}, depth {depth}")
        shadow = 0 if kind == "no lights" else want["hits"]
        print(f"{kind}, depth {depth}: traced {want['traced']}, hit pixels {want['hits']}, rounds {got['rounds']}")
        assert reflecting_hits(objs, want) > 200
        if kind != "three lights, scans":  # (primary rays + one shadow ray per primary hit, where there is a light; beyond that: reflection rays and theirs)
            assert (want["traced"] > W * H + shadow) == (depth > 0), f"{kind}, depth {depth}: reflection rays"
        if kind == "three lights, scans":
            # With the last light alone every shaded hit takes exactly one shadow ray and the hits are the same ones (what is hit
            # and what reflects does not depend on the lights): whatever three lights trace beyond that is a scan going on.
            alone = render(monkeypatch, objs, lights[2:], rays, depth, "brute")
            scans = want["traced"] - alone["traced"]
            print(f"    stale-specular scan rays: {scans}")
            assert scans > 50, f"depth {depth}: the scene makes no stale-specular scans"
            if depth > 0:
                assert got["rounds"] > depth + 2, f"depth {depth}: no scan went on into a further round"


# ---- batch edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_reflection_queues_around_a_batch_of_64(monkeypatch, n):
    """n primary rays that all hit an object whose absorption lets the reflection ray leave: round 2's closest-hit queue holds
    exactly n 16-byte records, which the prepare takes 64 at a time."""
    objs, lights = cloud()
    pool = camera.primary_rays(W, H)
    if "pool_idx" not in _CACHE:
        with hip(objs, lights, pool, 0, kernel="hittest", grid=False) as rt:
            _CACHE["pool_idx"] = rt.render_aux()[1].copy()
    idx = _CACHE["pool_idx"]
    sends = (idx >= 0) & (objs["absorption"][np.maximum(idx, 0)] <= 0.5)
    assert sends.sum() >= 257
    rays = pool[np.nonzero(sends)[0][:n]]
    got = render(monkeypatch, objs, lights, rays, 2)
    want = render(monkeypatch, objs, lights, rays, 2, "brute")
    assert want["hits"] == n
    assert want["traced"] >= 3 * n  # (primary, first shadow ray, reflection ray)
    assert_same(got, want, f"{n} reflection rays")


# ---- NaN reflection rays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [False, True], ids=["rounds", "tail"])
@pytest.mark.parametrize("name", ["fuzz seed 45", "tiny far box"])
def test_nan_reflection_rays(monkeypatch, name, tail):
    """A box normal that comes out zero makes a NaN reflection vector under the default arithmetic (test_device_opencl_fuzz_gpu.py:
    test_zero_box_normal, whose two scenes these are): the record holds NaN, the rebuilt start is NaN, and the slot starts no walk."""
    import test_device_opencl_fuzz_gpu as F
    from helpers import clear_lights
    if name == "fuzz seed 45":
        objs, lights, rays = F.fuzz_scene(np.random.default_rng(1000 + 45))
        lights, _ = clear_lights(objs, lights, np.random.default_rng(45))
    else:
        objs, lights, rays = F.tiny_far_box_scene()
    assert len(lights) > 0
    got = render(monkeypatch, objs, lights, rays, 3, tail=tail)
    want = render(monkeypatch, objs, lights, rays, 3, "brute")
    assert_same(got, want, name)
    probe = F.obj(R.SPHERE, (0.0, 0.0, 5.0e4), 1.0, seed=99)   # (the reference shades a NaN ray with the LAST object: a sphere no ray can reach changes pixels)
    probed = render(monkeypatch, R.objects_array(list(objs) + [probe]), lights, rays, 3, tail=tail)
    routed = int((probed["frame"] != got["frame"]).reshape(len(got["idx"]), -1).any(axis=1).sum())
    print(f"{name}: {routed} pixels take the NaN-ray route")
    assert routed > 0


# ---- the always-list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [False, True], ids=["rounds", "tail"])
def test_always_tested_objects(monkeypatch, tail):
    """scene_partial's far walls are tested by every ray before its walk. In the tail, an always-list sends wf_finish's closest-hit
    rays through the fine grid instead of the blocks: that reader takes the 16-byte record too."""
    from test_primary_depth_order_gpu import lights as wall_lights, scene_partial
    objs, lights = scene_partial(), wall_lights()
    rays = camera.primary_rays(64, 48)
    with hip(objs, lights, rays, 0, kernel="hittest") as rt:
        n_always = int(np.isposinf(rt.grid_spheres()[:, 3]).sum())
    assert n_always > 0, "no object of this scene is on the always-list"
    got = render(monkeypatch, objs, lights, rays, 3, tail=tail)
    want = render(monkeypatch, objs, lights, rays, 3, "brute")
    hit = want["idx"][want["idx"] >= 0]
    walls = np.isin(hit, np.arange(len(objs))[-6:-2])
    assert walls.sum() > 500 and (objs["absorption"][hit] <= 0.999).sum() > 500, "too few hits send a reflection ray"
    assert_same(got, want, "always-list")


# ---- triangles keep the 32-byte record ----------------------------------------------------------------------------------------
def test_triangles_keep_the_32_byte_record(monkeypatch):
    from test_frame_shapes_cpu import scene
    objs, lights = scene("tri")
    assert int((objs["type"] == 2).sum()) == 432   # (a frame with triangles rebuilds neither its shadow nor its reflection rays)
    z = float(camera.camera_z(96))
    got = render(monkeypatch, objs, lights, None, 3, camera=(96, 96, z))
    want = render(monkeypatch, objs, lights, None, 3, "records", camera=(96, 96, z))
    assert got["hits"] > 500 and reflecting_hits(objs, got) > 100
    assert_same(got, want, "triangles")


# ---- the tail: wf_finish traces and resumes over 16-byte records --------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_the_tail_of_a_small_frame(monkeypatch, mode):
    objs, lights = plates_scene()
    rays = camera.primary_rays(40, 32)   # 1 280 work-items: at most 2 048 live after round 1 - the rest of the frame is wf_finish's
    got = render(monkeypatch, objs, lights, rays, 3, tail=True, **MODES[mode])
    want = render(monkeypatch, objs, lights, rays, 3, "brute", **MODES[mode])
    assert got["rounds"] == 1, "the frame was not handed to wf_finish after its first round"
    assert reflecting_hits(objs, want) > 50
    assert_same(got, want, f"{mode}: tail")


# ---- one case each on a live context ------------------------------------------------------------------------------------------
def test_after_a_reflecting_object_has_moved(monkeypatch):
    objs, lights = cloud()
    rays = camera.primary_rays(W, H)
    before = render(monkeypatch, objs, lights, rays, 3, "brute")
    seen, counts = np.unique(before["idx"][before["idx"] >= 0], return_counts=True)
    reflecting = objs["absorption"][seen] <= 0.5
    a = int(seen[reflecting][np.argmax(counts[reflecting])])   # the reflecting object that covers most pixels: reflection rays leave it
    mv = objs["mv"][a].reshape(4, 4).T.astype(np.float64)
    mv[:3, 3] += (0.7, -0.4, 0.5)
    t = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
    t["mv"][0], t["mvInverse"][0] = mv.T.astype(np.float32).reshape(16), np.linalg.inv(mv).T.astype(np.float32).reshape(16)
    want = render(monkeypatch, R.with_transforms(objs, t, a), lights, rays, 3, "brute")
    assert not np.array_equal(want["frame"], before["frame"]) and (want["idx"] == a).sum() > 0
    monkeypatch.setenv("RT_WF_FINISH_THRESHOLD", "0")
    with hip(objs, lights, rays, 3, path="wavefront") as rt:
        first = bits(rt.Render().copy())
        rt.set_transforms(t, a)
        frame = bits(rt.Render().copy())
        t_aux, idx = rt.render_aux()
        st = rt.count_rays()
        info = rt.rays_info()
        assert info["grid_in_use"] == 1 and info["literal"] == 0, info
    monkeypatch.delenv("RT_WF_FINISH_THRESHOLD")
    assert np.array_equal(first, before["frame"])
    assert_same(dict(frame=frame, t=t_aux, idx=idx, traced=int(st.rays_traced), reference=int(st.rays_reference), hits=int(st.hit_pixels)), want, "moved")


def test_a_two_shard_frame(monkeypatch):
    import torch
    from opencl_raytracer_amd import sharding
    objs, lights = cloud()
    z = float(camera.camera_z(H))
    want = render(monkeypatch, objs, lights, None, 3, "brute", camera=(W, H, z))
    tile_rays = W * 8
    monkeypatch.setenv("RT_WF_FINISH_THRESHOLD", "0")
    pieces = []
    for rank in range(2):
        with hip(objs, lights, None, 3, camera=(W, H, z), path="wavefront") as rt:
            rt.set_shard(tile_rays, rank, 2)
            pieces.append(rt.Render().copy())
            info = rt.rays_info()
            assert info["grid_in_use"] == 1 and info["literal"] == 0, info
    monkeypatch.delenv("RT_WF_FINISH_THRESHOLD")
    frame = sharding.assemble_frame([torch.from_numpy(p) for p in pieces], tile_rays, W * H).numpy()
    assert np.array_equal(bits(frame).reshape(-1), want["frame"].reshape(-1))


def test_a_supersampled_frame(monkeypatch):
    objs, lights = cloud()
    z = float(camera.camera_z(32))
    out = {}
    for walk in ("blocks", "brute"):   # (no aux records with a supersampling factor: frame and ray counts)
        if walk == "blocks":
            monkeypatch.setenv("RT_WF_FINISH_THRESHOLD", "0")
        with hip(objs, lights, None, 3, camera=(32, 32, z), supersample=2, path="wavefront", grid=walk != "brute") as rt:
            frame = bits(rt.Render().copy())
            st = rt.count_rays()
            if walk == "blocks":
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, info
        monkeypatch.delenv("RT_WF_FINISH_THRESHOLD", raising=False)
        out[walk] = (frame, int(st.rays_traced), int(st.rays_reference), int(st.hit_pixels))
    assert out["blocks"][0].size == 32 * 32 * 4 and out["blocks"][3] > 400
    assert np.array_equal(out["blocks"][0], out["brute"][0]) and out["blocks"][1:] == out["brute"][1:]


def test_eight_bit_output(monkeypatch):
    objs, lights = cloud()
    z = float(camera.camera_z(H))
    out = {}
    for walk in ("blocks", "brute"):
        if walk == "blocks":
            monkeypatch.setenv("RT_WF_FINISH_THRESHOLD", "0")
        with hip(objs, lights, None, 3, camera=(W, H, z), path="wavefront", grid=walk != "brute") as rt:
            out[walk] = rt.render_packed("rgba8").copy()
            if walk == "blocks":
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, info
        monkeypatch.delenv("RT_WF_FINISH_THRESHOLD", raising=False)
    assert out["blocks"].dtype == np.uint8 and np.array_equal(out["blocks"], out["brute"]) and out["blocks"].any()
