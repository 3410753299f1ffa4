"""GPU: the frame a context renders depends on its current state only, never on how it got there.

rt_set_camera, rt_set_camera_multi and rt_set_shard on contexts that have already rendered, and the render entry points in
any order. The reference in every test is a FRESH context created directly in the final state (itself held to the oracle by
tests/test_frame_shapes_gpu.py; the cameras that file does not use are held to the oracle here); every comparison is bit for
bit on the frame, primary t, hit index and rays_reference. rt_set_camera demands width * height == n_rays, so a live context
moves between the factorizations of one ray count: 9 216 for the large scenes, 1 800 for the 40-object scene. Seeds are fixed;
a failure names the step and the calls up to it."""
import numpy as np
import pytest
import torch

from helpers import R
from opencl_raytracer_amd import sharding
from test_frame_shapes_cpu import DEPTH, FACTORS_1800, FACTORS_9216, camera_z_for, launch_form, pinhole_rays, scene
from test_frame_shapes_gpu import FORMATS, assert_same_snapshot, check_against_oracle, hip, same_bits, snapshot

pytestmark = pytest.mark.gpu
FACTORS = {"s40": FACTORS_1800, "s80": FACTORS_1800, "s300": FACTORS_9216, "tri": FACTORS_9216}
EVEN = {"s40": (36, 50), "s80": (36, 50), "s300": (96, 96), "tri": (128, 72)}               # out of the domain at z = 0 needs even sides
ODD = {"s40": (200, 9), "s80": (8, 225), "s300": (9, 1024), "tri": (1024, 9)}              # an odd side: z = 0 stays inside
INVALID_ARGUMENT = -1


def clean_env(monkeypatch):
    for k in ("RT_RENDER_PASSES", "RT_RENDER_SPLIT"):
        monkeypatch.delenv(k, raising=False)


class Fresh:
    """Snapshots of fresh contexts created directly in a state, remembered per state."""

    def __init__(self, name, kernel):
        self.name, self.kernel, self.seen = name, kernel, {}

    def make(self, cam, shard=None):
        objs, lights = scene(self.name)
        rt = hip(objs, lights, None, DEPTH, camera=cam, kernel=self.kernel)
        if shard:
            rt.set_shard(*shard)
        return rt

    def __call__(self, cam, shard=None):
        key = (cam, shard)
        if key not in self.seen:
            with self.make(cam, shard) as rt:
                snap = snapshot(rt)
                if self.kernel != "hittest":
                    snap["packed"] = {fmt: rt.render_packed(fmt) for fmt, _ in FORMATS}
            self.seen[key] = snap
        return self.seen[key]


def z_kinds(name, W, H):
    rule = camera_z_for(name, W, H)
    return {"rule": rule, "third": camera_z_for(name, W, H, 1.0 / 3.0), "triple": camera_z_for(name, W, H, 3.0), "away": -rule}


def camera_walk(name, seed, steps=44):
    """[(W, H, z, what)]: a fixed prefix with the cameras on both sides of camera_in_domain (every out-of-domain camera followed
    directly by an in-domain one), then seeded draws over the factorizations and distances."""
    rng = np.random.default_rng(seed)
    ew, eh = EVEN[name]
    ow, oh = ODD[name]
    walk = []
    for z in (0.0, 1e-16, 1e16):
        walk.append((ew, eh, float(np.float32(z)), "out of the domain"))
        W, H = FACTORS[name][int(rng.integers(0, len(FACTORS[name])))]
        walk.append((W, H, camera_z_for(name, W, H), "rule"))
    walk.append((ow, oh, 0.0, "z = 0 inside the domain"))
    walk.append((ew, eh, camera_z_for(name, ew, eh), "rule"))
    walk.append((ow, oh, float(np.float32(1e-16)), "z = 1e-16 inside the domain"))
    while len(walk) < steps:
        W, H = FACTORS[name][int(rng.integers(0, len(FACTORS[name])))]
        kind = ["rule", "rule", "third", "triple", "away"][int(rng.integers(0, 5))]
        walk.append((W, H, z_kinds(name, W, H)[kind], kind))
    return walk


@pytest.mark.parametrize("name,kernel", [("s40", "shade_and_reflect"), ("s80", "shade"), ("s300", "shade_and_reflect"), ("s300", "hittest"),
                                         ("tri", "shade_and_reflect")])
def test_camera_walk(monkeypatch, restatement, name, kernel):
    from opencl_raytracer_amd.hip_raytracer import RTError
    clean_env(monkeypatch)
    objs, lights = scene(name)
    fresh = Fresh(name, kernel)
    walk = camera_walk(name, seed=20 + len(name))
    assert len(walk) >= 40
    W0, H0 = FACTORS[name][0]
    history = [f"create {W0}x{H0}"]
    cam = (W0, H0, camera_z_for(name, W0, H0))
    was_out = False
    seen_wavefront = set()
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        rt.Render()
        for step, (W, H, z, what) in enumerate(walk):
            history.append(f"set_camera({W}, {H}, {z!r})")
            where = f"step {step} ({what}) after {history}"
            out = what == "out of the domain"
            if out and name == "tri":
                with pytest.raises(RTError) as refused:
                    rt.set_camera(W, H, z)
                assert refused.value.code == INVALID_ARGUMENT, where
                history[-1] += " refused"
            else:
                rt.set_camera(W, H, z)
                cam = (W, H, z)
            got = snapshot(rt)
            st = rt.stats()
            assert (st.pinhole, st.width, st.height, st.local_rays) == (1, cam[0], cam[1], cam[0] * cam[1]), where
            want = fresh(cam)
            assert_same_snapshot(got, want, where)
            assert got["wavefront"] == want["wavefront"], where
            seen_wavefront.add(got["wavefront"])
            if out and name == "s300":
                assert got["wavefront"] == 0, f"{where}: an out-of-domain camera renders with the literal loops"
            if was_out and name in ("s300", "tri"):
                assert got["wavefront"] == 1, f"{where}: not back on the large-scene path"
                if kernel == "shade_and_reflect" and name == "s300":
                    assert got["traced"] < got["rays_ref"], f"{where}: the literal flag did not come off"
            if out and name != "tri":
                assert got["traced"] == got["rays_ref"], f"{where}: the literal loops trace every reference ray"
            if what != "rule":   # the cameras test_frame_shapes_gpu.py does not hold to the oracle
                check_against_oracle(name, kernel, got, restatement[True].render(kernel, objs, lights, pinhole_rays(*cam), DEPTH), where)
            was_out = out and name != "tri"
    if name == "s300":
        assert seen_wavefront == {0, 1}


CLOUD = {"s40": (3.0, (-16.0, -6.0)), "s300": (8.0, (-40.0, -8.0))}   # where test_frame_shapes_cpu.scene puts the objects


def far_rays(name, n, seed):
    """Jittered, non-pinhole rays whose origins lie far from the origin, aimed into the cloud."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    spread, (z0, z1) = CLOUD[name]
    origin = np.array([60.0, -45.0, 35.0]) + rng.uniform(-4, 4, size=(n, 3))
    target = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(z0, z1, n)], axis=1)
    rays["start"][:, :3] = origin
    rays["start"][:, 3] = 1.0
    rays["direction"][:, :3] = (target - origin) * rng.uniform(0.5, 2.0, size=(n, 1))
    return rays


@pytest.mark.parametrize("name", ("s40", "s300"))
@pytest.mark.parametrize("kind", ("far origins", "direction.w = 0.5", "one ray of direction 0"))
def test_uploaded_rays_then_a_camera(monkeypatch, restatement, name, kind):
    """A camera replaces uploaded rays for good - also under a grid that was built for other origins, without a
    grid (direction.w != 0 builds none), and after a frame that rays_out_of_domain forced literal."""
    clean_env(monkeypatch)
    objs, lights = scene(name)
    shapes = FACTORS[name]
    n = shapes[0][0] * shapes[0][1]
    if kind == "far origins":
        rays = far_rays(name, n, 3)
    else:
        rays = pinhole_rays(*shapes[0], camera_z_for(name, *shapes[0]))
        if kind == "direction.w = 0.5":
            rays["direction"][:, 3] = 0.5
        else:
            rays["direction"][n // 3] = 0.0
    for kernel in ("shade_and_reflect", "hittest"):
        fresh = Fresh(name, kernel)
        with hip(objs, lights, rays, DEPTH, kernel=kernel, raygen=False) as rt:
            first = snapshot(rt)
            assert rt.stats().pinhole == 0
            check_against_oracle(name, kernel, first, restatement[True].render(kernel, objs, lights, rays, DEPTH), f"{name} {kind} {kernel} uploaded")
            if kind == "far origins":
                assert (first["idx"] >= 0).mean() > 0.25
            if kind == "one ray of direction 0" and kernel == "shade_and_reflect":
                assert first["traced"] == first["rays_ref"]
            history = [f"create with {kind}"]
            for W, H in (shapes[1], shapes[4], shapes[0], shapes[-1]):
                cam = (W, H, camera_z_for(name, W, H))
                rt.set_camera(*cam)
                history.append(f"set_camera{cam}")
                got = snapshot(rt)
                assert rt.stats().pinhole == 1, history
                assert_same_snapshot(got, fresh(cam), f"{kernel} after {history}")
                assert got["wavefront"] == fresh(cam)["wavefront"] or kind == "direction.w = 0.5", history
                if kind == "direction.w = 0.5" and name == "s300":
                    assert got["wavefront"] == 0   # no grid was built for those rays, and none is built later
                if kind == "one ray of direction 0" and name == "s300" and kernel == "shade_and_reflect":
                    assert got["wavefront"] == 1 and got["traced"] < got["rays_ref"], f"the literal flag did not come off: {history}"


def shard_walk(name, seed):
    """[("shard", tile, rank, world) | ("camera", W, H)]; tile is ("rows", r) of the CURRENT width or ("rays", k)."""
    shapes = FACTORS[name]
    rng = np.random.default_rng(seed)
    walk = [("shard", ("rows", 16), 1, 3), ("camera", *shapes[2]), ("shard", ("rows", 16), 1, 3), ("shard", ("rows", 16), 0, 1), ("camera", *shapes[1]),
            ("shard", ("rows", 4), 1, 2), ("camera", *shapes[3]), ("shard", ("rays", 50), 0, 2), ("shard", ("rays", 50), 4, 5), ("camera", *shapes[8]),
            ("shard", ("rows", 8), 4, 5), ("shard", ("rows", 8), 0, 5), ("shard", ("rows", 16), 2, 3), ("camera", *shapes[0]), ("shard", ("rows", 16), 0, 1),
            ("shard", ("rows", 16), 1, 3)]
    for _ in range(16):
        if rng.integers(0, 3) == 0:
            walk.append(("camera", *shapes[int(rng.integers(0, len(shapes)))]))
        else:
            tile = [("rows", 16), ("rows", 4), ("rays", 50), ("rows", 8)][int(rng.integers(0, 4))]
            world = int(rng.choice([1, 2, 3, 5]))
            walk.append(("shard", tile, int(rng.integers(0, world)), world))
    return walk


@pytest.mark.parametrize("name", ("s40", "s300"))
def test_shard_walk(monkeypatch, name):
    """rt_set_shard on a context that has rendered with another shard, interleaved with cameras: the shard is expressed in rays
    and survives a camera change; n_local grows and shrinks; buffers that only grow keep serving."""
    clean_env(monkeypatch)
    kernel = "shade_and_reflect"
    objs, lights = scene(name)
    fresh = Fresh(name, kernel)
    W, H = FACTORS[name][0]
    n = W * H
    cam, shard = (W, H, camera_z_for(name, W, H)), None
    history, locals_seen, forms = [f"create {W}x{H}"], [], set()
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        rt.Render()
        for step, call in enumerate(shard_walk(name, seed=77)):
            if call[0] == "camera":
                cam = (call[1], call[2], camera_z_for(name, call[1], call[2]))
                rt.set_camera(*cam)
                history.append(f"set_camera{cam}")
            else:
                _, (unit, k), rank, world = call
                shard = (k * cam[0] if unit == "rows" else k, rank, world)
                rt.set_shard(*shard)
                history.append(f"set_shard{shard}")
            where = f"step {step} after {history}"
            expect_local = sharding.local_rays(n, shard[0], shard[1], shard[2]) if shard else n
            assert rt.local_rays == expect_local, where
            locals_seen.append(expect_local)
            form = launch_form(cam[0], cam[1], cam[2], len(objs), *(shard or (0, 0, 1)))
            forms.add((form["empty"], form["tile2d"], form["tile_order"], form["padded"]))
            want = fresh(cam, shard)
            frame = rt.Render()
            assert same_bits(frame, want["frame"]), f"Render, {where}"
            for fmt, _ in FORMATS:
                assert np.array_equal(rt.render_packed(fmt), want["packed"][fmt]), f"render_packed({fmt}), {where}"
            t, idx = rt.render_aux()
            assert same_bits(t, want["t"]) and np.array_equal(idx, want["idx"]), f"render_aux, {where}"
            st = rt.count_rays()
            assert (int(st.rays_reference), int(st.hit_pixels), int(st.local_rays)) == (want["rays_ref"], want["hits"], expect_local), where
    steps = np.diff(locals_seen)
    assert (steps > 0).any() and (steps < 0).any() and 0 in locals_seen and n in locals_seen
    assert {f[0] for f in forms} == {False, True} and {f[1] for f in forms} == {False, True} and {f[3] for f in forms} == {False, True}


ENTRY_POINTS = ("Render", "render_device", "render_aux", "count_rays", "render_packed rgba8", "render_packed rgb8", "render_device_packed rgba8",
                "render_device_packed rgb8")


@pytest.mark.parametrize("name", ("s40", "s300", "tri"))
def test_entry_points_in_any_order(monkeypatch, name):
    """A seeded sequence of 64 calls over every render entry point, with and without forced passes: every result is what a fresh
    context returns for that entry point, and count_rays' figures never change."""
    clean_env(monkeypatch)
    kernel = "shade_and_reflect"
    objs, lights = scene(name)
    W, H = FACTORS[name][1]
    n = W * H
    cam = (W, H, camera_z_for(name, W, H))
    want = Fresh(name, kernel)(cam)
    counts = (want["rays_ref"], want["traced"], want["hits"])
    rng = np.random.default_rng(31)
    side = torch.cuda.Stream()
    history = []
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel) as rt:
        calls = list(ENTRY_POINTS) * 2 + [ENTRY_POINTS[int(rng.integers(0, len(ENTRY_POINTS)))] for _ in range(48)]
        order = rng.permutation(len(calls))
        for step, k in enumerate(order):
            call, passes = calls[int(k)], bool(rng.integers(0, 2))
            if passes: monkeypatch.setenv("RT_RENDER_PASSES", "2")
            else: monkeypatch.delenv("RT_RENDER_PASSES", raising=False)
            history.append(call + (" [passes]" if passes else ""))
            where = f"step {step} after {history}"
            if call == "Render":
                assert same_bits(rt.Render(), want["frame"]), where
            elif call == "render_device":
                out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
                with torch.cuda.stream(side):
                    rt.render_device(out.data_ptr(), side.cuda_stream)
                    copy = out.clone()
                side.synchronize()
                assert same_bits(copy.cpu().numpy(), want["frame"]), where
            elif call == "render_aux":
                t, idx = rt.render_aux()
                assert same_bits(t, want["t"]) and np.array_equal(idx, want["idx"]), where
            elif call == "count_rays":
                st = rt.count_rays()
                assert (int(st.rays_reference), int(st.rays_traced), int(st.hit_pixels)) == counts, where
            elif call.startswith("render_packed"):
                fmt = call.split()[1]
                assert np.array_equal(rt.render_packed(fmt), want["packed"][fmt]), where
            else:
                fmt = call.split()[1]
                out = torch.zeros((n, 4 if fmt == "rgba8" else 3), dtype=torch.uint8, device="cuda")
                with torch.cuda.stream(side):
                    rt.render_device_packed(out.data_ptr(), fmt, side.cuda_stream)
                    copy = out.clone()
                side.synchronize()
                assert np.array_equal(copy.cpu().numpy(), want["packed"][fmt]), where
            st = rt.stats()
            assert (int(st.local_rays), st.pinhole, st.width, st.height) == (n, 1, W, H), where
    assert len(history) >= 60


@pytest.mark.parametrize("name,first", [("s300", (96, 96)), ("s300", (1024, 9)), ("s40", (36, 50)), ("tri", (128, 72))])
def test_several_contexts_on_one_gpu_follow_the_camera(monkeypatch, name, first):
    """MultiHIPRaytracer(devices=(0, 0, 0)): set_camera across widths. The tile size stays the one chosen at creation - 16 rows
    of the FIRST width, in rays - so later frames are cut into tiles that are no whole rows; frame_elems never changes."""
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer
    clean_env(monkeypatch)
    kernel = "shade_and_reflect"
    objs, lights = scene(name)
    fresh = Fresh(name, kernel)
    n = first[0] * first[1]
    tile = 16 * first[0]
    elems = sharding.n_tiles(n, tile) * tile
    history = [f"create {first}"]
    rng = np.random.default_rng(8)
    shapes = [first] + [FACTORS[name][int(k)] for k in rng.permutation(len(FACTORS[name]))]
    with MultiHIPRaytracer(objs, lights, None, DEPTH, devices=(0, 0, 0), camera=(*first, camera_z_for(name, *first)), kernel=kernel) as m:
        for step, (W, H) in enumerate(shapes):
            cam = (W, H, camera_z_for(name, W, H))
            if step:
                m.set_camera(*cam)
                history.append(f"set_camera{cam}")
            where = f"step {step} after {history}"
            want = fresh(cam)
            assert m.frame_elems == elems, where
            assert same_bits(m.Render(), want["frame"]), f"Render, {where}"
            for fmt, _ in FORMATS:
                assert np.array_equal(m.render_packed(fmt), want["packed"][fmt]), f"render_packed({fmt}), {where}"
            frame = torch.zeros((elems, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            m.render_device(frame.data_ptr())
            assert same_bits(frame[:n].cpu().numpy(), want["frame"]), f"render_device, {where}"
            st = m.count_rays()
            assert (int(st.rays_reference), int(st.hit_pixels)) == (want["rays_ref"], want["hits"]), where
