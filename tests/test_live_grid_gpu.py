"""GPU: a LIVE grid - built for one population of rays - under ray buffers and poses it was not built around (DESIGN.md 4.1,
"which box the radii are built for"; hip_raytracer.h, "replaceable rays" and "posed cameras").

1. the gate: the three places in csrc/rt_api.cpp that decide whether a buffer or a pose stays on the grid, on the last float32
   inside each of the box's six faces and on the first one beyond it (test_live_grid_cpu.gate_cases), through the host route, the
   device-tensor route and rt_set_pose;
2. a live grid serves buffers that FILL its box (test_live_grid_cpu.population): the frame of a fresh context created with those
   rays - whose grid is built around them - and of a fresh brute-force context, bit for bit (a mesh has no brute force: there
   the second witness is a grid built for origins 200 units out); the two aimed populations against the oracle under the bars
   of test_frame_shapes_gpu.py;
3. the large-scene kernels with the grid switched off for a frame (do_launch, `grid_in_use`): a live context walked camera ->
   inside -> one origin one float32 outside -> a far pose -> inside -> camera, every step against fresh contexts.
The boxes are the library's own (rays_info()["box_lo"/"box_hi"] of the live context), never recomputed here. Every comparison
covers every ray. What these tests cannot show: a registration radius that is a few ulp short fails only on a grazing ray that
happens to be drawn. `pytest -s` prints hit shares, the largest |dRGB| against the oracle and the wall time of each test."""
import time

import numpy as np
import pytest

from helpers import clear_lights
from opencl_raytracer_amd import rays as RY
from test_context_lifecycle_gpu import INVALID_ARGUMENT, clean_env
from test_frame_shapes_cpu import DEPTH, camera_z_for
from test_frame_shapes_gpu import assert_same_snapshot, check_against_oracle, hip, packed_of, same_bits, snapshot, stitched
from test_live_grid_cpu import (FAR, KINDS, N, ORACLE_KINDS, SCAN_TRIP, check_gate_cases, far_creation_rays, first_outside, gate_base,
                                gate_cases, gate_faces, inward, last_inside, live_scene, population)
from test_set_rays_cpu import POSES
from test_set_rays_gpu import device_tensor

pytestmark = pytest.mark.gpu
F = np.float32
W = H = 96
MIN_HIT_SHARE = 0.05
SECONDS = {}


def camera_of(name):
    return (W, H, camera_z_for("s300" if name == "s608" else name, W, H))   # s608 is s300's cloud, denser


def snap(rt):
    """snapshot() and the exact object tests of its counted render."""
    s = snapshot(rt)
    s["tests"] = int(rt.stats().object_tests)
    return s


def hit_share(s):
    return float((s["idx"] >= 0).mean())


def fresh(objs, lights, kernel, rays=None, cam=None, **kw):
    """(snapshot, rays_info) of a fresh context created in that state."""
    with (hip(objs, lights, rays, DEPTH, kernel=kernel, raygen=False, **kw) if rays is not None else
          hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel, **kw)) as rt:
        return snap(rt), rt.rays_info()


def brute(objs, lights, kernel, rays=None, cam=None, **kw):
    """The independent witness: the large-scene kernels without any grid."""
    s, info = fresh(objs, lights, kernel, rays, cam, path="wavefront", grid=False, **kw)
    assert (s["wavefront"], info["grid_built"]) == (1, 0)
    return s


def same_info(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def same_but_for(a, b, at, label):
    """Two snapshots of buffers that differ in ray `at` alone: every other ray's pixel, time and index."""
    keep = np.arange(len(a["idx"])) != at
    assert same_bits(a["frame"][keep], b["frame"][keep]), f"{label}: frames differ on another ray than {at}"
    assert same_bits(a["t"][keep], b["t"][keep]) and np.array_equal(a["idx"][keep], b["idx"][keep]), f"{label}: t / index differ on another ray than {at}"


def timed(label, started):
    SECONDS[label] = time.perf_counter() - started
    print(f"[live grid] {label}: {SECONDS[label]:.1f} s")


def numbers(info, verdict, label):
    """origin_lo / origin_hi as NUMBERS (-0.0 == 0.0; a flushed denormal or a bit-ordered extreme is not equal)."""
    assert np.array_equal(info["origin_lo"], verdict["origin_lo"]) and np.array_equal(info["origin_hi"], verdict["origin_hi"]), \
        f"{label}: origin box {info['origin_lo']} .. {info['origin_hi']}, expected {verdict['origin_lo']} .. {verdict['origin_hi']}"


# ---- 1. the gate ------------------------------------------------------------------------------------------------------------
def walk_gate_cases(rt, name, cases, base, label):
    """Every case through both routes; returns the number of refusals."""
    from opencl_raytracer_amd.hip_raytracer import RTError
    refused_count = 0
    for what, rays, inside in cases:
        want = RY.ray_verdict(rays)
        for route in ("host", "device"):
            where = f"{label}, {what}, {route} route"
            before = rt.rays_info()
            if name == "tri" and not inside:   # a mesh is traced by the grid only
                with pytest.raises(RTError) as refused:
                    rt.set_rays(rays if route == "host" else device_tensor(rays))
                assert refused.value.code == INVALID_ARGUMENT, where
                assert same_info(rt.rays_info(), before), f"{where}: a refused buffer changed the context's state"
                refused_count += 1
                continue
            rt.set_rays(rays if route == "host" else device_tensor(rays))
            info = rt.rays_info()
            assert (info["source"], info["dir_w_zero"], info["directions_in_domain"], info["starts_ok"], info["literal"]) == (2, 1, 1, 1, 0), where
            numbers(info, want, where)
            assert info["grid_in_use"] == (1 if inside else 0), f"{where}: grid_in_use {info['grid_in_use']}"
            if not inside:
                rt.set_rays(base if route == "host" else device_tensor(base))
                assert rt.rays_info()["grid_in_use"] == 1, f"{where}: an inside buffer did not bring the grid back"
    return refused_count


@pytest.mark.parametrize("name", ("s300", "tri"))
def test_the_gate_on_every_face_of_the_box(name):
    from opencl_raytracer_amd.hip_raytracer import RTError
    started = time.perf_counter()
    objs, lights = live_scene(name)
    shares = []
    with hip(objs, lights, None, DEPTH, camera=camera_of(name), kernel="hittest") as rt:
        info = rt.rays_info()
        assert (info["source"], info["grid_built"], info["grid_in_use"]) == (1, 1, 1)
        lo, hi = info["box_lo"], info["box_hi"]
        cases = gate_cases(lo, hi, N)
        by_face = check_gate_cases(lo, hi, N, cases)   # ... the two cases of a face differ in exactly one float32 of one ray
        assert len(by_face) == 6 and ((hi[2] == 0) == (name == "tri"))
        base = gate_base(lo, hi, N)
        refusals = walk_gate_cases(rt, name, cases, base, name)
        assert refusals == (14 if name == "tri" else 0)
        # one pair of frames per face: the inside variant on the grid, the outside variant off it (a mesh: refused, nothing changes)
        for face, pair in by_face.items():
            at = int(np.flatnonzero((pair["inside"].view(np.uint32) != pair["outside"].view(np.uint32)).reshape(N, 8).any(axis=1))[0])
            rt.set_rays(device_tensor(pair["inside"]))
            on = snap(rt)
            assert (rt.rays_info()["grid_in_use"], on["wavefront"]) == (1, 1), face
            shares.append(hit_share(on))
            if name == "tri":
                with pytest.raises(RTError) as refused:
                    rt.set_rays(pair["outside"])
                assert refused.value.code == INVALID_ARGUMENT, face
                assert_same_snapshot(snap(rt), on, f"{name} {face}: after the refusal")
            else:
                rt.set_rays(pair["outside"])
                off = snap(rt)
                assert (rt.rays_info()["grid_in_use"], off["wavefront"]) == (0, 0), face   # 96..511 objects: the small-scene kernel
                same_but_for(on, off, at, f"{name} {face}")
        rt.set_rays(base)
        assert rt.rays_info()["grid_in_use"] == 1
    assert min(shares) > MIN_HIT_SHARE, shares
    print(f"[live grid] gate {name}: hit shares {min(shares):.3f} .. {max(shares):.3f}")
    timed(f"gate {name}", started)


@pytest.mark.parametrize("name", ("s300", "tri"))
def test_the_gate_beyond_the_scans_first_trip(name):
    """The moved ray is one that the scan kernel reaches in the second trip of its grid-stride loop."""
    started = time.perf_counter()
    objs, lights = live_scene(name)
    n = SCAN_TRIP + 1000
    with hip(objs, lights, None, 0, camera=(n, 1, -1.0), kernel="hittest") as rt:
        info = rt.rays_info()
        assert (info["grid_built"], info["grid_in_use"]) == (1, 1)
        lo, hi = info["box_lo"], info["box_hi"]
        cases = gate_cases(lo, hi, n)
        check_gate_cases(lo, hi, n, cases)
        assert len(cases) == 2 and all(f"ray {SCAN_TRIP + 77}" in what for what, _, _ in cases)
        assert walk_gate_cases(rt, name, cases, gate_base(lo, hi, n), f"{name}, {n} rays") == (2 if name == "tri" else 0)
    timed(f"gate beyond the first trip {name}", started)


@pytest.mark.parametrize("name", ("s300", "tri"))
def test_the_pose_gate_on_every_face_of_the_box(name):
    """rt_set_pose judges its single origin on the host: the same twelve face coordinates, the other two from the box's centre."""
    from opencl_raytracer_amd.hip_raytracer import RTError
    started = time.perf_counter()
    objs, lights = live_scene(name)
    M = POSES["pan"][0]
    cam = camera_of(name)
    shares = []
    with hip(objs, lights, None, DEPTH, camera=cam, kernel="hittest") as rt:
        info = rt.rays_info()
        assert (info["grid_built"], info["grid_in_use"]) == (1, 1)
        lo, hi = info["box_lo"], info["box_hi"]
        centre = inward((lo + hi) / 2.0, lo, hi)
        for axis, side in gate_faces():
            face = float((lo if side == "lo" else hi)[axis])
            where = f"{name} pose {'xyz'[axis]}.{side}"
            origin_in, origin_out = centre.copy(), centre.copy()
            origin_in[axis], origin_out[axis] = last_inside(face, side), first_outside(face, side)
            assert int((origin_in.view(np.uint32) != origin_out.view(np.uint32)).sum()) == 1
            rt.set_pose(*cam, M, origin_in)
            info = rt.rays_info()
            assert (info["source"], info["starts_ok"], info["literal"]) == (3, 1, 0), where
            assert np.array_equal(info["origin_lo"], origin_in) and np.array_equal(info["origin_hi"], origin_in), where
            assert info["grid_in_use"] == 1, f"{where}: the last float32 inside the face left the grid"
            on = snap(rt)   # the frame of the face, against a fresh context created with the pose's rays
            want, _ = fresh(objs, lights, "hittest", RY.posed_rays(*cam, M, origin_in))
            assert_same_snapshot(on, want, where)
            assert on["wavefront"] == 1, where
            shares.append(hit_share(on))
            if name == "tri":
                before = rt.rays_info()
                with pytest.raises(RTError) as refused:
                    rt.set_pose(*cam, M, origin_out)
                assert refused.value.code == INVALID_ARGUMENT, where
                assert same_info(rt.rays_info(), before), where
                assert_same_snapshot(snap(rt), on, f"{where}: after the refusal")
                continue
            rt.set_pose(*cam, M, origin_out)
            info = rt.rays_info()
            assert np.array_equal(info["origin_lo"], origin_out) and np.array_equal(info["origin_hi"], origin_out), where
            assert (info["source"], info["grid_in_use"]) == (3, 0), f"{where}: the first float32 beyond the face stayed on the grid"
            rt.set_pose(*cam, M, centre)
            assert rt.rays_info()["grid_in_use"] == 1, f"{where}: an inside pose did not bring the grid back"
    # a pose looks one way, so a face behind the scene sees little of it: the condition is on the faces together
    assert float(np.mean(shares)) > MIN_HIT_SHARE, shares
    print(f"[live grid] pose gate {name}: hit shares {min(shares):.3f} .. {max(shares):.3f}, mean {np.mean(shares):.3f}")
    timed(f"pose gate {name}", started)


# ---- 2. a live grid serves buffers that fill its box ----------------------------------------------------------------------------
def make_live(name, which, kernel, lights=None, **kw):
    objs, scene_lights = live_scene(name)
    lights = scene_lights if lights is None else lights
    if which == "A":   # created with the scene's camera: the box is {0} united with the objects
        return hip(objs, lights, None, DEPTH, camera=camera_of(name), kernel=kernel, **kw)
    return hip(objs, lights, far_creation_rays(objs, N), DEPTH, raygen=False, kernel=kernel, **kw)   # B: radii built for a large D


def serve(rt, name, kernel, kind, lights, restatement, label, route, oracle=True, **kw):
    """One population on the live context `rt`: flags, fresh context, brute force (a mesh: a differently built grid), oracle."""
    objs, _ = live_scene(name)
    info = rt.rays_info()
    lo, hi = info["box_lo"], info["box_hi"]
    rays = population(kind, lo, hi, objs, N, seed=7)
    rt.set_rays(rays if route == "host" else device_tensor(rays))
    got = snap(rt)
    info = rt.rays_info()
    assert (info["source"], info["grid_built"], info["grid_in_use"], info["literal"]) == (2, 1, 1, 0), label
    assert got["wavefront"] == 1, label
    share = hit_share(got)
    assert share > MIN_HIT_SHARE, (label, share)
    new, new_info = fresh(objs, lights, kernel, rays, **kw)
    assert (new_info["grid_built"], new_info["grid_in_use"], new["wavefront"]) == (1, 1, 1), label
    assert_same_snapshot(got, new, f"{label}: live against a fresh context")
    witness = new
    if name != "tri":
        witness = brute(objs, lights, kernel, rays, **kw)
        assert_same_snapshot(got, witness, f"{label}: live against brute force")
        if kernel != "hittest":
            assert got["tests"] < witness["tests"] // 2, f"{label}: {got['tests']} object tests - did the live frame go through the grid?"
    else:
        # No brute force for a mesh: the witness is a differently built grid. The fresh context's is not one: rt_create unites
        # the origin (0, 0, 0) with the rays' box, so for rays inside the live box the fresh box IS the live box (asserted, so
        # that a change of that rule shows here). The other grid is that of a context created with rays that start up to FAR
        # units out - a cube of 400 units about a mesh of 10, other cells, every radius built for a larger D and S_max.
        assert np.array_equal(new_info["box_lo"], lo) and np.array_equal(new_info["box_hi"], hi), f"{label}: the fresh grid's box"
        with hip(objs, lights, far_creation_rays(objs, N), DEPTH, raygen=False, kernel=kernel, **kw) as other:
            other.set_rays(rays)
            other_info = other.rays_info()
            assert (other_info["grid_built"], other_info["grid_in_use"]) == (1, 1), label
            assert (other_info["box_lo"] == -FAR).all() and (other_info["box_hi"] == FAR).all(), f"{label}: the two grids have one box"
            assert_same_snapshot(got, snap(other), f"{label}: live against a grid built for origins {FAR:g} units out")
    err = None
    if oracle and kind in ORACLE_KINDS:
        want = restatement[kw.get("fused", True)].render(kernel, objs, lights, rays, DEPTH)
        err = check_against_oracle(name, kernel, witness, want, f"{label}: {'fresh' if name == 'tri' else 'brute-force'} context against the oracle")
    print(f"[live grid] {label}: hit share {share:.3f}" + (f", largest |dRGB| against the oracle {err:.3e}" if err is not None else ""))
    return got


@pytest.mark.parametrize("name,which", (("s300", "A"), ("s300", "B"), ("s608", "A"), ("tri", "A")))
def test_a_live_grid_serves_buffers_that_fill_its_box(monkeypatch, restatement, name, which):
    clean_env(monkeypatch)
    started = time.perf_counter()
    objs, lights = live_scene(name)
    kernel = "shade_and_reflect"
    # B's box is a cube of 400 units about a scene of 50: uniform starts see nothing of it, so B takes the aimed populations -
    # the corners are where D and S_max are attained
    todo = KINDS if which == "A" else ORACLE_KINDS
    with make_live(name, which, kernel) as rt:
        info = rt.rays_info()
        assert (info["grid_built"], info["grid_in_use"]) == (1, 1)
        if which == "B":
            assert (info["box_lo"] == -FAR).all() and (info["box_hi"] == FAR).all()
        before = dict(info)
        for k, kind in enumerate(todo):
            serve(rt, name, kernel, kind, lights, restatement, f"{name} {which} {kernel} {kind}", ("host", "device")[k % 2])
        after = rt.rays_info()
        assert np.array_equal(after["box_lo"], before["box_lo"]) and np.array_equal(after["box_hi"], before["box_hi"]), "nothing is rebuilt"
    with make_live(name, which, "hittest") as rt:   # hittest on one population
        serve(rt, name, "hittest", "fill_random" if which == "A" else "fill_aimed", lights, restatement, f"{name} {which} hittest", "device")
    timed(f"serve {name} {which}", started)


@pytest.mark.parametrize("name", ("s300", "s608", "tri"))
def test_a_live_grid_under_the_other_arithmetics(monkeypatch, restatement, name):
    """The bitwise comparisons alone: unfused on every scene, the device arithmetic where it exists (no triangles)."""
    clean_env(monkeypatch)
    started = time.perf_counter()
    objs, lights = live_scene(name)
    kernel = "shade_and_reflect"
    with make_live(name, "A", kernel, fused=False) as rt:
        serve(rt, name, kernel, "on_surfaces", lights, restatement, f"{name} unfused on_surfaces", "device", oracle=False, fused=False)
    if name != "tri":
        cl_lights, _ = clear_lights(objs, lights, np.random.default_rng(5))   # no light in reach of an object: the default path
        with make_live(name, "A", kernel, lights=cl_lights, device_opencl=True) as rt:
            assert rt.rays_info()["literal"] == 0
            serve(rt, name, kernel, "axis_parallel", cl_lights, restatement, f"{name} device_opencl axis_parallel", "host", oracle=False, device_opencl=True)
    timed(f"other arithmetics {name}", started)


# ---- 3. the large-scene path with its grid switched off for a frame -----------------------------------------------------------
@pytest.mark.parametrize("name,path,kernel", (("s608", "auto", "shade_and_reflect"), ("s608", "auto", "hittest"), ("s300", "wavefront", "shade_and_reflect")))
def test_the_grid_switched_off_for_a_frame(monkeypatch, restatement, name, path, kernel):
    """s608 stays on the large-scene kernels by its size, s300 by the path flag: off the box, do_launch hands them empty grid,
    block-grid and light-tile descriptors. Every step is the frame of a fresh context in that state and of brute force; off the
    grid the counted render traces the rays and runs the object tests that brute force does (a table that stayed switched on - which
    need not change a pixel - shows there)."""
    clean_env(monkeypatch)
    started = time.perf_counter()
    objs, lights = live_scene(name)
    cam = camera_of(name)
    colour = kernel != "hittest"
    oracle = lambda rays: restatement[True].render(kernel, objs, lights, rays, DEPTH)   # noqa: E731
    M_far, o_far, zs = POSES["far"]
    far = (W, H, camera_z_for("s300", W, H, zs))
    with hip(objs, lights, None, DEPTH, camera=cam, kernel=kernel, path=path) as rt:
        info = rt.rays_info()
        assert (info["grid_built"], info["grid_in_use"]) == (1, 1)
        lo, hi = info["box_lo"], info["box_hi"]
        inside = population("fill_aimed", lo, hi, objs, N, seed=7)
        at, axis = N // 3, 0
        moved = inside.copy()
        moved["start"][at, axis] = first_outside(float(hi[axis]), "hi")
        assert int((moved.view(np.uint32) != inside.view(np.uint32)).sum()) == 1
        far_rays = RY.posed_rays(*far, M_far, o_far)
        assert not ((np.asarray(o_far) >= lo) & (np.asarray(o_far) <= hi)).all()
        reference = {}

        def check(step, got, on_grid, rays=None):
            where = f"{name} {path} {kernel} step {step}"
            info = rt.rays_info()
            assert info["grid_built"] == 1 and info["grid_in_use"] == (1 if on_grid else 0), f"{where}: grid_in_use {info['grid_in_use']}"
            assert got["wavefront"] == 1, f"{where}: left the large-scene kernels"
            assert hit_share(got) > MIN_HIT_SHARE, (where, hit_share(got))
            key = "camera" if rays is None else step
            if key not in reference:
                kw = dict(rays=rays) if rays is not None else dict(cam=cam)
                reference[key] = (fresh(objs, lights, kernel, path=path, **kw)[0], brute(objs, lights, kernel, **kw))
            new, witness = reference[key]
            assert_same_snapshot(got, new, f"{where}: live against a fresh context")
            assert_same_snapshot(got, witness, f"{where}: live against brute force")
            if on_grid and colour:
                assert got["tests"] < witness["tests"] // 2, f"{where}: {got['tests']} object tests - did the frame go through the grid?"
            if not on_grid:
                # Without any table every traced ray is tested against every object; a table that stayed switched on (the light
                # tiles, say) takes a class of rays off that loop - the last light's shadow rays alone are one per hit, a tenth
                # of the object tests at least (asserted below). The counter itself does not repeat (measured: 20 461 940 .. 20 466 164 over seven
                # counted renders of one frame, live and brute force alike; 0.16 % between a live and a fresh render of the far pose),
                # hence 1 % and not equality.
                print(f"[live grid] {where}: traced / object tests {got['traced']} / {got['tests']}, brute force {witness['traced']} / {witness['tests']}")
                assert got["traced"] == witness["traced"], f"{where}: traced {got['traced']} rays, brute force {witness['traced']}"
                assert witness["tests"] >= 0.99 * witness["traced"] * len(objs), f"{where}: brute force skipped objects"
                assert abs(got["tests"] - witness["tests"]) <= witness["tests"] // 100, \
                    f"{where}: off the grid the frame ran {got['tests']} object tests, brute force {witness['tests']} - is a table still switched on?"
                if colour:
                    assert got["hits"] * len(objs) >= witness["tests"] // 10, f"{where}: too few hits for the light tiles to show in the tests"   # ten times the bound
            return witness

        one = snap(rt)                                   # 1. the camera
        check(1, one, True)
        rt.set_rays(device_tensor(inside))               # 2. inside
        two = snap(rt)
        witness = check(2, two, True, inside)
        reference[5] = reference[2]
        err2 = check_against_oracle(name, kernel, witness, oracle(inside), f"{name} {path} {kernel} step 2 against the oracle")
        rt.set_rays(moved)                               # 3. one origin one float32 beyond x.hi
        three = snap(rt)
        witness = check(3, three, False, moved)
        err3 = check_against_oracle(name, kernel, witness, oracle(moved), f"{name} {path} {kernel} step 3 against the oracle")
        same_but_for(two, three, at, f"{name} {path} {kernel} steps 2 and 3")
        if name == "s608":   # the partitions of the off-grid frame: the same bits
            tr = 16 * W
            pieces, ts, idxs = [], [], []
            for rank in range(3):
                rt.set_shard(tr, rank, 3)
                pieces.append(rt.Render())
                t, idx = rt.render_aux()
                ts.append(t)
                idxs.append(idx)
            rt.set_shard(0, 0, 1)
            assert same_bits(stitched(pieces, tr, N), three["frame"]), "step 3: stitched shards differ from the unsharded frame"
            assert same_bits(stitched(ts, tr, N), three["t"]) and np.array_equal(stitched(idxs, tr, N), three["idx"]), "step 3: render_aux of the shards"
            monkeypatch.setenv("RT_RENDER_PASSES", "2")
            assert same_bits(rt.Render(), three["frame"]), "step 3: two passes differ from one"
            if colour:
                assert np.array_equal(rt.render_packed("rgba8"), packed_of(three["frame"], "rgba8")), "step 3: rgba8 in two passes"
            monkeypatch.delenv("RT_RENDER_PASSES")
            if colour:
                assert np.array_equal(rt.render_packed("rgba8"), packed_of(three["frame"], "rgba8")), "step 3: rgba8"
            assert rt.rays_info()["grid_in_use"] == 0 and rt.stats().wavefront == 1
        rt.set_pose(*far, M_far, o_far)                  # 4. the far pose
        four = snap(rt)
        assert rt.rays_info()["source"] == 3
        check(4, four, False, far_rays)
        rt.set_rays(inside)                              # 5. inside again
        five = snap(rt)
        check(5, five, True, inside)
        assert_same_snapshot(five, two, "steps 2 and 5")
        rt.set_camera(*cam)                              # 6. the camera again
        six = snap(rt)
        check(6, six, True)
        assert_same_snapshot(six, one, "steps 1 and 6")
        assert rt.rays_info()["source"] == 1
    print(f"[live grid] switch {name} {path} {kernel}: hit shares {[round(hit_share(s), 3) for s in (one, two, three, four)]}, "
          f"largest |dRGB| against the oracle {max(err2, err3):.3e}")
    timed(f"switch {name} {path} {kernel}", started)


def test_summary():
    """Not a check: the wall time of each test of this file (`-s`)."""
    for label, seconds in SECONDS.items():
        print(f"\n[live grid] {label}: {seconds:.1f} s")
    print(f"[live grid] wall time of this file's tests: {sum(SECONDS.values()):.1f} s")
