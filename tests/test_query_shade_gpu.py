"""GPU: shaded queries (hip_raytracer.h, "shaded queries") - rt_query_shade_device, rt_query_shade, rt_query_primary_shade,
rt_get_query_shade_info - against ONE fresh context per batch: rgba is its Render(), (t, index) its render_aux(), rays_reference and
hit_rays its count_rays(), bit for bit; and, in the default arithmetic, against the CPU backend's frame (t, index exactly,
|dRGB| <= 1e-5 on every ray).

Scene A: 3 objects (sphere, box, sphere), 2 lights - no grid, every ray takes the ordered loop.
Scene B: helpers.random_scene with 96 objects, the smallest count that builds a grid, and 3 lights, the last far outside the cloud.
The batch: a 32 x 32 camera grid and rays from inside the cloud, interleaved, with one ray of each class the grid does not serve in
every 16 - so every wave holds both routes and both kinds of path."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import R, compare_frames, instance, random_scene, rotation
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from opencl_raytracer_amd.hip_raytracer import RTError, RTQueryShadeInfo, RTShade

pytestmark = pytest.mark.gpu
F = np.float32
MAX_FLOAT = F(3.402823466e+38)
VP = ctypes.c_void_p
W, H, Z = 32, 32, -40.0
N_B = 96
MODES = {"default": {}, "unfused": dict(fused=False), "fast_phong": dict(fast_phong=True), "device_opencl": dict(device_opencl=True)}
KERNELS = ("shade_and_reflect", "shade")
CLASSES = ("outside the box", "zero direction", "a NaN component", "an inf component", "start.w = 0", "direction.w = 1", "dd < 1e-30")


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def material(k, absorption):
    rng = np.random.default_rng(500 + k)
    return R.Material(ambient=rng.uniform(0.1, 1, 3), diffuse=rng.uniform(0.1, 1, 3), specular=rng.uniform(0.1, 1, 3), absorption=absorption,
                      reflection=1 - absorption, shininess=[1.0, 5.0, 30.0][k % 3])


@functools.lru_cache(maxsize=None)
def scene_a():
    objs = [R.make_object(R.SPHERE, material(0, 0.5), *instance((-1.5, 0.3, -14.0), None, (1.4, 1.4, 1.4))),
            R.make_object(R.BOX, material(1, 0.7), *instance((1.2, -0.2, -12.0), rotation((0.3, 1.0, 0.2), 0.6), (1.8, 1.2, 1.5))),
            R.make_object(R.SPHERE, material(2, 0.2), *instance((0.2, 1.6, -18.0), None, (2.0, 1.5, 2.0)))]
    props = [R.LightProperties(ambient=(0.1, 0.1, 0.1), diffuse=(0.5, 0.4, 0.3), specular=(0.3, 0.3, 0.3)),
             R.LightProperties(ambient=(0.05, 0.1, 0.15), diffuse=(0.2, 0.4, 0.5), specular=(0.4, 0.3, 0.2))]
    lts = [R.make_light(props[0], position=(6.0, 8.0, -4.0, 1.0)), R.make_light(props[1], position=(0.3, -1.0, -0.5, 0.0))]
    return R.objects_array(objs), R.lights_array(lts)


@functools.lru_cache(maxsize=None)
def scene_b():
    objs, lts = random_scene(60, N_B - 60, 3, seed=77, directional_lights=1)
    lts["position"][2] = (300.0, 200.0, 150.0, 1.0)   # far outside the cloud
    return objs, lts


SCENES = {"A": scene_a, "B": scene_b}


def query_context(name, depth=2, kernel="shade_and_reflect", lts=None, **kw):
    objs, own = SCENES[name]()
    return hip(objs, own if lts is None else lts, None, depth, camera=(W, H, Z), kernel=kernel, **kw)


@functools.lru_cache(maxsize=None)
def box_of(name):
    """box_lo, box_hi of the scene's context (None, None: no grid)."""
    with query_context(name) as rt:
        info = rt.rays_info()
    assert info["grid_built"] == (1 if name == "B" else 0), name
    return (info["box_lo"].copy(), info["box_hi"].copy()) if info["grid_built"] else (None, None)


def camera_rays():
    """The pinhole grid of rt_set_camera(W, H, Z), ray by ray."""
    rays = np.zeros(W * H, dtype=R.RAY_DTYPE)
    col, row = np.tile(np.arange(W), H).astype(F), np.repeat(np.arange(H), W).astype(F)
    rays["start"][:, 3] = 1.0
    rays["direction"][:, 0] = col - F(W) / F(2.0)
    rays["direction"][:, 1] = (F(H) - row) - F(H) / F(2.0)
    rays["direction"][:, 2] = F(Z)
    return rays


@functools.lru_cache(maxsize=None)
def batch(name="B"):
    """2048 rays: camera ray, inside ray, camera ray, ... with ray 16 k + 5 replaced by class k % 7 (CLASSES)."""
    objs, _ = SCENES[name]()
    centres = objs["mv"].reshape(len(objs), 16)[:, 12:15].astype(np.float64)
    lo, hi = centres.min(axis=0) - 1.0, centres.max(axis=0) + 1.0
    rng = np.random.default_rng(7)
    n = 2 * W * H
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays[0::2] = camera_rays()
    inside = np.zeros(W * H, dtype=R.RAY_DTYPE)
    inside["start"][:, :3] = (lo + rng.uniform(0.0, 1.0, size=(W * H, 3)) * (hi - lo)).astype(F)
    inside["start"][:, 3] = 1.0
    aim = centres[rng.integers(0, len(objs), size=W * H)] - inside["start"][:, :3]
    inside["direction"][:, :3] = (aim * rng.uniform(0.5, 2.0, size=(W * H, 1))).astype(F)
    rays[1::2] = inside
    for k in range(n // 16):
        i, kind = 16 * k + 5, CLASSES[k % 7]
        target = centres[k % len(objs)]
        if kind == "outside the box":
            start = np.array([hi[0] + 40.0 + k % 5, lo[1] - 30.0, hi[2] + 50.0])
            rays["start"][i, :3] = start.astype(F)
            rays["direction"][i, :3] = (target - start).astype(F)
        elif kind == "zero direction":
            rays["direction"][i, :3] = 0.0
        elif kind == "a NaN component":
            rays["start"][i, k % 3] = np.nan
        elif kind == "an inf component":
            rays["direction"][i, k % 3] = np.inf
        elif kind == "start.w = 0":
            rays["start"][i, 3] = 0.0
        elif kind == "direction.w = 1":
            rays["direction"][i, 3] = 1.0
        else:
            d = rays["direction"][i, :3].astype(np.float64)
            rays["direction"][i, :3] = (d / np.linalg.norm(d) * 1.0e-16).astype(F)
    return rays


def fresh(objs, lts, rays, depth, kernel, **mode):
    """What a fresh context created with these rays delivers: the definition of a shaded query."""
    with hip(objs, lts, rays, depth, kernel=kernel, raygen=False, **mode) as rt:
        frame = rt.Render()
        t, index = rt.render_aux()
        st = rt.count_rays()
        return dict(rgba=frame, t=t, index=index, rays_reference=int(st.rays_reference), hit_rays=int(st.hit_pixels))


def assert_shade(got, want, label, info=None):
    for k in ("rgba", "t", "index"):
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape, (label, k)
        bad = (a != b).reshape(len(a), -1).any(axis=1)
        assert not bad.any(), f"{label}: {k} differs on {int(bad.sum())} rays, first at {int(np.nonzero(bad)[0][0])}"
    if info is not None:
        assert (info["rays_reference"], info["hit_rays"]) == (want["rays_reference"], want["hit_rays"]), (label, info, want["rays_reference"], want["hit_rays"])


def assert_route(info, rays, name, literal=False, mask=None):
    route = RY.query_shade_route(rays, *box_of(name), literal=literal, mask=mask)
    want = tuple(int(route[k].sum()) for k in ("traced", "grid", "brute", "literal"))
    assert (info["n_rays"], info["n_grid"], info["n_brute"], info["n_literal"]) == want, (info, want)


ALL = ("rgba", "t", "index")
GUARD = {"rgba": -3.5, "t": -7.25, "index": -77}


def guarded(n):
    import torch
    shapes = {"rgba": ((n + 1, 4), torch.float32), "t": ((n + 1,), torch.float32), "index": ((n + 1,), torch.int32)}
    return {k: torch.full(s, GUARD[k], dtype=d, device="cuda") for k, (s, d) in shapes.items()}


def snapshot(rt):
    frame = rt.Render()
    t, index = rt.render_aux()
    return dict(frame=bits(frame).copy(), t=bits(t).copy(), index=index.copy())


def same_snapshot(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---- counts and the guard element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_counts_and_the_guard_element(name):
    import torch
    objs, lts = SCENES[name]()
    rays = batch()
    with query_context(name) as rt:
        for n in (1, 63, 64, 65, 257, 1024):
            part = rays[:n]
            want = fresh(objs, lts, part, 2, "shade_and_reflect")
            got = rt.query_shade(part, want=ALL)
            info = rt.query_shade_info()
            assert_shade(got, want, f"{name} n = {n}", info)
            assert_route(info, part, name)
            d_rays = torch.from_numpy(part.view(np.float32).reshape(-1, 8).copy()).cuda()
            out = guarded(n)
            shade = RTShade(**{k: out[k].data_ptr() for k in ALL})
            assert rt._lib.rt_query_shade_device(rt._ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(shade), None) == 0
            torch.cuda.synchronize()
            for k in ALL:
                a = out[k].cpu().numpy()
                assert np.array_equal(bits(a[:n]), bits(got[k])), (name, n, k)
                assert (a[n:] == GUARD[k]).all(), (name, n, k, "guard")
            only = guarded(n)
            shade = RTShade(t=only["t"].data_ptr())
            assert rt._lib.rt_query_shade_device(rt._ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(shade), None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(bits(only["t"].cpu().numpy()[:n]), bits(got["t"]))
            assert (only["rgba"].cpu().numpy() == GUARD["rgba"]).all() and (only["index"].cpu().numpy() == GUARD["index"]).all()


# ---- mixed routes in one wave -------------------------------------------------------------------------------------------------------
def test_mixed_routes_in_one_wave():
    objs, lts = scene_b()
    rays = batch()
    route = RY.query_shade_route(rays, *box_of("B"))
    for k in ("grid", "brute", "literal"):
        per_wave = route[k].reshape(-1, 64).sum(axis=1)
        assert (per_wave > 0).all() and (per_wave < 64).all(), k
    assert (route["brute"] & ~route["literal"]).sum() >= 16          # from outside the box: brute force, the default path behind it
    want = fresh(objs, lts, rays, 2, "shade_and_reflect")             # ONE fresh context: it renders the whole batch literally
    with query_context("B") as rt:
        got = rt.query_shade(rays, want=ALL)
        info = rt.query_shade_info()
    assert_shade(got, want, "mixed routes", info)
    assert_route(info, rays, "B")
    hit = want["index"] >= 0
    assert (hit & route["grid"]).sum() > 300 and (hit & route["brute"]).sum() > 16 and (~hit).sum() > 300
    assert info["rays_traced"] <= info["rays_reference"] and info["object_tests"] > 0


# ---- bit equality in every mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_bit_equality(mode):
    rays = batch()[:512]
    for name in ("A", "B"):
        objs, lts = SCENES[name]()
        for kernel in KERNELS:
            for depth in (0, 1, 5):
                label = f"{mode} {name} {kernel} {depth}"
                want = fresh(objs, lts, rays, depth, kernel, **MODES[mode])
                with query_context(name, depth, kernel, **MODES[mode]) as rt:
                    got = rt.query_shade(rays, want=ALL)
                    info = rt.query_shade_info()
                assert_shade(got, want, label, info)
                assert (want["index"] >= 0).sum() > 20, label


@pytest.mark.parametrize("name", ["A", "B"])
def test_zero_lights(name):
    objs, _ = SCENES[name]()
    none = R.lights_array([])
    rays = batch()[:512]
    for kernel in KERNELS:
        want = fresh(objs, none, rays, 2, kernel)
        with query_context(name, 2, kernel, lts=none) as rt:
            got = rt.query_shade(rays, want=ALL)
            assert_shade(got, want, f"no lights {name} {kernel}", rt.query_shade_info())
        assert (want["index"] >= 0).any() and not got["rgba"][:, :3].any()


# ---- an anchor outside the code under test ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_against_the_cpu_backend(name):
    """t and index exactly, |dRGB| <= 1e-5 (the project's standing bar against the oracle) on EVERY ray of the batch.
    tests/test_query_shade_cpu.py checks, without a GPU, that the CPU backend reproduces the oracle on these rays."""
    objs, lts = SCENES[name]()
    rays = batch()
    for kernel in KERNELS:
        cpu = CPURaytracer(objs, lts, rays, 2, kernel=kernel)
        frame = cpu.Render()
        q = cpu.query_shade(rays)
        with query_context(name, 2, kernel) as rt:
            got = rt.query_shade(rays, want=ALL)
        a, b = got["t"], q["t"]
        assert np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))), f"{name} {kernel}: t"
        assert np.array_equal(got["index"], q["index"]), f"{name} {kernel}: index"
        err = compare_frames(got["rgba"], frame)
        print(f"[{name} {kernel}] max |dRGB| against the CPU backend: {err:.3e}")
        assert err <= 1e-5, f"{name} {kernel}: max |dRGB| = {err}"
        assert np.array_equal(got["rgba"][:, 3], frame[:, 3])


# ---- live state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_the_live_state_is_what_is_queried(order):
    objs, lts = scene_b()
    rays = batch()[:768]
    rng = np.random.default_rng(5)
    moved = 17
    xf = R.transforms_of(objs[moved:moved + 1]).copy()
    mv, inv = instance((0.5, -0.5, -15.0), rotation((0.1, 0.9, 0.3), 0.4), (1.3, 0.9, 1.1))
    xf["mv"][0], xf["mvInverse"][0] = mv.reshape(-1), inv.reshape(-1)
    visible = (rng.uniform(size=len(objs)) > 0.2).astype(np.uint8)
    visible[moved] = 1
    mats = R.materials_of(objs[30:50]).copy()
    mats["absorption"] = 0.4
    mats["diffuse"][:, :3] = rng.uniform(0.2, 1.0, size=(len(mats), 3)).astype(F)
    new_lights = lts[:2].copy()
    new_lights["position"][1] = (-8.0, 5.0, 2.0, 1.0)
    steps = [("transforms", lambda c: c.set_transforms(xf, moved), lambda o, l: (R.with_transforms(o, xf, moved), l)),
             ("visibility", lambda c: c.set_visibility(visible), lambda o, l: (R.with_visibility(o, visible), l)),
             ("materials", lambda c: c.set_materials(mats, 30), lambda o, l: (R.with_materials(o, mats, 30), l)),
             ("lights", lambda c: c.set_lights(new_lights), lambda o, l: (o, new_lights))]
    if order == "backwards":
        steps.reverse()
    with query_context("B") as rt:
        first = rt.query_shade(rays, want=ALL)
        assert_shade(first, fresh(objs, lts, rays, 2, "shade_and_reflect"), "untouched", rt.query_shade_info())
        prev = first
        for label, act, apply in steps:
            act(rt)
            objs, lts = apply(objs, lts)
            got = rt.query_shade(rays, want=ALL)
            assert_shade(got, fresh(objs, lts, rays, 2, "shade_and_reflect"), f"{order}: after {label}", rt.query_shade_info())
            assert not np.array_equal(bits(got["rgba"]), bits(prev["rgba"])), label
            prev = got
        assert rt.geometry_info()["n_dynamic"] == 1
    hidden = np.nonzero(visible == 0)[0]
    assert not np.isin(prev["index"][prev["index"] >= 0], hidden).any()


# ---- the frame is left alone --------------------------------------------------------------------------------------------------------
def test_the_frame_is_left_alone():
    objs, lts = scene_b()
    rays = batch()[:600]
    want = fresh(objs, lts, rays, 2, "shade_and_reflect")
    turned = RY.posed_rays(W, H, Z, rotation((1.0, 0.1, 0.0), -0.1), (0.2, 0.1, 0.5))
    M, inside = rotation((0.2, 1.0, 0.1), 0.15), (0.5, -0.3, -1.0)
    states = [("camera", lambda c: None), ("pose", lambda c: c.set_pose(W, H, Z, M, inside)), ("ray buffer", lambda c: c.set_rays(turned)),
              ("camera again", lambda c: c.set_camera(W, H, Z)), ("shard", lambda c: c.set_shard(8 * W, 1, 2))]
    with query_context("B") as rt:
        for label, act in states:
            act(rt)
            before, info = snapshot(rt), rt.rays_info()
            assert_shade(rt.query_shade(rays, want=ALL), want, label)
            rt.pick_colour(np.arange(0, W * H, 37))
            assert same_snapshot(snapshot(rt), before), f"{label}: the frame after the queries"
            now = rt.rays_info()
            assert all(np.array_equal(np.asarray(info[k]), np.asarray(now[k])) for k in info), label
    with hip(objs, lts, None, 2, camera=(W // 2, H // 2, Z / 2), supersample=2) as rt:      # a supersampled context
        before = rt.Render().copy()
        packed = rt.render_packed().copy()
        assert_shade(rt.query_shade(rays, want=ALL), want, "supersampled")
        assert np.array_equal(bits(rt.Render()), bits(before)) and np.array_equal(rt.render_packed(), packed)


# ---- mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_masked_rays_read_as_misses_and_are_not_counted(name):
    import torch
    objs, lts = SCENES[name]()
    rays = batch()[:700]
    mask = np.where(np.arange(700) % 3 == 1, -1 - np.arange(700) % 5, np.arange(700) % 4).astype(np.int32)
    off = mask < 0
    want = fresh(objs, lts, rays, 2, "shade_and_reflect")
    sub = fresh(objs, lts, rays[~off], 2, "shade_and_reflect")
    with query_context(name) as rt:
        got = rt.query_shade(rays, mask, want=ALL)
        info = rt.query_shade_info()
        assert_route(info, rays, name, mask=mask)
        assert (info["rays_reference"], info["hit_rays"]) == (sub["rays_reference"], sub["hit_rays"])
        d = rt.query_shade(torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(mask).cuda(), want=ALL)
        torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(bits(got[k][~off]), bits(want[k][~off])), k
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(got[k])), k
    assert (got["rgba"][off] == np.array([0, 0, 0, 1], dtype=F)).all() and (got["t"][off] == MAX_FLOAT).all() and (got["index"][off] == -1).all()
    assert (want["index"][off] >= 0).sum() > 20


# ---- literal contexts ---------------------------------------------------------------------------------------------------------------
def test_a_context_created_literal():
    objs, lts = scene_b()
    rays = batch()[:512]
    want = fresh(objs, lts, rays, 2, "shade_and_reflect")
    with query_context("B", literal=True) as rt:
        got = rt.query_shade(rays, want=ALL)
        info = rt.query_shade_info()
    assert_shade(got, want, "literal=True", info)
    assert (info["n_grid"], info["n_brute"], info["n_literal"]) == (0, 512, 512)
    assert info["rays_traced"] == info["rays_reference"]


@pytest.mark.parametrize("kind", ["zero", "inf"])
def test_a_degenerate_instance(kind):
    base, lts = scene_b()
    where = int(np.nonzero(base["type"] == R.SPHERE)[0][30])
    objs = base.copy()
    inv = objs["mvInverse"][where].reshape(4, 4).copy()
    if kind == "zero":
        inv[:3, :3] = 0.0
    else:
        inv[2, 2] = np.inf
        inv[3, 2] = np.nan
        objs["mv"][where].reshape(4, 4)[2, 2] = 0.0
    objs["mvInverse"][where] = inv.reshape(16)
    rays = batch()[:512]
    want = fresh(objs, lts, rays, 2, "shade_and_reflect")
    assert not np.array_equal(bits(want["rgba"]), bits(fresh(base, lts, rays, 2, "shade_and_reflect")["rgba"]))
    with hip(objs, lts, None, 2, camera=(W, H, Z)) as rt:
        assert rt.rays_info()["literal"] == 1
        got = rt.query_shade(rays, want=ALL)
        info = rt.query_shade_info()
    assert_shade(got, want, f"degenerate {kind}", info)
    assert (info["n_grid"], info["n_brute"], info["n_literal"]) == (0, 512, 512)


# ---- pick ---------------------------------------------------------------------------------------------------------------------------
def test_pick_colour():
    objs, lts = scene_b()
    items = np.concatenate([[0, W * H - 1, W - 1, W], np.random.default_rng(3).integers(0, W * H, size=46)]).astype(np.uint64)
    with query_context("B") as rt:
        frame = rt.Render().copy()
        t, index = rt.render_aux()
        got = rt.pick_colour(items, want=ALL)
        assert rt.query_shade_info()["n_rays"] == 50
        k = items.astype(np.int64)
        assert np.array_equal(bits(got["rgba"]), bits(frame[k])) and np.array_equal(bits(got["t"]), bits(t[k])) and np.array_equal(got["index"], index[k])
        assert (index[k] >= 0).any() and (index[k] < 0).any()
        hit = int(np.nonzero(index >= 0)[0][0])
        one = rt.pick_colour(hit % W, hit // W)
        assert one.shape == (4,) and np.array_equal(bits(one), bits(frame[hit])) and one[:3].any()
        rt.set_shard(8 * W, 1, 2)            # frame work-items, regardless of the shard
        assert np.array_equal(bits(rt.pick_colour(items)["rgba"]), bits(frame[k]))


def test_pick_without_rays_is_refused():
    from opencl_raytracer_amd.hip_raytracer import load_library
    lib = load_library()
    objs, lts = (np.ascontiguousarray(a) for a in scene_b())
    ctx = VP()
    assert lib.rt_create(ctypes.byref(ctx), objs.ctypes.data_as(VP), len(objs), lts.ctypes.data_as(VP), len(lts), None, W * H, 2, 2, 0, 0) == 0
    try:
        items = np.arange(4, dtype=np.uint64)
        rgba = np.full((4, 4), 5.0, dtype=F)
        shade = RTShade(rgba=rgba.ctypes.data)
        assert lib.rt_query_primary_shade(ctx, items.ctypes.data_as(VP), 4, ctypes.byref(shade)) == -5   # RT_ERR_STATE
        assert lib.rt_last_error(ctx) and (rgba == 5.0).all()
        info = RTQueryShadeInfo()
        assert lib.rt_get_query_shade_info(ctx, ctypes.byref(info)) == -5                              # no shaded query yet
        rays = batch()[:3]
        assert lib.rt_query_shade(ctx, rays.ctypes.data_as(VP), 3, None, ctypes.byref(shade)) == 0       # rays of the caller's own need none
        assert (rgba[:3, 3] == 1.0).all() and (rgba[3] == 5.0).all()
        assert lib.rt_get_query_shade_info(ctx, ctypes.byref(info)) == 0 and info.n_rays == 3
    finally:
        lib.rt_destroy(ctx)


# ---- the device form ----------------------------------------------------------------------------------------------------------------
def test_device_form_behind_a_torch_kernel_on_another_stream():
    import torch
    rays = batch()
    source = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_rays = torch.full_like(source, float("nan"))   # until the torch kernel has run, every ray is a NaN ray
    work = torch.full((1024, 1024), 1.0 / 1024.0, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with query_context("B") as dev, query_context("B") as host:
        with torch.cuda.stream(side):
            for _ in range(4):
                work = work @ work
            torch.mul(source, 1.0, out=d_rays)
            got = dev.query_shade(d_rays, want=ALL)
        assert all(v.is_cuda for v in got.values()) and got["rgba"].shape == (len(rays), 4) and got["index"].dtype == torch.int32
        side.synchronize()
        info = dev.query_shade_info()
        want = host.query_shade(rays, want=ALL)
        for k in ALL:
            assert np.array_equal(bits(got[k].cpu().numpy()), bits(want[k])), k
        assert_route(info, rays, "B")
        assert torch.equal(d_rays.view(torch.int32), source.view(torch.int32))   # the input is unchanged
        again = dev.query_shade(source)                                           # the legacy default stream; rgba alone
        torch.cuda.synchronize()
        assert list(again) == ["rgba"] and np.array_equal(bits(again["rgba"].cpu().numpy()), bits(want["rgba"]))
        assert dev.query_shade(source[:0])["rgba"].numel() == 0
        with pytest.raises(ValueError):
            dev.query_shade(source, want=("colour",))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_n_zero_change_nothing():
    import torch
    n = 16
    rays = batch()[:n]
    d_rays = torch.from_numpy(np.concatenate([rays.view(np.float32).reshape(-1), np.zeros(8, dtype=F)])).cuda()
    out = guarded(n + 1)
    host = {"rgba": np.full((n, 4), 5.0, dtype=F), "t": np.full(n, 5.0, dtype=F), "index": np.full(n, 9, dtype=np.int32)}
    h_shade = RTShade(**{k: v.ctypes.data for k, v in host.items()})
    items = np.array([0, 1, W * H], dtype=np.uint64)
    r_ptr = rays.ctypes.data_as(VP)

    def dev(rays_at=0, mask_at=None, **offsets):
        shade = RTShade(**{k: out[k].data_ptr() + offsets.get(k, 0) for k in ALL})
        mask = None if mask_at is None else VP(out["index"].data_ptr() + mask_at)
        return lambda: lib.rt_query_shade_device(ctx, VP(d_rays.data_ptr() + rays_at), n, mask, ctypes.byref(shade), None)

    with query_context("B") as rt:
        before = snapshot(rt)
        first = rt.query_shade(rays, want=ALL)
        info = rt.query_shade_info()
        lib, ctx = rt._lib, rt._ctx
        refused = [dev(rgba=4), dev(rgba=8), dev(t=2), dev(index=1), dev(rays_at=4), dev(rays_at=8), dev(mask_at=2),
                   lambda: lib.rt_query_shade_device(ctx, None, 3, None, ctypes.byref(RTShade(t=out["t"].data_ptr())), None),    # NULL rays, n != 0
                   lambda: lib.rt_query_shade_device(ctx, VP(d_rays.data_ptr()), n, None, ctypes.byref(RTShade()), None),       # all members NULL
                   lambda: lib.rt_query_shade_device(ctx, VP(d_rays.data_ptr()), n, None, None, None),                          # no struct
                   lambda: lib.rt_query_shade(ctx, None, 3, None, ctypes.byref(h_shade)), lambda: lib.rt_query_shade(ctx, r_ptr, n, None, ctypes.byref(RTShade())),
                   lambda: lib.rt_query_shade(ctx, r_ptr, n, None, None),
                   lambda: lib.rt_query_primary_shade(ctx, items.ctypes.data_as(VP), 3, ctypes.byref(h_shade)),                  # a work-item >= the ray count
                   lambda: lib.rt_query_primary_shade(ctx, None, 3, ctypes.byref(h_shade)),
                   lambda: lib.rt_query_primary_shade(ctx, items.ctypes.data_as(VP), 2, ctypes.byref(RTShade()))]
        for k, call in enumerate(refused):
            assert call() == -1, k
            assert lib.rt_last_error(ctx), k
        for call in (lambda: lib.rt_query_shade(ctx, None, 0, None, ctypes.byref(h_shade)),
                     lambda: lib.rt_query_shade_device(ctx, None, 0, None, ctypes.byref(RTShade(t=out["t"].data_ptr())), None),
                     lambda: lib.rt_query_primary_shade(ctx, None, 0, ctypes.byref(h_shade))):
            assert call() == 0                 # n == 0 is RT_OK and launches nothing
        torch.cuda.synchronize()
        for k, tensor in out.items():
            assert (tensor.cpu().numpy() == GUARD[k]).all(), k
        assert (host["rgba"] == 5.0).all() and (host["t"] == 5.0).all() and (host["index"] == 9).all()
        assert rt.query_shade_info() == info   # the last shaded query is still the last one
        assert same_snapshot(snapshot(rt), before)
        again = rt.query_shade(rays, want=ALL)
        assert all(np.array_equal(bits(again[k]), bits(first[k])) for k in ALL)
        # a plain query has its own counter block
        rt.query_closest(rays[:5])
        assert rt.query_info()["n_rays"] == 5 and rt.query_shade_info()["n_rays"] == n


def test_hittest_and_triangle_contexts_are_refused():
    from test_frame_shapes_cpu import camera_z_for, scene
    objs, lts = scene_b()
    rays = batch()[:8]
    rgba = np.full((8, 4), 5.0, dtype=F)
    shade = RTShade(rgba=rgba.ctypes.data)
    items = np.arange(8, dtype=np.uint64)
    tri, tri_lights = scene("tri")
    cases = [("hittest", hip(objs, lts, None, 0, camera=(W, H, Z), kernel="hittest"), b"colour"),
             ("triangles", hip(tri, tri_lights, None, 2, camera=(W, H, camera_z_for("tri", W, H))), b"triangle")]
    for label, rt, word in cases:
        with rt:
            before = snapshot(rt) if label == "triangles" else rt.Render().copy()
            lib, ctx = rt._lib, rt._ctx
            assert lib.rt_query_shade(ctx, rays.ctypes.data_as(VP), 8, None, ctypes.byref(shade)) == -5, label   # RT_ERR_STATE
            assert word in lib.rt_last_error(ctx), label
            assert lib.rt_query_primary_shade(ctx, items.ctypes.data_as(VP), 8, ctypes.byref(shade)) == -5, label
            with pytest.raises(RTError):
                rt.query_shade(rays)
            assert (rgba == 5.0).all()
            after = snapshot(rt) if label == "triangles" else rt.Render()
            assert same_snapshot(after, before) if label == "triangles" else np.array_equal(bits(after), bits(before))
