"""No GPU: replaceable rays (hip_raytracer.h, "replaceable rays") - the boundary, the two executable definitions of
opencl_raytracer_amd/rays.py, the CPU backend's SetRays, and the inputs tests/test_set_rays_gpu.py renders.

`scan_cases(n)` is the list of ray arrays the GPU scan is held to ray_verdict on; here ray_verdict itself is held to what
each case was BUILT to be (the flags are written down next to the construction; a box case asserts that the ray its label
names is the extreme). `POSES` are the views
a live context is walked through; the oracle alone says that each of them sees the scene."""
import ctypes
import re

import numpy as np
import pytest

from helpers import R, ROOT, rotation
from opencl_raytracer_amd import rays as RY
from test_frame_shapes_cpu import DEPTH, MIN_HIT_SHARE, MIN_MISS_SHARE, MIN_RAYS_PER_PIXEL, camera_z_for, pinhole_rays, scene

F = np.float32
SYMBOLS = ("rt_set_rays_device", "rt_set_rays", "rt_get_rays_info")
SCAN_COUNTS = (1, 63, 64, 65, 257, 1800, 9216, 300001)   # below, at, above a wave; ragged last workgroups; > one trip of the grid-stride loop

# ---- the views ----------------------------------------------------------------------------------------------------------
CONTEXTS = [("s40", "shade_and_reflect", (36, 50)), ("s80", "shade", (36, 50)), ("s300", "shade_and_reflect", (96, 96)),
            ("s300", "hittest", (96, 96)), ("tri", "shade_and_reflect", (128, 72))]


def euler(yaw=0.0, pitch=0.0, roll=0.0):
    """Ry(yaw) Rx(pitch) Rz(roll), degrees."""
    return rotation((0, 1, 0), np.radians(yaw)) @ rotation((1, 0, 0), np.radians(pitch)) @ rotation((0, 0, 1), np.radians(roll))


# name -> (rotation, origin, scale of the rule's z). A pan about the origin is physically exact for this renderer (the eye is
# the origin); "moved" stays inside the box every grid is built for; "far" leaves it (40 in front of a cloud at z < 0).
POSES = {"pan": (euler(12, -7, 30), (0.0, 0.0, 0.0), 1.0),
         "moved": (euler(-9, 5, 0), (0.5, -0.5, 1.0), 1.0),
         "far": (euler(0, 0, 15), (0.0, 0.0, 40.0), 3.0)}


def tri_moved_origin(box_lo):
    """The "moved" origin of the mesh scene, whose box ends at z = 0 (the camera's origin): a tenth of the way into it."""
    return (0.5, -0.5, float(F(0.1 * box_lo[2])))


def pose_rays(name, W, H, pose, origin=None):
    M, o, zs = POSES[pose]
    return RY.posed_rays(W, H, camera_z_for(name, W, H, zs), M, o if origin is None else origin)


def tri_box():
    """build_grid's box for the mesh scene (rt_scene.cpp): the origin united with every guard sphere padded by 1 %."""
    objs, _ = scene("tri")
    gs = objs["mvInverse"].reshape(len(objs), 16)[:, :4].astype(np.float64)
    return np.minimum(0.0, (gs[:, :3] - 1.01 * gs[:, 3:4]).min(0)), np.maximum(0.0, (gs[:, :3] + 1.01 * gs[:, 3:4]).max(0))


def sees_the_scene(want, n, kernel, label):
    """The conditions of test_frame_shapes_cpu.py on an oracle result."""
    hit = float((want["hit_index"] >= 0).mean())
    assert hit >= MIN_HIT_SHARE and 1.0 - hit >= MIN_MISS_SHARE, (label, hit)
    if kernel == "shade_and_reflect":
        assert want["rays_ref"] / n >= MIN_RAYS_PER_PIXEL, (label, want["rays_ref"] / n)


# ---- the scan's cases ---------------------------------------------------------------------------------------------------
def good_rays(n, seed=5):
    """Starts in [1, 2)^3 with w = 1, directions of length about 1..3 with w = 0: every predicate holds."""
    rng = np.random.default_rng(seed + n)
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays["start"][:, :3] = rng.uniform(1.0, 2.0, size=(n, 3))
    rays["start"][:, 3] = 1.0
    d = rng.normal(size=(n, 3))
    d[np.abs(d).sum(axis=1) < 0.1] = 1.0
    rays["direction"][:, :3] = d * rng.uniform(1.0, 2.0, size=(n, 1))
    return rays


OFFENCES = {   # name -> (field, value, the predicate it breaks)
    "direction.w = 1": ("direction", (None, None, None, 1.0), "dir_w_zero"),
    "direction 0": ("direction", (0.0, 0.0, 0.0, 0.0), "directions_in_domain"),
    "components 1e-16": ("direction", (1e-16, 1e-16, 1e-16, 0.0), "directions_in_domain"),      # |d|^2 = 3e-32 < 1e-30
    "components 1e16": ("direction", (1e16, 1e16, 1e16, 0.0), "directions_in_domain"),          # |d|^2 = 3e32 > 1e30
    "NaN direction": ("direction", (1.0, np.nan, 1.0, 0.0), "directions_in_domain"),
    "start.w = 0": ("start", (None, None, None, 0.0), "starts_ok"),
    "NaN start": ("start", (np.nan, 1.0, 1.0, 1.0), "starts_ok"),
    "infinite start": ("start", (1.0, np.inf, 1.0, 1.0), "starts_ok"),
    "start (3e38, 3e38, 0)": ("start", (3e38, 3e38, 0.0, 1.0), "starts_ok"),                    # finite components, fp32 sum overflows
}


def scan_cases(n):
    """[(label, rays, expectation)]: expectation = dict of the three flags and, where starts_ok, origin_lo / origin_hi as BUILT
    (None: whatever the random base gives - compare with ray_verdict only)."""
    base = good_rays(n)
    ok = dict(dir_w_zero=True, directions_in_domain=True, starts_ok=True)
    cases = [("all good", base.copy(), dict(ok, box=None))]
    places = sorted({0, n - 1} | ({63} if n > 63 else set()))
    for name, (field, value, breaks) in OFFENCES.items():
        for at in places:
            rays = base.copy()
            for k, v in enumerate(value):
                if v is not None:
                    rays[field][at, k] = v
            cases.append((f"{name} at {at}", rays, dict(ok, box=None, **{breaks: False})))

    def boxed(label, at, start, extreme, shift=0.0):
        """Ray `at` starts at `start`, the others at base + shift; `extreme` says which end of the box that ray must be."""
        rays = base.copy()
        rays["start"][:, :3] += F(shift)
        rays["start"][at, :3] = start
        others = np.delete(rays["start"][:, :3], at, axis=0)
        want_lo = np.minimum(others.min(0), start) if len(others) else start
        want_hi = np.maximum(others.max(0), start) if len(others) else start
        assert np.array_equal(want_lo if extreme == "lo" else want_hi, start)   # the case is what its label says
        cases.append((label, rays, dict(ok, box=(want_lo, want_hi))))
    boxed("the minimum, negative, at n - 1", n - 1, np.array([-5.0, -6.5, -7.25], F), "lo")
    boxed("the maximum at 0", 0, np.array([9.0, 10.5, 11.25], F), "hi")
    zero = np.array([-0.0, -0.0, -0.0], F)
    boxed("-0.0 below positive starts", n // 2, zero, "lo")
    boxed("-0.0 above negative starts", n // 2, zero, "hi", shift=-4.0)   # raw bits of a negative float order the wrong way round
    den = np.array([1e-45, 3e-45, 1e-40], F)
    boxed("a denormal below positive starts", n - 1, den, "lo")
    boxed("a negative denormal above negative starts", 0, -den, "hi", shift=-4.0)
    return cases


def check_verdict(got, want, label):
    """`got`: a ray_verdict-shaped dict (flags as bools, origin_lo / origin_hi arrays or None)."""
    for key in ("dir_w_zero", "directions_in_domain", "starts_ok"):
        assert bool(got[key]) == bool(want[key]), f"{label}: {key} is {got[key]}, expected {want[key]}"
    if want["starts_ok"] and want.get("origin_lo") is not None:
        # as NUMBERS: -0.0 == 0.0 holds, a flushed denormal or a bit-ordered extreme does not
        assert np.array_equal(np.asarray(got["origin_lo"], F), np.asarray(want["origin_lo"], F)), f"{label}: origin_lo {got['origin_lo']} != {want['origin_lo']}"
        assert np.array_equal(np.asarray(got["origin_hi"], F), np.asarray(want["origin_hi"], F)), f"{label}: origin_hi {got['origin_hi']} != {want['origin_hi']}"


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_header_and_wrapper_declare_the_entry_points():
    from opencl_raytracer_amd import hip_raytracer as hr
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in hr.EXPORTS
    assert "typedef struct rt_rays_info_t" in text
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert hasattr(hr.HIPRaytracer, "set_rays") and hasattr(hr.HIPRaytracer, "rays_info")


def test_library_exports_them_and_refuses_a_null_context_without_a_device():
    from opencl_raytracer_amd import hip_raytracer as hr
    if not hr.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = hr.load_library()
    assert lib.rt_abi_version() == 3
    rays = good_rays(4)
    info = hr.RTRaysInfo()
    assert lib.rt_set_rays_device(None, rays.ctypes.data_as(ctypes.c_void_p), 4, None) == -1
    assert lib.rt_set_rays(None, rays.ctypes.data_as(ctypes.c_void_p), 4) == -1
    assert lib.rt_get_rays_info(None, ctypes.byref(info)) == -1
    assert ctypes.sizeof(hr.RTRaysInfo) == 104   # 4 u32, 2 x 3 floats, 2 x 3 doubles, 4 u32


@pytest.mark.parametrize("n", (1, 63, 65, 257, 1800))
def test_ray_verdict_on_hand_made_arrays(n):
    cases = scan_cases(n)
    assert len(cases) == 1 + len(OFFENCES) * (3 if n > 63 else (2 if n > 1 else 1)) + 6
    for label, rays, want in cases:
        got = RY.ray_verdict(rays)
        expect = dict(want)
        if want["box"] is not None:
            expect["origin_lo"], expect["origin_hi"] = want["box"]
        check_verdict(got, expect, f"n = {n}, {label}")
        assert (got["origin_lo"] is None) == (not want["starts_ok"]), label
        if want["starts_ok"]:   # against the definition in float64: min / max of exactly representable numbers
            s = rays["start"][:, :3].astype(np.float64)
            assert np.array_equal(got["origin_lo"].astype(np.float64), s.min(0)) and np.array_equal(got["origin_hi"].astype(np.float64), s.max(0)), label


def test_ray_verdict_keeps_the_order_of_operations():
    """(dx*dx + dy*dy) + dz*dz in float32: 1e19^2 overflows no float32 sum on its own terms but 3e38 + 3e38 does; and the window's
    edges are exclusive."""
    rays = good_rays(3)
    rays["direction"][0, :3] = (1e15, 0.0, 0.0)          # dd = 1e30 as float32 rounds it: not < 1e30f
    assert RY.ray_verdict(rays)["directions_in_domain"] == bool(F(1e15) * F(1e15) < F(1e30))
    rays["direction"][0, :3] = (9e14, 0.0, 0.0)
    assert RY.ray_verdict(rays)["directions_in_domain"]
    rays["direction"][0, :3] = (1.5e19, 1.5e19, 0.0)      # each square 2.25e38 is finite, their float32 sum is inf
    assert not RY.ray_verdict(rays)["directions_in_domain"]
    rays = good_rays(3)
    rays["start"][1, :3] = (3e38, -3e38, 3e38)            # (sx + sy) + sz = 3e38: finite, left to right
    assert RY.ray_verdict(rays)["starts_ok"]
    rays["start"][1, :3] = (3e38, 3e38, -3e38)            # (sx + sy) overflows first
    assert not RY.ray_verdict(rays)["starts_ok"]


def test_posed_rays_with_the_identity_is_the_pinhole_grid():
    for W, H, z in ((36, 50, -75.0), (7, 5, 0.0), (96, 96, 76.8), (1, 9, -1e-16)):
        assert RY.posed_rays(W, H, z, np.eye(3)).tobytes() == pinhole_rays(W, H, z).tobytes()
    M, origin, _ = POSES["moved"]
    rays = RY.posed_rays(36, 50, -75.0, M, origin)
    grid = pinhole_rays(36, 50, -75.0)["direction"][:, :3]
    Mf = M.astype(F)
    k = 36 * 17 + 5   # one ray by hand, in the stated order
    want = [F(F(F(Mf[r, 0] * grid[k, 0]) + F(Mf[r, 1] * grid[k, 1])) + F(Mf[r, 2] * grid[k, 2])) for r in range(3)]
    assert [rays["direction"][k, r] for r in range(3)] == want and rays["direction"][k, 3] == 0
    assert np.array_equal(rays["start"], np.tile(np.array([0.5, -0.5, 1.0, 1.0], F), (1800, 1)))
    v = RY.ray_verdict(rays)
    assert v["dir_w_zero"] and v["directions_in_domain"] and v["starts_ok"] and np.array_equal(v["origin_lo"], v["origin_hi"])


def test_cpu_backend_set_rays_renders_the_oracles_frame(restatement):
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    objs, lights = scene("s40")
    W, H = 36, 50
    first = pinhole_rays(W, H, camera_z_for("s40", W, H))
    for kernel in ("shade_and_reflect", "hittest"):
        rt = CPURaytracer(objs, lights, first, DEPTH, kernel=kernel)
        before = rt.Render()
        for pose in ("pan", "far"):
            rays = pose_rays("s40", W, H, pose)
            rt.set_rays(rays)
            got = rt.Render()
            want = restatement[True].render(kernel, objs, lights, rays, DEPTH)["out"]
            same = (got == want) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{kernel} {pose}: {int((~same).sum())} values differ from the oracle"
            assert not np.array_equal(got, before)
        with pytest.raises(ValueError):
            rt.set_rays(first[:-1])


@pytest.mark.parametrize("name,shape", sorted({(name, shape) for name, _, shape in CONTEXTS}))
def test_every_pose_sees_the_scene(restatement, name, shape):
    """Conditions on the inputs of test_set_rays_gpu.py, from the oracle alone (the hittest context renders the rays of the s300
    shade_and_reflect context)."""
    objs, lights = scene(name)
    W, H = shape
    lo, hi = tri_box()
    for pose in POSES:
        if name == "tri" and pose == "far":
            continue   # refused: a mesh is traced by the grid only
        origin = tri_moved_origin(lo) if (name == "tri" and pose == "moved") else None
        rays = pose_rays(name, W, H, pose, origin)
        o = rays["start"][0, :3].astype(np.float64)
        if name == "tri":
            assert (o >= lo).all() and (o <= hi).all(), (pose, o, lo, hi)
        want = restatement[True].render("shade_and_reflect", objs, lights, rays, DEPTH)
        sees_the_scene(want, W * H, "shade_and_reflect", f"{name} {pose}")
