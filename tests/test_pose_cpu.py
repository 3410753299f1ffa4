"""No GPU: posed cameras (hip_raytracer.h, "posed cameras") - the boundary, the CPU backend's SetPose against SetRays on
rays.posed_rays, the wrappers' argument validation, scene_tool --pose, and the inputs tests/test_pose_gpu.py renders."""
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT, rotation
from opencl_raytracer_amd import camera, rays as RY
from test_frame_shapes_cpu import DEPTH, camera_z_for, pinhole_rays, scene
from test_set_rays_cpu import euler

F = np.float32
SYMBOLS = ("rt_set_pose", "rt_generate_rays_device", "rt_set_pose_multi")

# ---- the generator's cases ----------------------------------------------------------------------------------------------
# below and at a wave (64), a ragged second workgroup (256), many workgroups; one row, one column; widths that are no multiple of
# either; the last one has more rays than one trip of the generator's launch writes (1024 workgroups x 256 rays = 262 144), so
# some lanes take a second ray
SHAPES = ((1, 1), (3, 5), (64, 1), (1, 64), (65, 7), (130, 3), (257, 129), (520, 505))
NON_ORTHONORMAL = np.array([[1.5, 0.0, -0.25], [-2.0, 0.75, 0.0], [0.0, -0.5, 3.0]])   # a zero in every row, negative entries
MATRICES = {"identity": np.eye(3),
            "about x": rotation((1, 0, 0), np.radians(25.0)),
            "about y": rotation((0, 1, 0), np.radians(-40.0)),
            "about z": rotation((0, 0, 1), np.radians(100.0)),
            "yaw pitch roll": euler(12, -7, 30),
            "non-orthonormal": NON_ORTHONORMAL}
ORIGINS = ((0.0, 0.0, 0.0), (1.5, -2.25, 1e3))


def depths(height):
    """A camera_z value (negative, no round number) and a positive z."""
    return (float(camera.camera_z(max(height, 2))), 7.75)


# what leaves the default path's domain or the scan's start predicate: (matrix, origin) -> the verdict it was BUILT to get
OFF_DOMAIN = {"M = 0": (np.zeros((3, 3)), (0.0, 0.0, 0.0), dict(directions_in_domain=False, starts_ok=True)),
              "M with a NaN": (np.array([[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]]), (0.0, 0.0, 0.0), dict(directions_in_domain=False, starts_ok=True)),
              "M scaled by 1e20": (np.eye(3) * 1e20, (0.0, 0.0, 0.0), dict(directions_in_domain=False, starts_ok=True)),   # dd overflows
              "origin with an inf": (np.eye(3), (0.0, np.inf, 0.0), dict(directions_in_domain=True, starts_ok=False))}


def test_header_and_wrappers_carry_the_new_names():
    from opencl_raytracer_amd import cpu_raytracer, distributed, hip_raytracer as hr
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in hr.EXPORTS
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert "posed cameras" in header and "ray buffer generated from a pose" in header
    for cls, names in ((hr.HIPRaytracer, ("set_pose", "generate_rays")), (hr.MultiHIPRaytracer, ("set_pose",)),
                       (distributed.ShardedHIPRaytracer, ("set_pose",)), (cpu_raytracer.CPURaytracer, ("set_pose",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert "rt_set_pose" in RY.__doc__
    for host, needle in (("HIPRaytracer.hpp", "void SetPose("), ("CPURaytracer.hpp", "void SetPose(")):
        assert needle in (ROOT / "opencl-raytracer_amd" / "host" / host).read_text(), host


def test_library_exports_them_and_refuses_a_null_context_without_a_device():
    from opencl_raytracer_amd import hip_raytracer as hr
    if not hr.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = hr.load_library()
    assert lib.rt_abi_version() == 3
    m, o = hr.pose_arguments(np.eye(3))
    assert lib.rt_set_pose(None, 4, 4, -1.0, m, o, None) == -1
    assert lib.rt_generate_rays_device(None, 4, 4, -1.0, m, o, None, None) == -1
    assert lib.rt_set_pose_multi(None, 4, 4, -1.0, m, o) == -1


def test_pose_arguments_round_like_posed_rays_and_refuse_other_shapes():
    from opencl_raytracer_amd import hip_raytracer as hr
    M = euler(12, -7, 30)
    m, o = hr.pose_arguments(M, (0.1, 0.2, 1e3))
    assert np.array_equal(np.array(list(m), F), M.astype(F).reshape(9))   # row-major, float64 -> float32 once
    assert np.array_equal(np.array(list(o), F), np.array([0.1, 0.2, 1e3], F))
    for bad in (np.eye(4), np.zeros(9), [[1, 0, 0], [0, 1, 0]]):
        with pytest.raises(ValueError):
            hr.pose_arguments(bad)
        with pytest.raises(ValueError):
            RY.posed_rays(2, 2, -1.0, bad)
    for bad in ((0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 3.0):
        with pytest.raises(ValueError):
            hr.pose_arguments(np.eye(3), bad)


def test_the_cases_are_what_their_labels_say():
    """The inputs of the GPU tests, from the definitions alone."""
    rays_per_trip = 1024 * 256
    counts = [w * h for w, h in SHAPES]
    assert min(counts) == 1 and max(counts) > rays_per_trip and 64 in counts   # one lane, a second trip of the launch, exactly a wave
    assert any(c < 64 for c in counts) and any(256 < c < 512 and c % 64 for c in counts) and any(2048 < c < rays_per_trip for c in counts)
    assert all((row == 0).any() for row in NON_ORTHONORMAL) and (NON_ORTHONORMAL < 0).sum() >= 3
    assert abs(np.linalg.det(NON_ORTHONORMAL)) > 0.1 and not np.allclose(NON_ORTHONORMAL @ NON_ORTHONORMAL.T, np.eye(3))
    for label, M in MATRICES.items():
        if label not in ("identity", "non-orthonormal"):
            assert np.allclose(M @ M.T, np.eye(3)) and not np.array_equal(M.astype(F).astype(np.float64), M), label   # rounded from float64
    for W, H in SHAPES[:-1]:
        for z in depths(H):
            for label, M in MATRICES.items():
                for origin in ORIGINS:
                    v = RY.ray_verdict(RY.posed_rays(W, H, z, M, origin))
                    assert v["dir_w_zero"] and v["directions_in_domain"] and v["starts_ok"], (W, H, z, label)
                    assert np.array_equal(v["origin_lo"], np.array(origin, F)) and np.array_equal(v["origin_hi"], np.array(origin, F))
    for label, (M, origin, built) in OFF_DOMAIN.items():
        v = RY.ray_verdict(RY.posed_rays(32, 24, -20.0, M, origin))
        assert v["dir_w_zero"], label
        assert (v["directions_in_domain"], v["starts_ok"]) == (built["directions_in_domain"], built["starts_ok"]), label


@pytest.mark.parametrize("kernel", ("shade_and_reflect", "hittest"))
def test_cpu_backend_set_pose_is_set_rays_on_posed_rays(kernel):
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    objs, lights = scene("s40")
    W, H = 36, 50
    z = camera_z_for("s40", W, H)
    first = pinhole_rays(W, H, z)
    posed = CPURaytracer(objs, lights, first, DEPTH, kernel=kernel)
    replaced = CPURaytracer(objs, lights, first, DEPTH, kernel=kernel)
    before = posed.Render()
    for label, M, origin in (("yaw pitch roll", MATRICES["yaw pitch roll"], ORIGINS[0]), ("non-orthonormal", NON_ORTHONORMAL, (0.5, -0.5, 1.0)),
                             ("identity", np.eye(3), ORIGINS[0]), ("M = 0", np.zeros((3, 3)), ORIGINS[0])):
        posed.set_pose(W, H, z, M, origin)
        replaced.set_rays(RY.posed_rays(W, H, z, M, origin))
        got, want = posed.Render(), replaced.Render()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kernel}, {label}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
        assert np.array_equal(got.view(np.uint32), before.view(np.uint32)) == (label == "identity"), label
    posed.set_rays(first)   # a later set_rays replaces the pose
    assert np.array_equal(posed.Render().view(np.uint32), before.view(np.uint32))
    for bad in ((W + 1, H), (W, H - 1), (0, 0)):
        with pytest.raises(ValueError):
            posed.set_pose(*bad, z, np.eye(3))
    with pytest.raises(ValueError):
        posed.set_pose(W, H, z, np.eye(4))
    with pytest.raises(ValueError):
        posed.set_pose(W, H, z, np.eye(3), (0.0, 1.0))


def _scene_tool(args, out):
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([str(tool), *args], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return out.read_bytes()


def test_scene_tool_cpu_takes_a_pose(tmp_path):
    """--pose with the identity is the unposed picture, byte for byte; a real pose is the P3 of the Python CPU backend's frame of
    posed_rays; and --pose combines with --ss."""
    from opencl_raytracer_amd import ppm, resolve, scene_loader
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    scene_file = ROOT / "scenes" / "simpleSphere.txt"
    W, H = 32, 24
    z = camera.camera_z(H)
    zbits = f"{int(F(z).view(np.uint32)):08x}"
    plain, same, turned, fine = (tmp_path / n for n in ("plain.ppm", "identity.ppm", "turned.ppm", "fine.ppm"))
    base = ["render", str(scene_file), str(W), str(H), "2"]
    unposed = _scene_tool(base + [str(plain), zbits, "cpu"], plain)
    assert _scene_tool(base + [str(same), zbits, "cpu", "--pose", "1,0,0,0,1,0,0,0,1,0,0,0"], same) == unposed
    M, origin = MATRICES["about z"].astype(F), (0.25, -0.5, 0.5)
    text = ",".join(repr(float(v)) for v in list(M.reshape(9)) + list(origin))
    objs, lights = scene_loader.load_scene(str(scene_file))
    got = _scene_tool(["render", "--pose", text] + base[1:] + [str(turned), zbits, "cpu"], turned)
    frame = CPURaytracer(objs, lights, RY.posed_rays(W, H, z, M, origin), 2).Render()
    assert got == ppm.format_p3(W, H, ppm.rgba_to_rgb(frame)) and got != unposed
    s = 2
    sw, sh, sz = camera.supersampled(W, H, z, s)
    got = _scene_tool(base + [str(fine), zbits, "cpu", "--ss", str(s), "--pose", text], fine)
    samples = CPURaytracer(objs, lights, RY.posed_rays(sw, sh, sz, M, origin), 2).Render()
    assert got == ppm.format_p3(W, H, ppm.rgba_to_rgb(resolve.box_filter(samples, sw, s)))
    res = subprocess.run([str(ROOT / "opencl-raytracer_amd" / "host" / "scene_tool")] + base + [str(fine), zbits, "cpu", "--pose", "1,0,0"],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 1 and "--pose takes" in res.stderr
