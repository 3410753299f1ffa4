"""GPU: RT_FLAG_DEVICE_OPENCL (HIPRaytracer(device_opencl=True)) against the reference's kernels as AMD's OpenCL toolchain
builds them for gfx950 (oracle.DeviceReference). Unlike test_device_reference_gpu there is no float64 stability filter: the
flagged backend computes the same operations, so primary t is bit-identical on every ray and colour is within 1e-5 on every
pixel. The culling checks at the end compare flagged renders with one another and need no device reference."""
import hashlib

import numpy as np
import pytest

from helpers import SCENES, camera, random_scene
from oracle import oracle
from test_device_reference_gpu import KN, _cases

pytestmark = pytest.mark.gpu
needs_device_ref = pytest.mark.skipif(not oracle.device_reference_available(),
                                      reason="oracle/_ref/*_gfx950.co or libdevice_ref.so not built")

RGB_ATOL = 1e-5
MAXF = np.float32(3.402823466e+38)
VARIANTS = (("monolithic", False), ("wavefront", False), ("monolithic", True))


def render(kernel, objs, lights, rays, mb, path="auto", literal=False, **kw):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    with HIPRaytracer(objs, lights, rays, mb, kernel=kernel, path=path, literal=literal, device_opencl=True, **kw) as rt:
        out = rt.Render()
        if kernel == "hittest":
            return out
        t, _ = rt.render_aux()
        return out, t


def same_t(a, b):
    """bit-identical, except for the sign of a zero"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


def check_colour(name, dev, got):
    d = np.abs(dev[:, :3].astype(np.float64) - got[:, :3]).max(1)
    assert d.max(initial=0) <= RGB_ATOL, (name, float(d.max()), int(np.argmax(d)))
    return int(np.all(dev[:, :3].view(np.uint32) == got[:, :3].view(np.uint32), axis=1).sum()), float(d.max(initial=0))


CASES = list(_cases((0, 1, 2)))


@needs_device_ref
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixtures_and_seeded_scenes(case, capsys):
    name, k, objs, lights, rays, mb = case
    dev_t = oracle.DeviceReference("hittest").render(objs, lights, rays)["out"]
    dev = oracle.DeviceReference(k).render(objs, lights, rays, mb)["out"] if k else None
    rows = []
    for path, literal in VARIANTS:
        if k == 0:
            t = render("hittest", objs, lights, rays, 0, path, literal)
            same = same_t(dev_t, t)
            assert same.all(), (name, path, literal, int((~same).sum()), int(np.argmin(same)))
            rows.append(f"{name:44s} {path:10s} literal={int(literal)} rays {len(t):6d} bit-identical t {int(same.sum()):6d}")
        else:
            out, t = render(KN[k], objs, lights, rays, mb, path, literal)
            assert np.array_equal(dev_t < MAXF, t < MAXF), (name, path, literal)   # the hit/miss mask
            bits, worst = check_colour(name, dev, out)
            rows.append(f"{name:44s} {path:10s} literal={int(literal)} pixels {len(out):6d} bit-identical RGB {bits:6d} "
                        f"max|dRGB| {worst:.2e}")
    with capsys.disabled():
        print("\n" + "\n".join(rows))


@needs_device_ref
def test_config3_full_frame(capsys):
    """simpleScene 4096 x 4096, shade_and_reflect depth 3: in-kernel rays and uploaded rays, and primary t of the frame."""
    from opencl_raytracer_amd import scene_loader
    objs, lights = scene_loader.load_scene(str(SCENES / "simpleScene.txt"))
    W = H = 4096
    rays = camera.primary_rays(W, H)
    dev_t = oracle.DeviceReference("hittest").render(objs, lights, rays)["out"]
    dev = oracle.DeviceReference("shade_and_reflect").render(objs, lights, rays, 3)["out"]
    t = render("hittest", objs, lights, rays, 0)
    assert same_t(dev_t, t).all(), int((~same_t(dev_t, t)).sum())
    rows = []
    for what, r, cam in (("in-kernel rays", None, (W, H, float(camera.camera_z(H)))), ("uploaded rays", rays, None)):
        out, _ = render("shade_and_reflect", objs, lights, r, 3, camera=cam)
        bits, worst = check_colour("config3 " + what, dev, out)
        rows.append(f"config3 {what:15s} pixels {len(out)} bit-identical RGB {bits} max|dRGB| {worst:.2e}")
    with capsys.disabled():
        print(f"\nconfig3 hittest rays {len(t)} bit-identical t {int(same_t(dev_t, t).sum())} (hits {int((dev_t < MAXF).sum())})")
        print("\n".join(rows))


def _config4():
    from opencl_raytracer_amd import synthetic
    return synthetic.spheres_and_lights(100_000, 32)


@needs_device_ref
def test_config4_pixels(capsys):
    """synthetic 100k spheres + 32 lights, 4096 x 4096 depth 3: the 4 608 scattered pixels of test_parity_wide_gpu and
    four full rows, from the flagged headline path (whole frame, in-kernel rays, grid)."""
    from test_parity_wide_gpu import rays_of_pixels, scattered_pixels
    objs, lights = _config4()
    W = H = 4096
    px, py = scattered_pixels(W, H, 64, 512, seed=4)
    rows_y = np.array([0, 1365, 2048, 4095])
    px = np.concatenate([px, np.tile(np.arange(W), len(rows_y))])
    py = np.concatenate([py, np.repeat(rows_y, W)])
    rays = rays_of_pixels(W, H, px, py)
    dev_t = oracle.DeviceReference("hittest").render(objs, lights, rays)["out"]
    dev = oracle.DeviceReference("shade_and_reflect").render(objs, lights, rays, 3)["out"]
    frame, t = render("shade_and_reflect", objs, lights, None, 3, camera=(W, H, float(camera.camera_z(H))))
    got, got_t = frame.reshape(H, W, 4)[py, px], t.reshape(H, W)[py, px]
    same = same_t(dev_t, got_t)
    assert same.all(), int((~same).sum())
    bits, worst = check_colour("config4", dev, got)
    with capsys.disabled():
        print(f"\nconfig4 pixels {len(px)} bit-identical t {int(same.sum())} bit-identical RGB {bits} max|dRGB| {worst:.2e}")
    assert int((dev_t < MAXF).sum()) > 4000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_culling_exact_config4_crop():
    """a 512^2 window of config 4: the grid path against brute force (grid=False) and against the literal loops"""
    objs, lights = _config4()
    rays = camera.crop_rays(4096, 4096, 1792, 1792, 512, 512)
    grid, _ = render("shade_and_reflect", objs, lights, rays, 3, path="wavefront")
    brute, _ = render("shade_and_reflect", objs, lights, rays, 3, path="wavefront", grid=False)
    assert np.array_equal(_bits(grid), _bits(brute))
    lit, _ = render("shade_and_reflect", objs, lights, rays, 3, path="wavefront", literal=True)
    assert np.array_equal(_bits(grid), _bits(lit))


def test_culling_exact_random_scenes():
    """~200 seeded scenes with spheres, boxes and directional lights: monolithic against wavefront, bit for bit"""
    rays = camera.primary_rays(48, 32)
    n_diff = []
    for seed in range(200):
        rng = np.random.default_rng(seed)
        objs, lights = random_scene(int(rng.integers(1, 24)), int(rng.integers(0, 12)), int(rng.integers(1, 5)), seed=1000 + seed,
                                    directional_lights=int(rng.integers(0, 2)))
        kernel = KN[seed % 3]
        mono = render(kernel, objs, lights, rays, 3, path="monolithic")
        wave = render(kernel, objs, lights, rays, 3, path="wavefront")
        if kernel != "hittest":
            mono, wave = mono[0], wave[0]
        if not np.array_equal(_bits(mono), _bits(wave)):
            n_diff.append(seed)
    assert not n_diff, n_diff


def test_multi_device_matches_single():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer, MultiHIPRaytracer
    objs, lights = random_scene(40, 10, 3, seed=77, directional_lights=1)
    W, H = 256, 192
    z = float(camera.camera_z(H))
    with HIPRaytracer(objs, lights, None, 3, camera=(W, H, z), device_opencl=True) as rt:
        one = rt.Render()
    with MultiHIPRaytracer(objs, lights, None, 3, devices=(0, 0), camera=(W, H, z), device_opencl=True) as m:
        two = m.Render()
    assert np.array_equal(_bits(one), _bits(np.asarray(two).reshape(one.shape)))


@needs_device_ref
def test_known_answer_simple_sphere():
    """config 1 (simpleSphere 256 x 256, shade_and_reflect depth 3): the flagged P3 is byte-identical to the device build's"""
    from opencl_raytracer_amd import ppm, scene_loader
    objs, lights = scene_loader.load_scene(str(SCENES / "simpleSphere.txt"))
    rays = camera.primary_rays(256, 256)
    dev = oracle.DeviceReference("shade_and_reflect").render(objs, lights, rays, 3)["out"]
    out, _ = render("shade_and_reflect", objs, lights, rays, 3)
    want = ppm.format_p3(256, 256, ppm.rgba_to_rgb(dev))
    got = ppm.format_p3(256, 256, ppm.rgba_to_rgb(out))
    assert int((out[:, :3].sum(1) != 0).sum()) == 1565
    print(f"device_opencl simpleSphere 256x256 P3 md5 {hashlib.md5(got).hexdigest()}")
    assert got == want
