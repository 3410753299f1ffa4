"""CPU: the RT_FLAG_DEVICE_OPENCL interface - the header defines the bit, rt_create accepts it alone (on a machine without a
GPU it then fails with RT_ERR_NO_DEVICE, past the argument checks) and refuses it with RT_FLAG_UNFUSED / RT_FLAG_FAST_PHONG
or with triangles, from C and from Python."""
import re
from pathlib import Path

import numpy as np
import pytest

import helpers  # noqa: F401  (registers the package under its importable name)
from helpers import camera, random_scene

ROOT = Path(__file__).resolve().parents[1]
RT_ERR_INVALID_ARGUMENT, RT_ERR_NO_DEVICE = -1, -2


def gpu_present():
    import torch
    return torch.cuda.is_available() and torch.cuda.device_count() > 0


def test_header_defines_the_flag():
    text = (ROOT / "include" / "hip_raytracer.h").read_text()
    m = re.search(r"#define\s+RT_FLAG_DEVICE_OPENCL\s+(0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == 0x80
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", text)


def _create(flags, objs=None):
    import ctypes
    from opencl_raytracer_amd import hip_raytracer as hr
    lib = hr.load_library()
    if objs is None:
        objs, lights = random_scene(3, 2, 1, seed=1)
    else:
        _, lights = random_scene(3, 2, 1, seed=1)
    rays = camera.primary_rays(8, 8)
    ctx = ctypes.c_void_p()
    rc = lib.rt_create(ctypes.byref(ctx), hr._ptr(objs), len(objs), hr._ptr(lights), len(lights), hr._ptr(rays), len(rays), 3,
                       2, 0, flags)
    msg = lib.rt_last_error(None)
    msg = msg.decode() if msg else ""
    if rc == 0:
        lib.rt_destroy(ctx)
    return rc, msg


def test_flag_alone_passes_the_argument_checks():
    from opencl_raytracer_amd import hip_raytracer as hr
    rc, msg = _create(hr.FLAG_DEVICE_OPENCL)
    assert "unknown flag bits" not in msg
    if gpu_present():
        assert rc == 0, msg
    else:
        assert rc == RT_ERR_NO_DEVICE, msg


@pytest.mark.parametrize("other", ["FLAG_UNFUSED", "FLAG_FAST_PHONG"])
def test_refused_combinations(other):
    from opencl_raytracer_amd import hip_raytracer as hr
    rc, msg = _create(hr.FLAG_DEVICE_OPENCL | getattr(hr, other))
    assert rc == RT_ERR_INVALID_ARGUMENT
    assert "RT_FLAG_DEVICE_OPENCL" in msg and "RT_" + other in msg


def test_refused_for_triangles():
    from opencl_raytracer_amd import hip_raytracer as hr
    objs, _ = random_scene(3, 2, 1, seed=1)
    objs = objs.copy()
    objs["type"][1] = 2
    rc, msg = _create(hr.FLAG_DEVICE_OPENCL, objs)
    assert rc == RT_ERR_INVALID_ARGUMENT and "triangles" in msg


@pytest.mark.parametrize("kw", [{"fused": False}, {"fast_phong": True}])
def test_python_kwargs(kw):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer, MultiHIPRaytracer, RTError
    objs, lights = random_scene(3, 2, 1, seed=1)
    rays = camera.primary_rays(8, 8)
    with pytest.raises(RTError) as e:
        HIPRaytracer(objs, lights, rays, 3, device_opencl=True, **kw)
    assert e.value.code == RT_ERR_INVALID_ARGUMENT and "RT_FLAG_DEVICE_OPENCL" in str(e.value)
    if "fused" in kw:
        with pytest.raises(RTError) as e:
            MultiHIPRaytracer(objs, lights, rays, 3, devices=(0,), device_opencl=True, **kw)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT and "RT_FLAG_DEVICE_OPENCL" in str(e.value)


def test_python_kwarg_alone():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer, RTError
    objs, lights = random_scene(3, 2, 1, seed=1)
    rays = camera.primary_rays(8, 8)
    if gpu_present():
        with HIPRaytracer(objs, lights, rays, 3, device_opencl=True) as rt:
            assert np.isfinite(rt.Render()).all()
        return
    with pytest.raises(RTError) as e:
        HIPRaytracer(objs, lights, rays, 3, device_opencl=True)
    assert e.value.code == RT_ERR_NO_DEVICE
