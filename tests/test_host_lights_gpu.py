"""GPU: replaceable lights through the C++ flavour of the boundary - HIPRaytracer::SetLights and LightTilesInfo in
host/host_lights_test.cpp, on the one-GPU and the several-GPU object - against the Python flavour: the same scene file, the same
lights, the same frame bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import R, SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_lights_test"


def test_cpp_set_lights_renders_the_python_frame(tmp_path):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth = 96, 64, 3
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    recs = np.array([[-6.0, 9.0, 4.0, 1.0, 0.1, 0.5, 0.4], [0.2, 1.0, 0.3, 0.0, 0.0, 0.3, 0.2], [12.0, 3.0, 6.0, 1.0, 0.05, 0.6, 0.5]], dtype=np.float32)
    lights_file, dump = tmp_path / "lights.bin", tmp_path / "frame.bin"
    recs.tofile(lights_file)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth), str(lights_file), str(dump)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    assert lines["n_lights"] == "3" and lines["frames_differ"] == "1"
    assert lines["back_to_first"] == "1" and lines["history_free"] == "1"
    assert lines["two_shards_same"] == "1"              # the several-GPU object, two shards on one device
    frame = np.fromfile(dump, dtype=np.float32).reshape(-1, 4)
    objs, _ = scene_loader.load_scene(str(scene_file))
    lts = R.lights_array([R.make_light(R.LightProperties(ambient=(r[4],) * 3, diffuse=(r[5],) * 3, specular=(r[6],) * 3), position=tuple(r[:4]))
                          for r in recs])
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        want = rt.Render()
        info = rt.light_tiles_info()
    assert lines["tiles"].split()[0] == str(info["enabled"])   # the small scene has no grid: no table on either side
    assert (want[:, :3] != 0).any(axis=1).mean() > 0.05
    assert np.array_equal(frame.view(np.uint32), want.view(np.uint32))
