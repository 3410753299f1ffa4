"""GPU: ambient-occlusion frames through the C++ flavour of the boundary - HIPRaytracer::RenderAO / AOInfo in host/host_ao_test.cpp, on
the one-GPU object and per shard of the several-GPU object - against CPURaytracer::RenderAO in the same program on a shipped scene,
with an object hidden, and against the Python flavour with the same table of directions."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_ao_test"


def test_cpp_ao_equals_the_cpu_backends():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth, K = 96, 64, 3, 8
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth), str(K)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    for tag in ("", "changed_"):
        for check in ("same_as_cpu", "info"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
    assert W * H > int(lines["shaded"]) > 300                                               # counts with signal
    # the hidden object is gone from the pass (in this scene it is the one whose own surface occludes its samples: a scaled sphere)
    assert int(lines["changed_shaded"]) < int(lines["shaded"]) and int(lines["sum"]) < int(lines["changed_sum"])
    assert lines["two_shards_same"] == "1" and lines["frame_untouched"] == "1"
    # the Python flavour on the same scene, rays and table: direction j is ((37 j) % 17 - 8, (53 j) % 19 - 9, (29 j) % 13 + 1) / 8
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    j = np.arange(16 * K)
    dirs = np.stack([((37 * j) % 17 - 8) * 0.125, ((53 * j) % 19 - 9) * 0.125, ((29 * j) % 13 + 1) * 0.125, 0 * j], axis=1).astype(np.float32)
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        got = rt.render_ao(dirs, K, 1e-3, want=("unoccluded",))["unoccluded"]
    assert int(got.sum()) == int(lines["sum"]) and int((got < K).sum()) == int(lines["shaded"])
