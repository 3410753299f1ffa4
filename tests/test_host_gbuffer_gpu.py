"""GPU: G-buffer frames through the C++ flavour of the boundary - HIPRaytracer::RenderGBuffer / GBufferInfo in
host/host_gbuffer_test.cpp, on the one-GPU object and per shard of the several-GPU object - against CPURaytracer::RenderGBuffer in the
same program on a shipped scene, with an object hidden and one recoloured, and against the Python flavour."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_gbuffer_test"


def test_cpp_gbuffer_equals_the_cpu_backends():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth = 96, 64, 3
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    for tag in ("", "changed_"):
        for check in ("same_as_cpu", "misses_zero", "info", "same_as_pick_hits"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
    assert W * H > int(lines["hits"]) > int(lines["changed_hits"]) > 0.02 * W * H     # the hidden object is gone from the records
    assert int(lines["painted"]) == 0 and int(lines["changed_painted"]) > 0           # object 0 shows its new colour
    assert lines["two_shards_same"] == "1" and lines["frame_untouched"] == "1"
    # the Python flavour on the same scene and rays
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        g = rt.render_gbuffer(want=("index",))
    assert int((g["index"] >= 0).sum()) == int(lines["hits"])
