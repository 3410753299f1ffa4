"""GPU: ray queries through the C++ flavour of the boundary - HIPRaytracer::QueryClosest / QueryOccluded / Pick in
host/host_query_test.cpp, on the one-GPU and the several-GPU object - against CPURaytracer::QueryClosest / QueryOccluded in the same
program, on a shipped scene, and against the Python flavour."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_query_test"


def test_cpp_queries_equal_the_cpu_backends():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth = 96, 64, 3
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    for tag in ("", "hidden_"):
        for check in ("frame_rays_t", "frame_rays_index", "pick", "other_rays_t", "other_rays_index", "occluded", "info_routes"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
        assert lines[tag + "info_rays"] == "38"                       # the last query: the 38 rays of another kind
        assert 0 < int(lines[tag + "occluded_count"]) < 38
    assert int(lines["frame_rays_hits"]) > int(lines["hidden_frame_rays_hits"]) > 0.02 * W * H   # the hidden object is gone from the answers
    assert lines["frame_untouched"] == "1" and lines["pick_refused"] == "1" and lines["two_shards_same"] == "1"
    # the Python flavour on the same scene and rays
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        _, index = rt.query_closest(rays)
    assert int((index >= 0).sum()) == int(lines["frame_rays_hits"])
