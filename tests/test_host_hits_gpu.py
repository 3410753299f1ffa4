"""GPU: hit-record queries through the C++ flavour of the boundary - HIPRaytracer::QueryHits / PickHits / PickHit in
host/host_hits_test.cpp, on the one-GPU and the several-GPU object - against CPURaytracer::QueryHits in the same program along a
three-bounce reflection chain on a shipped scene, and against the Python flavour."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_hits_test"


def test_cpp_hit_records_equal_the_cpu_backends():
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
        for check in ("bounce1", "bounce2", "bounce3", "misses_zero", "bounce2_traced", "bounce3_traced", "pick_hits", "pick_hit"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
        assert W * H > int(lines[tag + "bounce1_hits"]) > int(lines[tag + "bounce2_hits"]) > 0   # the chain goes on, and thins out
    assert int(lines["bounce1_hits"]) > int(lines["hidden_bounce1_hits"]) > 0.02 * W * H          # the hidden object is gone from the answers
    assert int(lines["pick_hit_index"]) >= 0                                                      # the centre pixel meets an object
    assert lines["frame_untouched"] == "1" and lines["pick_refused"] == "1" and lines["mask_refused"] == "1" and lines["two_shards_same"] == "1"
    # the Python flavour on the same scene and rays
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        first = rt.query_hits(rays)
        second = rt.query_hits(first["reflected"], first["index"], want=("index",))
    assert int((first["index"] >= 0).sum()) == int(lines["bounce1_hits"])
    assert int((second["index"] >= 0).sum()) == int(lines["bounce2_hits"])
