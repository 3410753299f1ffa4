"""GPU: shaded queries through the C++ flavour of the boundary - HIPRaytracer::QueryShade / PickColours / PickColour in
host/host_shade_test.cpp - on a shipped scene: the answer for the frame's own rays is the frame, bit for bit; t and index are the
CPU backend's (CPURaytracer::QueryShade in the same program) and the colours agree within 1e-5, before and after SetVisibility and
SetMaterials; rays of the caller's own with a mask; and the Python flavour on the same scene."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_shade_test"


def test_cpp_shaded_queries():
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
        for check in ("is_the_frame", "primary", "info"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
        assert float(lines[tag + "colour_error"]) <= 1e-5, res.stdout
        assert W * H > int(lines[tag + "hits"]) > 0.02 * W * H
    assert lines["changed_frame_differs"] == "1" and int(lines["changed_hits"]) < int(lines["hits"])   # the hidden object is gone
    assert lines["own_primary"] == "1" and float(lines["own_colour_error"]) <= 1e-5 and int(lines["own_hits"]) > 0.01 * W * H
    for check in ("masked", "pick_colours", "pick_colour", "frame_after_picks", "pick_refused", "mask_refused", "hittest_refused"):
        assert lines[check] == "1", (check, res.stdout)
    # the Python flavour on the same scene and rays
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = np.float32(-H)   # the program's grid: z = -height
    with HIPRaytracer(objs, lts, rays, depth) as rt:
        frame = rt.Render().copy()
        got = rt.query_shade(rays, want=("rgba", "index"))
    assert np.array_equal(got["rgba"].view(np.uint32), frame.view(np.uint32))
    assert int((got["index"] >= 0).sum()) == int(lines["hits"])
