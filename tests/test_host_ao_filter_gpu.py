"""GPU: filtered ambient occlusion through the C++ flavour of the boundary - HIPRaytracer::RenderAOFiltered / FilterAO / AOFilterInfo in
host/host_ao_filter_test.cpp - against CPURaytracer::RenderAOFiltered in the same program on a shipped scene, with an object hidden,
and against the Python flavour with the same table of directions."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import camera, scene_loader

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_ao_filter_test"


def test_cpp_filtered_ao_equals_the_cpu_backends():
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth, K, radius, normal_min, plane_max = 96, 64, 3, 8, 2, 0.875, 0.125     # (thresholds exact in float and in the program's atof)
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth), str(K), str(radius), str(normal_min), str(plane_max)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    for tag in ("", "changed_"):
        for check in ("same_as_cpu", "info", "pass_alone_same"):
            assert lines[tag + check] == "1", (tag + check, res.stdout)
    assert int(lines["blurred"]) > 300 and int(lines["taps"]) > 3 * int(lines["blurred"])   # windows with signal
    assert lines["changed_taps"] != lines["taps"]                                           # the hidden object is gone from the pass
    assert lines["two_shards_refused"] == "1" and lines["frame_untouched"] == "1"
    # the Python flavour on the same scene, rays and table: direction j is ((37 j) % 17 - 8, (53 j) % 19 - 9, (29 j) % 13 + 1) / 8
    objs, lts = scene_loader.load_scene(str(scene_file))
    j = np.arange(16 * K)
    dirs = np.stack([((37 * j) % 17 - 8) * 0.125, ((53 * j) % 19 - 9) * 0.125, ((29 * j) % 13 + 1) * 0.125, 0 * j], axis=1).astype(np.float32)
    with HIPRaytracer(objs, lts, None, depth, camera=(W, H, float(-H))) as rt:       # the program's grid: z = -height
        got = rt.render_ao_filtered(dirs, K, 1e-3, radius, normal_min, plane_max, want=("grey", "taps"))
    assert int(got["taps"].sum()) == int(lines["taps"]) and int(got["grey"].sum()) == int(lines["grey"])
    assert int((got["taps"] > 1).sum()) == int(lines["blurred"])
