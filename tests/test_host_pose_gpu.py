"""GPU: posed cameras through the C++ flavour of the boundary - HIPRaytracer::SetPose in host/host_pose_test.cpp, on the one-GPU
and the several-GPU object - against the Python flavour: the same scene file, the same pose, the same frame bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import SCENES
from opencl_raytracer_amd import rays as RY, scene_loader
from test_set_rays_cpu import POSES

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "opencl-raytracer_amd" / "host" / "hip_raytracer_host_pose_test"


def test_cpp_set_pose_renders_the_python_frame(tmp_path):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    if not BIN.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H, depth = 96, 64, 3
    z = np.float32(-80.0)
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    M, origin, _ = POSES["pan"]
    pose_file, dump = tmp_path / "pose.bin", tmp_path / "frame.bin"
    np.concatenate([M.astype(np.float32).reshape(9), np.asarray(origin, np.float32)]).tofile(pose_file)
    res = subprocess.run([str(BIN), str(scene_file), str(W), str(H), str(depth), f"{int(z.view(np.uint32)):08x}", str(pose_file), str(dump)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    assert lines["pinhole_after"] == "0 0 0"            # SetPose's rays are rendered from the buffer
    assert lines["source"] == "3" and lines["frames_differ"] == "1" and lines["wrong_size_refused"] == "1"
    assert lines["two_shards_same"] == "1"              # the several-GPU object, two shards on one device
    frame = np.fromfile(dump, dtype=np.float32).reshape(-1, 4)
    objs, lights = scene_loader.load_scene(str(scene_file))
    with HIPRaytracer(objs, lights, RY.posed_rays(W, H, z, M, origin), depth, raygen=False) as rt:
        want = rt.Render()
    assert (want[:, :3] != 0).any(axis=1).mean() > 0.05, "the panned view misses the scene"
    assert np.array_equal(frame.view(np.uint32), want.view(np.uint32))
