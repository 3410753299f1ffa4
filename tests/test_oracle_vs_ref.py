"""CPU: the restatement against the reference kernels compiled verbatim (oracle/_ref) on seeded random scenes beyond the
committed fixtures. The reference's outputs come live from oracle/_ref where it was built (the build container; they are
then also held against the stored copy), else from tests/golden/ref_runs/oracle_vs_ref.npz, which
tests/golden/make_golden.py --reference-runs wrote from those same kernels."""
import numpy as np
import pytest

from helpers import GOLDEN, camera, ref_run_scene, same_floats
from oracle import oracle

REF_RUNS = GOLDEN / "ref_runs" / "oracle_vs_ref.npz"


def reference_out(key, kernel, fused, objs, lights, rays, max_bounces):
    stored = np.load(REF_RUNS)[key]
    if not oracle.reference_available():
        return stored
    live = oracle.Reference(kernel, fused).render(objs, lights, rays, max_bounces)["out"]
    assert same_floats(live, stored), f"{key}: oracle/_ref no longer computes the stored reference output"
    return live


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("kernel", ["hittest", "shade", "shade_and_reflect"])
@pytest.mark.parametrize("seed", [101, 102, 103])
def test_random_scene_bit_exact(seed, kernel, fused, restatement):
    objs, lights, rays = ref_run_scene(seed)
    ref = reference_out(f"random_{seed}_{kernel}_{'fused' if fused else 'unfused'}", kernel, fused, objs, lights, rays, 3)
    got = restatement[fused].render(kernel, objs, lights, rays, 3)["out"]
    if kernel != "hittest":
        ref, got = ref[:, :3], got[:, :3]
    assert same_floats(ref, got)


def test_known_answer_simple_sphere_ppm(restatement):
    """Config 1 known answer: 256x256 simpleSphere written as P3 has md5 28365bd1...; the restatement
    renders the same pixels."""
    import hashlib
    from helpers import SCENES
    from opencl_raytracer_amd import ppm, scene_loader
    objs, lights = scene_loader.load_scene(str(SCENES / "simpleSphere.txt"))
    rays = camera.primary_rays(256, 256)
    for kernel in ("shade", "shade_and_reflect"):
        for fused in (True, False):
            out = reference_out(f"simpleSphere_256_{kernel}_{'fused' if fused else 'unfused'}", kernel, fused, objs, lights, rays, 3)
            assert int((out[:, :3].sum(1) != 0).sum()) == 1565
            blob = ppm.format_p3(256, 256, ppm.rgba_to_rgb(out))
            assert len(blob) == 397825
            assert hashlib.md5(blob).hexdigest() == "28365bd12a502710be0c9a9a1a8057a9"
            assert same_floats(restatement[fused].render(kernel, objs, lights, rays, 3)["out"][:, :3], out[:, :3]), (kernel, fused)
