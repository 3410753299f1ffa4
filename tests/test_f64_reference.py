"""CPU: the float64 restatement (oracle/f64.py) against the x86 restatement (oracle/rt_oracle.c, fused), and its stability
classifier.

Inputs: every golden fixture's inputs, the seeded scenes of test_oracle_vs_ref.py (101-103) and a tessellated roundedCube
(the triangle extension, which otherwise has only self-parity).

Bars, on STABLE pixels (f64 margin >= f64.TAU) - both measured here, against the fused x86 restatement:
  * T_T = 1e-5 relative on primary t. Measured worst 8.5e-6 (hittest_spheres / random_mixed100): a primary t near a
    silhouette is the quotient of a radical that has cancelled down to ~1e-4 of its terms, so fp32's 6e-8 grows to
    ~eps / sqrt(margin) there.
  * T_RGB = 2e-4 absolute on RGB. Measured worst 1.65e-4 (random_mixed100_shade_and_reflect): powf(rDotV, shininess) with
    shininess 100 multiplies rDotV's relative fp32 error by 100, and a reflection chain adds up to four such terms.
(Both live in helpers.py, F64_T_T / F64_T_RGB, shared with tests/test_device_reference_gpu.py.)
NOT covered: scenes of the benchmark's generator (synthetic_1k; helpers.F64_NO_HIT_MINIMUM says why none of their hits
is stable). The classifier is checked against the fp32 arithmetic itself: every pixel whose primary hit/miss or hit index
changes when its ray is nudged by one ulp must be unstable."""
import numpy as np
import pytest

from helpers import (F64_T_RGB, F64_T_T, R, SCENES, f64_degenerate, f64_needs_hits, fixture_names, load_fixture,
                     ref_run_scene)
from oracle import f64

T_T, T_RGB = F64_T_T, F64_T_RGB
KN = {0: "hittest", 1: "shade", 2: "shade_and_reflect"}

# the share of pixels excluded over all ordinary inputs (synthetic_1k included): measured 3.59 %.
# History of the margin's error model: the t-sign tests (a secondary ray meeting the surface it leaves, an origin on a
# box face) first measured |t| against the start's error taken as 4 eps |S| / |D| in view space; 1.71 % excluded then
# (synthetic_1k not counted). The first comparison with the gfx950-built reference found a stable pixel it shadowed by
# its own sphere (random_mixed100_shade, pixel 910: t = -7.7e-5, 22 such errors), so the error is now carried through
# each instance's mvInverse (f64._object_sd); that added 1.67 points (to 3.38 %, synthetic_1k not counted).
EXCLUSION_CAP = 0.04


_degenerate = f64_degenerate


def _triangle_scene():
    from opencl_raytracer_amd import camera, scene_loader, tessellate as T
    objs, lights = scene_loader.load_scene(str(SCENES / "roundedCube.txt"))
    return T.tessellate(objs, 6, 12, 2), lights, camera.primary_rays(48, 48)


def _inputs():
    for name in fixture_names():
        fx = load_fixture(name)
        yield name, fx["kernel"], fx["objs"], fx["lights"], fx["rays"], fx["max_bounces"]
    for seed in (101, 102, 103):
        objs, lights, rays = ref_run_scene(seed)
        for k in (0, 2):
            yield f"seed{seed}_{KN[k]}", k, objs, lights, rays, 3
    tri, lights, rays = _triangle_scene()
    for k in (0, 2):
        yield f"triangles_roundedCube_{KN[k]}", k, tri, lights, rays, 3


INPUTS = list(_inputs())
IDS = [i[0] for i in INPUTS]


@pytest.fixture(scope="module")
def f64_runs():
    return {}


def _run(cache, inp):
    name, k, objs, lights, rays, mb = inp
    if name not in cache:
        cache[name] = f64.render(k, objs, lights, rays, mb)
    return cache[name]


@pytest.mark.parametrize("inp", INPUTS, ids=IDS)
def test_f64_matches_the_fp32_restatement_on_stable_pixels(inp, restatement, f64_runs):
    name, k, objs, lights, rays, mb = inp
    ref = _run(f64_runs, inp)
    x86 = restatement[True].render(k, objs, lights, rays, mb)
    st = ref["stable"]
    assert np.array_equal(ref["hit_index"][st], x86["hit_index"][st]), name
    hit = st & (x86["hit_index"] >= 0)
    if hit.any():
        rel = np.abs(ref["hit_t"][hit] - x86["hit_t"][hit]) / ref["hit_t"][hit]
        assert rel.max() <= T_T, (name, float(rel.max()))
    if k:
        d = np.abs(ref["out"][st] - x86["out"][st, :3].astype(np.float64))
        assert d.size == 0 or d.max() <= T_RGB, (name, float(d.max()))
    else:
        assert np.array_equal(ref["out"][st] == f64.MAX_FLOAT, x86["out"][st] == np.float32(f64.MAX_FLOAT))
    if f64_needs_hits(name):
        assert hit.sum() >= 5, (name, int(hit.sum()))    # not a vacuous comparison (a lone sphere keeps 9 of 97)


def _nudge(rays, direction):
    """Every float of every ray moved by one ulp (towards +inf or -inf)."""
    f = rays.view(np.float32).reshape(len(rays), 8).copy()
    moved = np.nextafter(f, np.float32(np.inf) if direction > 0 else np.float32(-np.inf))
    keep = np.zeros_like(f, bool)
    keep[:, 3] = keep[:, 7] = True    # w components (1 and 0) keep their meaning
    out = np.where(keep, f, moved).astype(np.float32)
    return out.view(R.RAY_DTYPE).reshape(len(rays))


@pytest.mark.parametrize("inp", [i for i in INPUTS if not _degenerate(i[0])], ids=[i[0] for i in INPUTS if not _degenerate(i[0])])
def test_classifier_covers_one_ulp_flips(inp, restatement, f64_runs):
    name, k, objs, lights, rays, mb = inp
    ref = _run(f64_runs, inp)
    base = restatement[True].render(0, objs, lights, rays, 0)["hit_index"]
    for direction in (+1, -1):
        moved = restatement[True].render(0, objs, lights, _nudge(rays, direction), 0)["hit_index"]
        flipped = moved != base
        assert not (flipped & ref["stable"]).any(), (name, direction, np.nonzero(flipped & ref["stable"])[0][:10])


def test_exclusion_cap(f64_runs, capsys):
    excl = total = 0
    lines = []
    for inp in INPUTS:
        ref = _run(f64_runs, inp)
        e, n = int((~ref["stable"]).sum()), len(ref["stable"])
        lines.append(f"{inp[0]:48s} excluded {e:6d} / {n:6d} ({e / n:6.2%}){'  [degenerate]' if _degenerate(inp[0]) else ''}")
        if not _degenerate(inp[0]):
            excl += e
            total += n
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print(f"ordinary inputs: {excl} of {total} pixels excluded ({excl / total:.2%}); cap {EXCLUSION_CAP:.0%}")
    assert excl <= EXCLUSION_CAP * total
