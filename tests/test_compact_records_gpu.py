"""GPU: the compact records of scale-and-translate scenes (hip_raytracer.h, "compact records"). While every sphere and box of a scene
is a scale-and-translate instance the round machine's kernels read 64-byte records with the diagonals and translations instead of the
full rows, and run the same arithmetic on rows rebuilt with literal zeros: the frame, the primary t and the primary index are the
ones the full records give (RT_COMPACT_RECORDS=0), bit for bit.

1. compact on against off, under the three arithmetic flags, with and without the grid;
2. rt_set_transforms rotates one object (compact off: the info call says so) and puts it back (on again): each state is a fresh context's;
3. rt_set_materials changes an absorption, rt_set_visibility hides an object that was hit: each is a fresh context's, and the read-back
   checkers, which compare the compact copy too, pass;
4. the two scenes of test_zero_box_normal (NaN reflection rays), rebuilt without their rotations.
The scene: 200 spheres and axis-aligned, non-uniformly scaled boxes around (0, 0, -40), 64 x 64 pixels, depth 3, two lights - the round
machine, the grid and the light tiles, asserted through the info calls."""
import contextlib
import functools
import os

import numpy as np
import pytest

from helpers import R, instance, rotation
from test_primary_depth_order_gpu import MODES, bits, hip
from test_set_lights_cpu import CENTRE, POSITIONS, SPREAD, make_lights

pytestmark = pytest.mark.gpu
W, H, Z = 64, 64, -160.0
DEPTH = 3
N = 200


@contextlib.contextmanager
def compact_records(value):
    """RT_COMPACT_RECORDS for the contexts created inside (rt_create reads it); None: unset."""
    before = os.environ.pop("RT_COMPACT_RECORDS", None)
    if value is not None:
        os.environ["RT_COMPACT_RECORDS"] = value
    try:
        yield
    finally:
        os.environ.pop("RT_COMPACT_RECORDS", None)
        if before is not None:
            os.environ["RT_COMPACT_RECORDS"] = before


@functools.lru_cache(maxsize=None)
def diagonal_cloud():
    """130 spheres and 70 boxes, no rotation, axis scales 0.4 .. 1.6 drawn per axis, shuffled so that the types interleave."""
    rng = np.random.default_rng(61)
    types = [R.SPHERE] * 130 + [R.BOX] * 70
    rng.shuffle(types)
    objs = []
    for t in types:
        pos = (rng.uniform(-SPREAD, SPREAD), rng.uniform(-SPREAD, SPREAD), rng.uniform(CENTRE[2] - SPREAD, CENTRE[2] + SPREAD))
        a = float(rng.choice([1.0, 0.9995, 0.7, 0.5, 0.2]))
        mat = R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3), absorption=a,
                         reflection=1 - a, shininess=float(rng.choice([1.0, 5.0, 30.0])))
        objs.append(R.make_object(t, mat, *instance(pos, None, rng.uniform(0.4, 1.6, size=3))))
    objs = R.objects_array(objs)
    assert len(objs) == N and is_diagonal(objs)
    return objs


def is_diagonal(objs):
    """The predicate on an object array: +0.0f bits in the off-diagonal places of both upper 3x3, bottom rows (0,0,0,1)."""
    off, bottom = [1, 2, 4, 6, 8, 9], [3, 7, 11]
    for name in ("mv", "mvInverse"):
        m = np.ascontiguousarray(objs[name], dtype=np.float32).reshape(len(objs), 16)
        if m[:, off].view(np.uint32).any() or (m[:, bottom] != 0).any() or (m[:, 15] != 1).any():
            return False
    return True


def without_rotations(objs):
    """The same objects as scale-and-translate instances: mv's translation and the lengths of its three axes."""
    out = objs.copy()
    for k in range(len(objs)):
        mv = objs["mv"][k].reshape(4, 4).astype(np.float64)   # column-major: mv[c][r]
        scale = np.linalg.norm(mv[:3, :3], axis=1)
        m, inv = instance(mv[3, :3], None, scale)
        out["mv"][k] = m.reshape(16)
        out["mvInverse"][k] = inv.reshape(16)
        out["mvInverseTranspose"][k] = np.ascontiguousarray(inv.reshape(4, 4).T).reshape(16)
    assert is_diagonal(out)
    return out


def lights():
    """Two lights 30 units outside the cloud: the first one's shadow rays walk the grid, the last one's read its light tiles; under
    RT_FLAG_DEVICE_OPENCL neither is in an object's reach (no literal frame)."""
    return make_lights(POSITIONS["+x"], POSITIONS["+y"])


def snapshot(rt):
    frame = rt.Render()
    t, idx = rt.render_aux()
    st = rt.count_rays()
    return dict(frame=frame, t=t, idx=idx, rays_ref=int(st.rays_reference), hits=int(st.hit_pixels), wavefront=int(st.wavefront))


def assert_same(got, want, label):
    for key in ("frame", "t", "idx"):
        a, b = bits(got[key]).reshape(-1), bits(want[key]).reshape(-1)
        assert a.shape == b.shape and np.array_equal(a, b), f"{label}: {key} differs on {int((a != b).sum())} words"
    assert got["rays_ref"] == want["rays_ref"] and got["hits"] == want["hits"], label


def live(objs, **kw):
    kw.setdefault("camera", (W, H, Z))
    return hip(objs, lights(), None, DEPTH, **kw)


_FULL = {}


def full_records(key, objs, **kw):
    """Snapshot of a fresh context that reads the full records (RT_COMPACT_RECORDS=0); remembered per key."""
    if key not in _FULL:
        with compact_records("0"), live(objs, **kw) as rt:
            assert rt.compact_info()["in_use"] == 0 and rt.compact_info()["allowed"] == 0
            _FULL[key] = snapshot(rt)
    return _FULL[key]


# ---- 1. compact on against off -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "no_grid"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_compact_equals_full(mode, grid):
    objs = diagonal_cloud()
    # (200 objects without a grid are the small-scene path's by default: the round machine is asked for)
    want = full_records(("cloud", mode, grid), objs, grid=grid, path="wavefront", **MODES[mode])
    assert want["wavefront"] == 1 and want["hits"] > W * H // 8
    for value in (None, "1"):
        with compact_records(value), live(objs, grid=grid, path="wavefront", **MODES[mode]) as rt:
            info = rt.compact_info()
            assert info == dict(table_built=1, n_not_diagonal=0, allowed=1, in_use=1), info
            assert rt.rays_info()["literal"] == 0
            if grid:   # the round machine with its grid and the last light's tiles
                assert rt.rays_info()["grid_built"] == 1 and rt.rays_info()["grid_in_use"] == 1 and rt.light_tiles_info()["enabled"] == 1
            else:
                assert rt.rays_info()["grid_in_use"] == 0
            got = snapshot(rt)
        assert got["wavefront"] == 1
        assert_same(got, want, f"{mode}, grid {grid}, RT_COMPACT_RECORDS {value}")


# ---- 2. the predicate follows rt_set_transforms --------------------------------------------------------------------------------
def test_rotating_one_object_switches_the_records():
    objs = diagonal_cloud()
    with live(objs) as rt:
        before = snapshot(rt)
        _, idx = rt.render_aux()
        k = int(np.bincount(idx[idx >= 0]).argmax())   # the object that covers most pixels
        mv = objs["mv"][k].reshape(4, 4).astype(np.float64)
        turned = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
        m, inv = instance(mv[3, :3], rotation((0.3, 1.0, 0.2), 0.6), np.linalg.norm(mv[:3, :3], axis=1))
        turned["mv"][0], turned["mvInverse"][0] = m.reshape(16), inv.reshape(16)
        rt.set_transforms(turned, k)
        info = rt.compact_info()
        assert (info["n_not_diagonal"], info["in_use"], info["allowed"]) == (1, 0, 1), info
        rotated = snapshot(rt)
        assert not np.array_equal(bits(rotated["frame"]), bits(before["frame"]))
        with live(R.with_transforms(objs, turned, k)) as ref:
            assert ref.compact_info()["in_use"] == 0 and ref.compact_info()["n_not_diagonal"] == 1
            assert_same(rotated, snapshot(ref), "one object rotated")
        rt.read_transforms()                                      # every copy agrees, the compact one included
        rt.set_transforms(R.transforms_of(objs)[k:k + 1], k)      # ... and back
        info = rt.compact_info()
        assert (info["n_not_diagonal"], info["in_use"]) == (0, 1), info
        back = snapshot(rt)
        assert rt.geometry_info()["n_dynamic"] == 1               # (it stays a dynamic object, on the always-list)
        rt.read_transforms()
    assert_same(back, before, "put back")
    assert_same(back, full_records(("cloud", "fused", True), objs, grid=True, path="wavefront"), "put back, against the full records")


def test_a_scene_that_becomes_diagonal():
    """Created with one rotated object (no frame reads the compact records), made diagonal by rt_set_transforms: they serve the next frame."""
    objs = diagonal_cloud()
    k = 17
    mv = objs["mv"][k].reshape(4, 4).astype(np.float64)
    m, inv = instance(mv[3, :3], rotation((1.0, 0.2, -0.4), 1.1), np.linalg.norm(mv[:3, :3], axis=1))
    start = objs.copy()
    start["mv"][k], start["mvInverse"][k] = m.reshape(16), inv.reshape(16)
    with live(start) as rt:
        assert rt.compact_info() == dict(table_built=1, n_not_diagonal=1, allowed=1, in_use=0)
        rt.Render()
        rt.set_transforms(R.transforms_of(objs)[k:k + 1], k)
        assert rt.compact_info()["in_use"] == 1
        got = snapshot(rt)
    with live(objs) as ref:
        assert_same(got, snapshot(ref), "made diagonal")


# ---- 2b. the predicate of rt_create, on real contexts --------------------------------------------------------------------------
def changed(objs, k, name, place, value):
    out = objs.copy()
    m = out[name][k].copy()
    m.view(np.uint32)[place] = np.array([value], dtype=np.float32).view(np.uint32)[0]
    out[name][k] = m
    return out


@pytest.mark.parametrize("case", ["diagonal", "neg_zero mv", "neg_zero mvInverse", "nan", "bottom row", "triangle", "never hit"])
def test_the_predicate_on_a_context(case):
    """What rt_create says of a scene (rt_get_compact_info) - the table, the count, the next frame's switch - and, where the change
    leaves a scene the round machine renders, that the frame is the one the full records give."""
    objs = diagonal_cloud()
    k = 23
    expect = dict(table_built=1, n_not_diagonal=1, allowed=1, in_use=0)
    if case == "diagonal":
        expect = dict(table_built=1, n_not_diagonal=0, allowed=1, in_use=1)
    elif case.startswith("neg_zero"):          # -0.0f in an off-diagonal place: the same matrix to every comparison, not to the predicate
        objs = changed(objs, k, case.split()[1], 4, -0.0)
    elif case == "nan":
        objs = changed(objs, k, "mv", 9, np.nan)    # (mv only: the bounds come from mvInverse, the scene stays on the default path)
    elif case == "bottom row":                 # diagonal, but not affine: affine_w decides
        objs = changed(objs, k, "mv", 7, 0.25)
        expect = dict(table_built=1, n_not_diagonal=0, allowed=1, in_use=0)
    elif case == "triangle":                   # no table at all
        objs = objs.copy()
        objs["type"][k] = 2
        expect = dict(table_built=0, n_not_diagonal=0, allowed=0, in_use=0)
    elif case == "never hit":                  # a type no kernel reads the rows of: a rotated one does not count
        objs = objs.copy()
        objs["type"][k] = 7
        m, inv = instance((0.0, 0.0, -40.0), rotation((1.0, 0.3, 0.2), 0.8), (1.0, 0.7, 1.2))
        objs["mv"][k], objs["mvInverse"][k] = m.reshape(16), inv.reshape(16)
        expect = dict(table_built=1, n_not_diagonal=0, allowed=1, in_use=1)
    with live(objs, path="wavefront") as rt:
        assert rt.compact_info() == expect, (case, rt.compact_info())
        got = snapshot(rt)
        assert rt.compact_info() == expect
    assert got["wavefront"] == 1
    assert_same(got, full_records(("predicate", case), objs, path="wavefront"), case)


# ---- 3. materials and visibility keep the compact copy true --------------------------------------------------------------------
def test_materials_and_visibility():
    objs = diagonal_cloud()
    with live(objs) as rt:
        before = snapshot(rt)
        _, idx = rt.render_aux()
        seen = np.bincount(idx[idx >= 0], minlength=N)
        a, b = (int(v) for v in np.argsort(seen)[-2:])           # two objects that are hit
        mats = R.materials_of(objs)[a:a + 1].copy()
        mats["absorption"][0] = 0.35
        rt.set_materials(mats, a)
        assert rt.compact_info()["in_use"] == 1
        recoloured = snapshot(rt)
        assert not np.array_equal(bits(recoloured["frame"]), bits(before["frame"]))
        rt.read_materials()                                       # ColdObject = ObjectRecord = CompactObject
        with_mat = R.with_materials(objs, mats, a)
        with live(with_mat) as ref:
            assert_same(recoloured, snapshot(ref), "absorption changed")
        mask = np.ones(1, dtype=np.uint8) * 0
        rt.set_visibility(mask, b)
        hidden = snapshot(rt)
        assert not np.isin(b, hidden["idx"]) and np.isin(b, before["idx"])
        vis = rt.read_visibility()                                # every copy of the type word, the compact one included
        assert vis[b] == 0 and vis.sum() == N - 1
        full_mask = np.ones(N, dtype=np.uint8)
        full_mask[b] = 0
        with live(R.with_visibility(with_mat, full_mask)) as ref:
            assert ref.compact_info()["in_use"] == 1   # (a hidden object is no sphere or box: it does not count)
            assert_same(hidden, snapshot(ref), "one object hidden")
        assert_same(hidden, full_records(("hidden", a, b), R.with_visibility(with_mat, full_mask)), "hidden, against the full records")


# ---- 4. NaN reflection rays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fuzz seed 45", "tiny far box"])
def test_nan_reflection_rays(name):
    import test_device_opencl_fuzz_gpu as Z45
    if name == "fuzz seed 45":
        objs, lts, rays = Z45.fuzz_scene(np.random.default_rng(1000 + 45))
    else:
        objs, lts, rays = Z45.tiny_far_box_scene()
    objs = without_rotations(objs)
    runs = {}
    for value in ("0", None):
        with compact_records(value), hip(objs, lts, rays, DEPTH, path="wavefront") as rt:
            assert rt.compact_info()["in_use"] == (0 if value == "0" else 1)
            runs[value] = snapshot(rt)
    assert_same(runs[None], runs["0"], name)
    if name == "tiny far box":   # the construction survives the rebuild: zero box normals make NaN reflection rays (the probe of test_zero_box_normal)
        assert Z45.nan_route_pixels(objs, lts, rays, DEPTH, device_opencl=False) > 0
