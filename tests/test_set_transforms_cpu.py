"""Replaceable transforms without a GPU: the names, the executable definition (records.with_transforms) and the CPU backend.

1. TRANSFORM_DTYPE is rt_transform: 128 bytes, mv then mvInverse, the two fields of OBJECT_DTYPE;
2. with_transforms / transforms_of round trip; with_transforms changes exactly the three matrices of the range (mvInverseTranspose
   becomes the transpose), from a transform array and from an object array: materials, type and padding untouched;
3. names: header, wrappers, Makefiles, EXPORTS, ABI 3, sizeof(rt_geometry_info_t);
4. CPURaytracer.set_transforms equals a fresh CPU backend created with with_transforms(...) on a golden-fixture scene, bit for bit,
   after a history of calls, and together with set_lights / set_materials / set_pose.
The moves here (new_transforms) are the GPU tests' (test_set_transforms_gpu.py)."""
import ctypes
import re

import numpy as np
import pytest

from helpers import R, ROOT, instance, load_fixture, rotation
from test_set_materials_cpu import as_words, new_materials

F = np.float32


def transform(centre, rot=None, scale=(1.0, 1.0, 1.0)):
    """One TRANSFORM_DTYPE record: mv = T * R * S and its inverse, as helpers.instance rounds them."""
    mv, inv = instance(centre, rot, scale)
    t = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
    t["mv"][0] = mv.reshape(16)
    t["mvInverse"][0] = inv.reshape(16)
    return t


def new_transforms(n, seed, centre=(0.0, 0.0, -40.0), spread=4.0, scale=(0.4, 1.6)):
    """n transforms unlike any scene's: random places within `spread` of `centre`, random rotations, non-uniform scales."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=R.TRANSFORM_DTYPE)
    for k in range(n):
        pos = np.asarray(centre) + rng.uniform(-spread, spread, size=3)
        out[k] = transform(pos, rotation(rng.normal(size=3), rng.uniform(0, 2 * np.pi)), rng.uniform(*scale, size=3))[0]
    return out


def raw(a, size):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).reshape(-1, size)


# ---- 1. the record ---------------------------------------------------------------------------------------------------------------
def test_transform_dtype_is_rt_transform():
    assert R.TRANSFORM_DTYPE.itemsize == 128 and R.TRANSFORM_DTYPE.names == ("mv", "mvInverse")
    header = (ROOT / "include" / "rt_records.h").read_text()
    body = header[header.index("typedef struct rt_transform {"):header.index("} rt_transform;")]
    assert re.findall(r"^\s*float\s+(\w+)\[(\d+)\];", body, flags=re.M) == [("mv", "16"), ("mvInverse", "16")]
    assert re.search(r"RT_STATIC_ASSERT\(sizeof\(rt_transform\) == 128", header)
    assert R.TRANSFORM_DTYPE.fields["mv"][1] == 0 and R.TRANSFORM_DTYPE.fields["mvInverse"][1] == 64
    for name in R.TRANSFORM_DTYPE.names:
        assert R.TRANSFORM_DTYPE.fields[name][0] == R.OBJECT_DTYPE.fields[name][0]
    assert R.OBJECT_DTYPE.fields["mvInverse"][1] - R.OBJECT_DTYPE.fields["mv"][1] == 64
    # ... and bytes 64 .. 191 of an object are its transform
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    assert np.array_equal(raw(objs, 320)[:, 64:192], raw(R.transforms_of(objs), 128))


# ---- 2. the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [(0, 12), (0, 1), (3, 5), (11, 1), (12, 0), (5, 0)])
def test_with_transforms_changes_exactly_the_range(first, count):
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    assert len(objs) == 12
    xf = new_transforms(count, seed=3)
    before = objs.copy()
    out = R.with_transforms(objs, xf, first)
    assert np.array_equal(raw(objs, 320), raw(before, 320))                       # the input is not touched
    raw_in, raw_out = raw(objs, 320), raw(out, 320)
    assert np.array_equal(raw_out[:, :64], raw_in[:, :64]) and np.array_equal(raw_out[:, 256:], raw_in[:, 256:])   # materials, type, padding: everywhere
    outside = np.ones(len(objs), dtype=bool)
    outside[first:first + count] = False
    assert np.array_equal(raw_out[outside], raw_in[outside])                      # the neighbours, whole
    assert np.array_equal(raw_out[first:first + count, 64:192], raw(xf, 128))
    assert np.array_equal(raw(R.transforms_of(out)[first:first + count], 128), raw(xf, 128))   # the round trip
    for k in range(count):                                                         # mvInverseTranspose: the transpose, the same bits
        inv = xf["mvInverse"][k].reshape(4, 4)
        assert np.array_equal(as_words(out["mvInverseTranspose"][first + k]), as_words(np.ascontiguousarray(inv.T).reshape(16)))
    # an object array as the source: its matrices are taken, nothing else
    donor = R.with_transforms(R.with_materials(objs[::-1].copy(), new_materials(12, seed=4)), xf, 0) if count else objs[:0]
    out2 = R.with_transforms(objs, donor[:count], first)
    assert np.array_equal(raw(out2, 320), raw_out)


def test_round_trip_of_a_whole_array():
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    xf = R.transforms_of(objs)
    assert xf.dtype == R.TRANSFORM_DTYPE and len(xf) == len(objs)
    again = R.with_transforms(objs, xf)
    assert np.array_equal(raw(again, 320)[:, :192], raw(objs, 320)[:, :192]) and np.array_equal(raw(again, 320)[:, 256:], raw(objs, 320)[:, 256:])
    assert np.array_equal(raw(R.transforms_of(xf), 128), raw(xf, 128)) and R.transforms_of(xf) is not xf   # a transform array passes, copied


def test_with_transforms_refuses_a_range_beyond_the_objects():
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    for first, count in ((12, 1), (0, 13), (7, 6), (-1, 1)):
        with pytest.raises(ValueError):
            R.with_transforms(objs, new_transforms(count, seed=1), first)


# ---- 3. names --------------------------------------------------------------------------------------------------------------------
def test_names_and_abi():
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    names = ("rt_set_transforms", "rt_set_transforms_multi", "rt_read_transforms", "rt_get_geometry_info")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert "---- replaceable transforms" in header and "dlsym of rt_set_transforms" in header
    from opencl_raytracer_amd import cpu_raytracer, distributed, hip_raytracer
    for name in names:
        assert name in hip_raytracer.EXPORTS
    for cls, methods in ((hip_raytracer.HIPRaytracer, ("set_transforms", "read_transforms", "geometry_info")),
                         (hip_raytracer.MultiHIPRaytracer, ("set_transforms",)), (distributed.ShardedHIPRaytracer, ("set_transforms",)),
                         (cpu_raytracer.CPURaytracer, ("set_transforms",))):
        for name in methods:
            assert callable(getattr(cls, name)), (cls, name)
    # rt_geometry_info_t: four words, 64 ids, two words, a double
    body = header[header.index("typedef struct rt_geometry_info_t {"):header.index("} rt_geometry_info_t;")]
    declared = [(m.group(1), m.group(2)) for m in re.finditer(r"^\s*(uint32_t|double)\s+(\w+)", body, flags=re.M)]
    assert [n for _, n in declared] == [n for n, _ in hip_raytracer.RTGeometryInfo._fields_]
    assert ctypes.sizeof(hip_raytracer.RTGeometryInfo) == 4 * 4 + 4 * 64 + 2 * 4 + 8
    csrc = ROOT / "opencl-raytracer_amd" / "csrc"
    makefile = (csrc / "Makefile").read_text()
    for name in ("rt_transforms.hip", "rt_transforms.o", "rt_transforms.h", "rt_geometry.cpp", "rt_geometry.o"):
        assert name in makefile, name
    assert (csrc / "rt_transforms.hip").exists() and (csrc / "rt_transforms.h").exists() and (csrc / "rt_geometry.cpp").exists()
    assert "check_set_transforms" in (csrc / "rt_context.h").read_text() and "check_set_transforms" in (csrc / "rt_multi.cpp").read_text()
    host = ROOT / "opencl-raytracer_amd" / "host"
    assert "hip_raytracer_host_transforms_test" in (host / "Makefile").read_text() and (host / "host_transforms_test.cpp").exists()
    for hpp in ("HIPRaytracer.hpp", "CPURaytracer.hpp"):
        assert re.search(r"void\s+SetTransforms\s*\(\s*uint32_t\s+first", (host / hpp).read_text()), hpp


# ---- 4. the CPU backend ----------------------------------------------------------------------------------------------------------
def fixture_scene():
    fx = load_fixture("directional_shade_and_reflect")
    objs = fx["objs"]
    centre = np.array([R.transforms_of(objs)["mv"][:, 12 + a].mean() for a in range(3)], dtype=np.float64)   # where the scene's objects are
    return fx, objs, centre


def test_cpu_backend_set_transforms_equals_fresh():
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    fx, objs, centre = fixture_scene()
    lights, rays, depth = fx["lights"], fx["rays"], fx["max_bounces"]
    n = len(objs)
    A, B, C = new_transforms(n, seed=5, centre=centre, spread=2.0), new_transforms(4, seed=6, centre=centre, spread=1.0), new_transforms(1, seed=7, centre=centre, spread=0.5)
    constructor = CPURaytracer(objs, lights, rays, depth).Render()
    rt = CPURaytracer(objs, lights, rays, depth)
    e1 = R.with_transforms(objs, A)
    e2 = R.with_transforms(e1, B, 5)
    e3 = R.with_transforms(e2, C, 6)
    e4 = R.with_transforms(e3, B[1:2], 6)
    steps = [("all", A, 0, e1), ("four in the middle", B, 5, e2),          # calls add up
             ("one of them to a third place", C, 6, e3), ("... and back to its second place", B[1:2], 6, e4),
             ("the last one, from an object array", objs[n - 1:], n - 1, R.with_transforms(e4, objs[n - 1:], n - 1)),
             ("the originals", R.transforms_of(objs), 0, objs)]
    frames = []
    for label, xf, first, expect in steps:
        rt.set_transforms(xf, first)
        got = rt.Render()
        fresh = CPURaytracer(expect, lights, rays, depth)
        want = fresh.Render()
        assert np.array_equal(as_words(got), as_words(want)), label
        assert (rt.rays_traced, rt.hit_pixels) == (fresh.rays_traced, fresh.hit_pixels), label
        frames.append(got)
    assert np.array_equal(as_words(frames[-1]), as_words(constructor))
    assert not np.array_equal(as_words(frames[0]), as_words(constructor)) and not np.array_equal(as_words(frames[0]), as_words(frames[1]))
    assert not np.array_equal(as_words(frames[2]), as_words(frames[1])) and np.array_equal(as_words(frames[3]), as_words(frames[1]))
    with pytest.raises(ValueError):
        rt.set_transforms(A, 1)


@pytest.mark.parametrize("kernel", ["hittest", "shade"])
def test_cpu_backend_other_kernels(kernel):
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    fx, objs, centre = fixture_scene()
    lights, rays, depth = fx["lights"], fx["rays"], fx["max_bounces"]
    A = new_transforms(5, seed=9, centre=centre, spread=2.0)
    rt = CPURaytracer(objs, lights, rays, depth, kernel=kernel)
    before = rt.Render()
    rt.set_transforms(A, 3)
    got = rt.Render()
    assert np.array_equal(as_words(got), as_words(CPURaytracer(R.with_transforms(objs, A, 3), lights, rays, depth, kernel=kernel).Render()))
    assert not np.array_equal(as_words(got), as_words(before))


def test_cpu_backend_set_transforms_with_the_other_setters():
    from opencl_raytracer_amd import rays as RY
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    fx, objs, centre = fixture_scene()
    lights, rays, depth = fx["lights"], fx["rays"], fx["max_bounces"]
    W, H = fx["camera"][0], fx["camera"][1]
    A, mats = new_transforms(6, seed=8, centre=centre, spread=2.0), new_materials(len(objs), seed=8)
    other_lights = lights.copy()
    other_lights["position"][:, 0] += F(3.0)
    M = np.array([[0.98, 0.0, 0.199], [0.0, 1.0, 0.0], [-0.199, 0.0, 0.98]])
    posed = RY.posed_rays(W, H, -float(H), M, (0.5, 0.0, 1.0))
    moved = R.with_transforms(objs, A, 2)
    want = CPURaytracer(R.with_materials(moved, mats), other_lights, posed, depth).Render()
    for order in ("transforms first", "transforms last"):
        rt = CPURaytracer(objs, lights, rays, depth)
        if order == "transforms first":
            rt.set_transforms(A, 2)
        rt.set_materials(mats)
        rt.set_lights(other_lights)
        rt.set_rays(posed)
        if order == "transforms last":
            rt.set_transforms(A, 2)
        assert np.array_equal(as_words(rt.Render()), as_words(want)), order
        rt.set_pose(W, H, -float(H), M, (0.5, 0.0, 1.0))
        assert np.array_equal(as_words(rt.Render()), as_words(want)), order
    # ... and without materials: the transforms alone go with a pose
    rt = CPURaytracer(objs, lights, rays, depth)
    rt.set_pose(W, H, -float(H), M, (0.5, 0.0, 1.0))
    rt.set_transforms(A, 2)
    assert np.array_equal(as_words(rt.Render()), as_words(CPURaytracer(moved, lights, posed, depth).Render()))
