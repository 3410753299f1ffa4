"""Replaceable materials without a GPU: the names, the executable definition (records.with_materials) and the CPU backend.

1. MATERIAL_DTYPE is rt_material: 64 bytes, the offsets of rt_records.h, the first four fields of OBJECT_DTYPE;
2. with_materials changes exactly the material fields of the range, from a material array and from an object array;
3. names: header, wrappers, Makefile, EXPORTS, ABI 3;
4. CPURaytracer.set_materials equals a fresh CPU backend created with with_materials(...) on a golden-fixture scene, bit for
   bit, overlapping calls add up, and the originals put back give the constructor's frame.
The material sets here are the GPU tests' (test_set_materials_gpu.py)."""
import re

import numpy as np
import pytest

from helpers import R, ROOT, load_fixture

F = np.float32
DEAD = ("reflection", "transparency")   # read by no kernel, like the pad lane of each colour


def new_materials(n, seed, absorption=(1.0, 0.7, 0.4)):
    """n materials unlike any scene's: random colours, and - because no kernel reads them - random reflection, transparency and
    pad lanes, which must not matter."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=R.MATERIAL_DTYPE)
    for name in ("ambient", "diffuse", "specular"):
        m[name] = rng.uniform(0.0, 1.0, size=(n, 4)).astype(F)
    m["absorption"] = rng.choice(np.array(absorption, dtype=F), size=n)
    m["shininess"] = rng.choice(np.array([0.5, 1.0, 5.0, 30.0, 100.0], dtype=F), size=n)
    m["reflection"] = rng.uniform(0.0, 1.0, size=n).astype(F)
    m["transparency"] = rng.uniform(0.0, 1.0, size=n).astype(F)
    return m


def live_words(materials):
    """What rt_read_materials returns for these materials: the eleven floats the kernels read, the five other words 0."""
    m = R.materials_of(materials)
    for name in ("ambient", "diffuse", "specular"):
        m[name][:, 3] = 0
    for name in DEAD:
        m[name] = 0
    return m


def as_words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the record ---------------------------------------------------------------------------------------------------------------
def test_material_dtype_is_rt_material():
    assert R.MATERIAL_DTYPE.itemsize == 64
    header = (ROOT / "include" / "rt_records.h").read_text()
    body = header[header.index("typedef struct rt_material {"):header.index("} rt_material;")]
    declared = []
    for ty, names in re.findall(r"^\s*(float)\s+([^;]+);", body, flags=re.M):
        for nm in names.split(","):
            m = re.search(r"(\w+)\s*(?:\[(\d+)\])?", nm.strip())
            declared.append((m.group(1), int(m.group(2) or 1)))
    assert declared == [("ambient", 4), ("diffuse", 4), ("specular", 4), ("absorption", 1), ("reflection", 1), ("transparency", 1), ("shininess", 1)]
    offset = 0
    for name, count in declared:   # C floats, no padding: the offsets add up
        assert R.MATERIAL_DTYPE.fields[name][1] == offset == R.OBJECT_DTYPE.fields[name][1], name
        assert R.MATERIAL_DTYPE.fields[name][0] == R.OBJECT_DTYPE.fields[name][0], name
        offset += 4 * count
    assert offset == 64 and R.OBJECT_DTYPE.fields["mv"][1] == 64
    assert R.MATERIAL_DTYPE.names == R.OBJECT_DTYPE.names[:7] == R.MATERIAL_FIELDS
    # ... and an object's first 64 bytes are its material
    fx = load_fixture("directional_shade_and_reflect")
    raw = np.frombuffer(fx["objs"].tobytes(), dtype=np.uint8).reshape(-1, 320)[:, :64]
    assert np.array_equal(raw, np.frombuffer(R.materials_of(fx["objs"]).tobytes(), dtype=np.uint8).reshape(-1, 64))


# ---- 2. the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [(0, 12), (0, 1), (3, 5), (11, 1), (12, 0), (5, 0)])
def test_with_materials_changes_exactly_the_range(first, count):
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    assert len(objs) == 12
    mats = new_materials(count, seed=3)
    before = objs.copy()
    out = R.with_materials(objs, mats, first)
    assert np.array_equal(as_words(objs.view(np.uint8)), as_words(before.view(np.uint8)))   # the input is not touched
    raw_in = np.frombuffer(objs.tobytes(), dtype=np.uint8).reshape(-1, 320)
    raw_out = np.frombuffer(out.tobytes(), dtype=np.uint8).reshape(-1, 320)
    assert np.array_equal(raw_out[:, 64:], raw_in[:, 64:])                       # matrices, type, padding: everywhere
    outside = np.ones(len(objs), dtype=bool)
    outside[first:first + count] = False
    assert np.array_equal(raw_out[outside, :64], raw_in[outside, :64])           # the neighbours' materials
    assert np.array_equal(raw_out[first:first + count, :64], np.frombuffer(mats.tobytes(), dtype=np.uint8).reshape(-1, 64))
    # an object array as the source: its material fields are taken, nothing else
    donor = R.with_materials(objs[::-1].copy(), mats, 0) if count else objs[:0]
    out2 = R.with_materials(objs, donor[:count], first)
    assert np.array_equal(np.frombuffer(out2.tobytes(), dtype=np.uint8), np.frombuffer(out.tobytes(), dtype=np.uint8))


def test_with_materials_refuses_a_range_beyond_the_objects():
    objs = load_fixture("directional_shade_and_reflect")["objs"]
    for first, count in ((12, 1), (0, 13), (7, 6), (-1, 1)):
        with pytest.raises(ValueError):
            R.with_materials(objs, new_materials(count, seed=1), first)


# ---- 3. names --------------------------------------------------------------------------------------------------------------------
def test_names_and_abi():
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    names = ("rt_set_materials", "rt_set_materials_device", "rt_set_materials_multi", "rt_read_materials")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    from opencl_raytracer_amd import cpu_raytracer, distributed, hip_raytracer
    for name in names:
        assert name in hip_raytracer.EXPORTS
    for cls, methods in ((hip_raytracer.HIPRaytracer, ("set_materials", "read_materials")), (hip_raytracer.MultiHIPRaytracer, ("set_materials",)),
                         (distributed.ShardedHIPRaytracer, ("set_materials",)), (cpu_raytracer.CPURaytracer, ("set_materials",))):
        for name in methods:
            assert callable(getattr(cls, name)), (cls, name)
    csrc = ROOT / "opencl-raytracer_amd" / "csrc"
    makefile = (csrc / "Makefile").read_text()
    assert "rt_materials.hip" in makefile and "rt_materials.o" in makefile
    assert (csrc / "rt_materials.hip").exists() and (csrc / "rt_materials.h").exists()
    host = ROOT / "opencl-raytracer_amd" / "host"
    assert "hip_raytracer_host_materials_test" in (host / "Makefile").read_text() and (host / "host_materials_test.cpp").exists()
    for hpp in ("HIPRaytracer.hpp", "CPURaytracer.hpp"):
        assert re.search(r"void\s+SetMaterials\s*\(\s*uint32_t\s+first", (host / hpp).read_text()), hpp


# ---- 4. the CPU backend ----------------------------------------------------------------------------------------------------------
def test_cpu_backend_set_materials_equals_fresh():
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    fx = load_fixture("directional_shade_and_reflect")
    objs, lights, rays, depth = fx["objs"], fx["lights"], fx["rays"], fx["max_bounces"]
    n = len(objs)
    A, B = new_materials(n, seed=5), new_materials(4, seed=6, absorption=(1.0, 0.5))
    constructor = CPURaytracer(objs, lights, rays, depth).Render()
    rt = CPURaytracer(objs, lights, rays, depth)
    steps = [("all", A, 0, R.with_materials(objs, A)),
             ("four in the middle", B, 5, R.with_materials(R.with_materials(objs, A), B, 5)),      # calls add up
             ("the last one, from an object array", objs[:1], n - 1, R.with_materials(R.with_materials(R.with_materials(objs, A), B, 5), objs[:1], n - 1)),
             ("the originals", R.materials_of(objs), 0, objs)]
    frames = []
    for label, mats, first, expect in steps:
        rt.set_materials(mats, first)
        got = rt.Render()
        fresh = CPURaytracer(expect, lights, rays, depth)
        want = fresh.Render()
        assert np.array_equal(as_words(got), as_words(want)), label
        assert (rt.rays_traced, rt.hit_pixels) == (fresh.rays_traced, fresh.hit_pixels), label
        frames.append(got)
    assert np.array_equal(as_words(frames[-1]), as_words(constructor))
    assert not np.array_equal(as_words(frames[0]), as_words(constructor)) and not np.array_equal(as_words(frames[0]), as_words(frames[1]))
    with pytest.raises(ValueError):
        rt.set_materials(A, 1)


def test_cpu_backend_set_materials_with_replaced_rays_and_pose():
    from opencl_raytracer_amd import rays as RY
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    fx = load_fixture("directional_shade_and_reflect")
    objs, lights, rays, depth = fx["objs"], fx["lights"], fx["rays"], fx["max_bounces"]
    W, H = fx["camera"][0], fx["camera"][1]
    A = new_materials(len(objs), seed=8)
    M = np.array([[0.98, 0.0, 0.199], [0.0, 1.0, 0.0], [-0.199, 0.0, 0.98]])
    posed = RY.posed_rays(W, H, -float(H), M, (0.5, 0.0, 1.0))
    want = CPURaytracer(R.with_materials(objs, A), lights, posed, depth).Render()
    rt = CPURaytracer(objs, lights, rays, depth)
    rt.set_materials(A)
    rt.set_rays(posed)
    assert np.array_equal(as_words(rt.Render()), as_words(want))
    rt.set_pose(W, H, -float(H), M, (0.5, 0.0, 1.0))
    assert np.array_equal(as_words(rt.Render()), as_words(want))
