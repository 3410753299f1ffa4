"""Ray queries without a GPU: the CPU backend's query (the executable definition of HIPRaytracer.query_closest / query_occluded),
the per-ray route predicate, and the names.

1. CPURaytracer.query_closest on every golden hittest fixture's own rays (hittest_*, box_edges_hittest, general_w_hittest,
   index_recovery_hittest) and on the tie_* fixtures' rays: t equals the CPU backend's hittest Render of the same rays bit for bit
   (Render writes MAX_FLOAT where the loop's time is not < MAX_FLOAT, so a NaN time - which the query returns as it is - compares
   against MAX_FLOAT there), and on the hittest fixtures the reference's own recorded times. No fixture records a winner index, so
   the index is checked by self-consistency (3) and, on the tie fixtures, against the reference's tie rules;
2. occluded equals the predicate !(t >= 1 or t < 0) applied to t;
3. index self-consistency: for every hit, a query with only that object visible returns the same t, bit for bit;
4. rays.query_route at its boundaries: dd at 1e-30 and 1e30 on either side, the last float inside and the first float outside each
   face of the box, start.w = 2, direction.w = 1, one NaN, one inf; and the inward rounding of the box;
5. the live state: set_transforms / set_visibility enter the query as records.with_transforms / with_visibility do;
6. names: header, wrappers, Makefiles, EXPORTS, ABI 3, sizeof(rt_query_info_t)."""
import ctypes
import re

import numpy as np
import pytest

from helpers import R, ROOT, fixture_names, load_fixture, same_floats
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer

F = np.float32
MAX_FLOAT = F(3.402823466e+38)
NAMES = ("rt_query_closest_device", "rt_query_occluded_device", "rt_query_closest", "rt_query_occluded", "rt_query_primary",
         "rt_get_query_info")
HITTEST = [n for n in fixture_names() if n.startswith("hittest_") or n in ("box_edges_hittest", "general_w_hittest", "index_recovery_hittest")]
TIES = [n for n in fixture_names() if n.startswith("tie_")]


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def predicate(t):
    with np.errstate(invalid="ignore"):
        return (~((t >= F(1.0)) | (t < F(0.0)))).astype(np.uint8)


def test_the_fixture_lists():
    assert len(HITTEST) == 5 and len(TIES) == 3


# ---- 1, 2. against the hittest frame of the same rays ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HITTEST + TIES)
def test_query_equals_the_hittest_frame(name):
    fx = load_fixture(name)
    objs, rays = fx["objs"], fx["rays"]
    cpu = CPURaytracer(objs, fx["lights"], rays, 0, kernel="hittest")
    frame = cpu.Render()
    t, index = cpu.query_closest(rays)
    assert t.shape == frame.shape and index.shape == frame.shape and index.dtype == np.int32
    with np.errstate(invalid="ignore"):
        hit = t < MAX_FLOAT
    as_frame = np.where(hit, t, MAX_FLOAT).astype(F)
    assert np.array_equal(words(as_frame), words(frame))
    assert hit.any()
    assert np.array_equal(index >= 0, hit) and (index[~hit] == -1).all() and (index[hit] < len(objs)).all()
    if fx["kernel"] == 0:   # the reference's own times for these rays (same_floats: the sign of a zero is implementation-defined there)
        assert same_floats(as_frame, fx["out_fused"])
    occluded = cpu.query_occluded(rays)
    assert occluded.dtype == np.uint8 and np.array_equal(occluded, predicate(t))
    # a second backend object, other frame rays, another kernel: the query depends on the objects and its own rays only
    other = CPURaytracer(objs, fx["lights"], rays[:1], 3, kernel="shade_and_reflect")
    t2, index2 = other.query_closest(rays)
    assert np.array_equal(words(t2), words(t)) and np.array_equal(index2, index)


def test_ties_go_to_the_later_sphere_and_the_earlier_box():
    for name, winners in (("tie_two_spheres", {1}), ("tie_two_boxes", {0})):
        fx = load_fixture(name)
        a, b = fx["objs"][0], fx["objs"][1]
        if not np.array_equal(a["mvInverse"], b["mvInverse"]):
            continue   # (the fixture's two objects are not coincident everywhere: nothing to state for every ray)
        _, index = CPURaytracer(fx["objs"], fx["lights"], fx["rays"], 0, kernel="hittest").query_closest(fx["rays"])
        assert set(np.unique(index[index >= 0])) == winners, name


# ---- 3. index self-consistency -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hittest_spheres", "hittest_boxes", "index_recovery_hittest", "tie_sphere_box_sphere"])
def test_the_named_object_alone_gives_the_same_time(name):
    fx = load_fixture(name)
    objs, rays = fx["objs"], fx["rays"]
    cpu = CPURaytracer(objs, fx["lights"], rays, 0, kernel="hittest")
    t, index = cpu.query_closest(rays)
    winners = np.unique(index[index >= 0])
    assert winners.size >= 1
    for k in winners:
        mask = np.zeros(len(objs), dtype=np.uint8)
        mask[k] = 1
        alone = CPURaytracer(objs, fx["lights"], rays, 0, kernel="hittest")
        alone.set_visibility(mask)
        sel = index == k
        ta, ia = alone.query_closest(rays[sel])
        assert np.array_equal(words(ta), words(t[sel])) and (ia == k).all(), f"{name}: object {k}"


# ---- 4. the route predicate --------------------------------------------------------------------------------------------------------
LO, HI = np.array([-3.1, -2.2, -50.3]), np.array([4.7, 5.9, -1.3])   # no float32 numbers: the inward rounding matters


def ray(start=(0.0, 0.0, -10.0, 1.0), direction=(0.0, 0.0, -1.0, 0.0)):
    r = np.zeros(1, dtype=R.RAY_DTYPE)
    r["start"][0] = np.asarray(start, dtype=F)
    r["direction"][0] = np.asarray(direction, dtype=F)
    return r


def route(r):
    return bool(RY.query_route(r, LO, HI)[0])


def test_route_of_a_plain_ray_and_of_no_grid():
    assert route(ray())
    assert not RY.query_route(ray(), None, None)[0]
    assert RY.query_route(np.zeros(0, dtype=R.RAY_DTYPE), LO, HI).shape == (0,)


def test_inward_box():
    lo, hi = RY.inward_box(LO, HI)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert (lo.astype(np.float64) >= LO).all() and (hi.astype(np.float64) <= HI).all()
    assert (np.nextafter(lo, F(-np.inf)).astype(np.float64) < LO).all() and (np.nextafter(hi, F(np.inf)).astype(np.float64) > HI).all()
    exact_lo, exact_hi = RY.inward_box([-2.0, 0.5, -64.0], [2.0, 0.75, 1.0])   # float32 numbers stay
    assert np.array_equal(exact_lo, np.array([-2.0, 0.5, -64.0], dtype=F)) and np.array_equal(exact_hi, np.array([2.0, 0.75, 1.0], dtype=F))


def dd_of(d):
    d = np.asarray(d, dtype=F)
    return F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))


@pytest.mark.parametrize("bound,inside_is_larger", [(1.0e-30, True), (1.0e30, False)])
def test_route_at_the_direction_window(bound, inside_is_larger):
    # directions along z whose dd = fl(z * z) lies on either side of the bound: walk z float by float across it
    z = F(np.sqrt(np.float64(F(bound))))
    while dd_of((0, 0, z)) > F(bound):
        z = np.nextafter(z, F(0))
    while dd_of((0, 0, z)) <= F(bound):
        z = np.nextafter(z, F(np.inf))
    above, below = z, np.nextafter(z, F(0))   # dd(above) > bound >= dd(below)
    assert dd_of((0, 0, above)) > F(bound) >= dd_of((0, 0, below))
    assert route(ray(direction=(0, 0, above, 0))) == inside_is_larger
    if dd_of((0, 0, below)) == F(bound):      # the bound itself is outside the open window
        assert not route(ray(direction=(0, 0, below, 0)))
    while dd_of((0, 0, below)) >= F(bound):
        below = np.nextafter(below, F(0))
    assert route(ray(direction=(0, 0, below, 0))) == (not inside_is_larger)
    assert not route(ray(direction=(0, 0, 0, 0)))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_route_at_the_faces_of_the_box(axis):
    lo, hi = RY.inward_box(LO, HI)
    for face, outward in ((lo, F(-np.inf)), (hi, F(np.inf))):
        s = np.array([0.0, 0.0, -10.0, 1.0], dtype=F)
        s[axis] = face[axis]
        assert route(ray(start=s)), "the last float inside"
        s[axis] = np.nextafter(face[axis], outward)
        assert not route(ray(start=s)), "the first float outside"
        assert not (LO[axis] <= np.float64(s[axis]) <= HI[axis])   # ... which the double box excludes too


def test_route_of_the_other_components():
    assert not route(ray(start=(0, 0, -10, 2)))
    assert not route(ray(direction=(0, 0, -1, 1)))
    assert not route(ray(start=(np.nan, 0, -10, 1)))
    assert not route(ray(direction=(0, np.nan, -1, 0)))
    assert not route(ray(start=(0, np.inf, -10, 1)))
    assert not route(ray(direction=(np.inf, 0, -1, 0)))
    assert not route(ray(direction=(-np.inf, 0, -1, 0)))
    many = np.concatenate([ray(), ray(start=(0, 0, -10, 2)), ray(), ray(direction=(0, 0, 0, 0))])
    assert RY.query_route(many, LO, HI).tolist() == [True, False, True, False]


# ---- 5. the live state -------------------------------------------------------------------------------------------------------------
def test_setters_enter_the_query():
    fx = load_fixture("index_recovery_hittest")
    objs, rays = fx["objs"], fx["rays"]
    cpu = CPURaytracer(objs, fx["lights"], rays, 0, kernel="hittest")
    t0, i0 = cpu.query_closest(rays)
    mask = (np.arange(len(objs)) % 2).astype(np.uint8)
    moved = R.transforms_of(objs[:3][::-1])
    cpu.set_visibility(mask)
    cpu.set_transforms(moved, 4)
    t1, i1 = cpu.query_closest(rays)
    want = R.with_visibility(R.with_transforms(objs, moved, 4), mask, 0)
    t2, i2 = CPURaytracer(want, fx["lights"], rays, 0, kernel="hittest").query_closest(rays)
    assert np.array_equal(words(t1), words(t2)) and np.array_equal(i1, i2)
    assert not np.array_equal(i1, i0)
    assert not np.isin(i1[i1 >= 0], np.nonzero(mask == 0)[0]).any()
    frame = cpu.Render()   # ... and the frame of the same object agrees with its query
    with np.errstate(invalid="ignore"):
        assert np.array_equal(words(np.where(t1 < MAX_FLOAT, t1, MAX_FLOAT)), words(frame))


def test_an_empty_query_and_an_empty_scene():
    fx = load_fixture("hittest_spheres")
    cpu = CPURaytracer(fx["objs"], fx["lights"], fx["rays"], 0, kernel="hittest")
    t, index = cpu.query_closest(fx["rays"][:0])
    assert t.shape == (0,) and index.shape == (0,) and cpu.query_occluded(fx["rays"][:0]).shape == (0,)
    t, index = CPURaytracer(fx["objs"][:0], fx["lights"], fx["rays"], 0, kernel="hittest").query_closest(fx["rays"][:5])
    assert (t == MAX_FLOAT).all() and (index == -1).all()


# ---- 6. names ----------------------------------------------------------------------------------------------------------------------
def test_names():
    from opencl_raytracer_amd import hip_raytracer
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert "dlsym of rt_query_closest_device" in header and "NOT part of this call" in header
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in hip_raytracer.EXPORTS
    for method in ("query_closest", "query_occluded", "pick", "query_info"):
        assert callable(getattr(hip_raytracer.HIPRaytracer, method)) and callable(getattr(hip_raytracer.MultiHIPRaytracer, method))
    assert ctypes.sizeof(hip_raytracer.RTQueryInfo) == 40
    assert re.search(r"typedef struct rt_query_info_t \{\s*uint64_t n_rays;[^}]*uint64_t n_grid;[^}]*uint64_t n_brute;[^}]*uint64_t object_tests;"
                     r"[^}]*double device_ms;\s*\} rt_query_info_t;", header)
    make = (ROOT / "opencl-raytracer_amd" / "csrc" / "Makefile").read_text()
    for word in ("rt_query.hip", "rt_query.o", "rt_query.h", "rt_query_host.cpp", "rt_query_host.o", "rt_query.s"):
        assert word in make, word
    host_make = (ROOT / "opencl-raytracer_amd" / "host" / "Makefile").read_text()
    assert "hip_raytracer_host_query_test" in host_make
    hpp = (ROOT / "opencl-raytracer_amd" / "host" / "HIPRaytracer.hpp").read_text()
    cpu_hpp = (ROOT / "opencl-raytracer_amd" / "host" / "CPURaytracer.hpp").read_text()
    for method in ("QueryClosest", "QueryOccluded", "Pick"):
        assert method in hpp
    assert "QueryClosest" in cpu_hpp and "QueryOccluded" in cpu_hpp
    assert "pick" in (ROOT / "opencl-raytracer_amd" / "host" / "scene_tool.cpp").read_text()


def test_the_library_exports_the_entry_points():
    from opencl_raytracer_amd import hip_raytracer
    if not hip_raytracer.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = hip_raytracer.load_library()   # dlopen + declarations: needs no GPU
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rt_query_closest(None, None, 0, None, None) == -1   # a NULL context: RT_ERR_INVALID_ARGUMENT, nothing dereferenced
    assert lib.rt_get_query_info(None, None) == -1


# ---- 7. scene_tool pick --------------------------------------------------------------------------------------------------------------
def test_scene_tool_pick_on_the_cpu_backend():
    import subprocess
    from helpers import SCENES
    from opencl_raytracer_amd import camera, scene_loader
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H = 96, 64
    scene_file = SCENES / "multipleSpheres.txt"   # its C++ and Python loaders agree bit for bit (tests/test_host_cpp_cpu.py)
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)              # 60 degrees of vertical field of view; the tool is given this z by its bits
    z_bits = format(int(np.float32(rays["direction"][0, 2]).view(np.uint32)), "x")
    t, index = CPURaytracer(objs, lts, rays[:1], 0, kernel="hittest").query_closest(rays)
    assert (index >= 0).any() and (index < 0).any()
    seen = set()
    for i, j in ((48, 32), (0, 0), (95, 63), (30, 32), (66, 30)):
        res = subprocess.run([str(tool), "pick", str(scene_file), str(W), str(H), str(i), str(j), "cpu", z_bits], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        word, k, time, backend = res.stdout.strip().splitlines()[-1].split()
        assert word == "pick" and backend == "cpu"
        assert int(k) == index[j * W + i] and np.float32(time) == t[j * W + i], (i, j, res.stdout)
        seen.add(int(k))
    assert len(seen) >= 2
    res = subprocess.run([str(tool), "pick", str(scene_file), str(W), str(H), str(W), "0", "cpu"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 1


# ---- 8. plain float32 arrays ---------------------------------------------------------------------------------------------------------
def test_rays_as_an_n_by_8_float32_array():
    fx = load_fixture("general_w_hittest")
    rays = fx["rays"]
    plain = rays.view(np.float32).reshape(-1, 8).copy()
    assert plain.shape == (len(rays), 8)
    again = R.rays_of(plain)
    assert again.dtype == R.RAY_DTYPE and again.shape == rays.shape and again.tobytes() == rays.tobytes()
    assert R.rays_of(rays).tobytes() == rays.tobytes() and R.rays_of(plain.reshape(2, -1, 8)).tobytes() == rays.tobytes()
    assert R.rays_of(plain[3]).shape == (1,) and R.rays_of(plain[:0]).shape == (0,)
    cpu = CPURaytracer(fx["objs"], fx["lights"], rays, 0, kernel="hittest")
    t, index = cpu.query_closest(rays)
    t2, index2 = cpu.query_closest(plain)
    assert (index >= 0).any() and np.array_equal(words(t2), words(t)) and np.array_equal(index2, index)
    assert np.array_equal(cpu.query_occluded(plain), cpu.query_occluded(rays))
    for bad in (plain[:, :7], plain.astype(np.float64), plain.reshape(-1), np.float32(1.0), np.arange(8)):
        with pytest.raises(ValueError):
            R.rays_of(bad)
        with pytest.raises(ValueError):
            cpu.query_closest(bad)
