"""Hit-record queries without a GPU (hip_raytracer.h, "hit-record queries"): the CPU backend's query_hits / hit_records (the
executable definition of HIPRaytracer.query_hits in the default arithmetic), hits.hit_records (the definition under
RT_FLAG_UNFUSED), hits.chain, and the names.

1. CPURaytracer.query_hits: (t, index) are query_closest's, the records are hit_records(rays, t, index) of the same backend, zero
   records on misses and on masked rays;
2. the link to verified code: on a shade_and_reflect golden scene (whose Render the fixtures pin) the chain's first reflected ray is
   the one built by hand from the point, the normal and the ray's direction, and traced by query_closest it gives the chain's second
   bounce; the reflected start lies within 0.0011 (1 + |P|) of the point and |normal|^2 - 1 within 4 * 2^-23;
3. hits.hit_records against the float64 restatement's cast() on the rays it calls stable: the definition is the reference's geometry;
4. conditions on the inputs the GPU tests use: enough sphere hits, box hits and misses; NaN and finite normals on the tiny far box;
5. names: header, wrappers, Makefiles, EXPORTS, ABI 3, sizeof(rt_hits_t)."""
import ctypes
import re

import numpy as np
import pytest

from helpers import R, ROOT, load_fixture, same_floats
from opencl_raytracer_amd import hits as HT
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from oracle import f64
from test_device_opencl_fuzz_gpu import obj, rays_to
from test_set_materials_gpu import cloud, lights

F = np.float32
MAX_FLOAT = F(3.402823466e+38)
NAMES = ("rt_query_hits_device", "rt_query_hits", "rt_query_primary_hits")
RECORDS = ("point", "normal", "reflected")
U = 2.0 ** -23
SEEDS = (5, 14, 21)
# 3: the largest deviation of hits.hit_records from oracle/f64.py's cast() over its stable rays of cloud_rays(1000, seed) for SEEDS,
# measured on the CPU: the point 1.02e-6 of the scene scale (the largest |centre coordinate|, 45.98), the normal 6.2e-5 absolute
# (fp32 rounding of the object-space point, amplified by the instances' scales) - with a 4x margin: the restatement's own error is
# float64's, the deviation is fp32 rounding that varies with the seed.
TOL_POINT_REL = 4.1e-6
TOL_NORMAL_ABS = 2.5e-4


def words(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint32)


def floats(rays):
    return np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)


def centres(objs):
    return objs["mv"].reshape(len(objs), 16)[:, 12:15].astype(np.float64)


def cloud_rays(n, seed, objs=None):
    """test_query_gpu.in_box_rays without a GPU: the box is the centres' +- 1 instead of the context's."""
    objs = cloud() if objs is None else objs
    c = centres(objs)
    lo, hi = c.min(axis=0) - 1.0, c.max(axis=0) + 1.0
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.99
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays["start"][:, :3] = (mid + rng.uniform(-1.0, 1.0, size=(n, 3)) * half).astype(F)
    rays["start"][:, 3] = 1.0
    aim = c[rng.integers(0, len(objs), size=n)] - rays["start"][:, :3].astype(np.float64)
    wander = rng.normal(size=(n, 3)) * rng.uniform(0.1, 30.0, size=(n, 1))
    rays["direction"][:, :3] = np.where((np.arange(n) % 2 == 0)[:, None], aim, wander).astype(F)
    return rays


def tiny_far_box(seed=45, n=512):
    """One box of 0.01 units 1 000 units away and n rays from near the origin at its front face (tiny_far_box_scene of
    test_device_opencl_fuzz_gpu.py): the object-space hit point carries the cancellation of 1e5-sized coordinates, so part of the
    hits have no coordinate beyond 0.4998 and get a zero object-space normal."""
    rng = np.random.default_rng(seed)
    c = np.array([0.3, -0.2, -1000.0])
    objs = R.objects_array([obj(R.BOX, c, 0.01, seed=1)])
    uv = rng.uniform(-0.45, 0.45, (n, 2)) * 0.01
    targets = c + np.stack([uv[:, 0], uv[:, 1], np.full(n, 0.005)], 1)
    return objs, rays_to(rng.uniform(-3, 3, (n, 3)).astype(F), targets)


def backend(objs, rays):
    return CPURaytracer(objs, lights(), rays[:1], 0, kernel="hittest")


def assert_zero_records(h, where, label):
    for k in RECORDS:
        assert not words(h[k][where]).any(), f"{label}: {k} is not all-zero bytes"


# ---- 1. the CPU backend's query ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_query_hits_is_query_closest_with_the_record_stage(seed):
    objs, rays = cloud(), cloud_rays(1000, seed)
    cpu = backend(objs, rays)
    t, index = cpu.query_closest(rays)
    h = cpu.query_hits(rays)
    assert np.array_equal(words(h["t"]), words(t)) and np.array_equal(h["index"], index)
    assert h["point"].shape == (1000, 4) and h["normal"].shape == (1000, 4) and h["reflected"].dtype == R.RAY_DTYPE
    rec = cpu.hit_records(rays, t, index)
    for k in RECORDS:
        assert np.array_equal(words(rec[k]), words(h[k])), k
    hit = index >= 0
    assert hit.any() and (~hit).any()
    assert_zero_records(h, ~hit, "misses")
    assert (h["normal"][hit, 3] == 0).all() and (h["point"][hit, 3] == 1).all()
    assert (h["reflected"]["start"][hit, 3] == 1).all() and (h["reflected"]["direction"][hit, 3] == 0).all()
    # a masked ray reads as a miss whatever it would have hit; the others are untouched
    mask = np.where(np.arange(1000) % 3 == 0, -1, 7).astype(np.int32)
    m = cpu.query_hits(rays, mask)
    off = mask < 0
    assert (hit & off).any()
    assert (m["t"][off] == MAX_FLOAT).all() and (m["index"][off] == -1).all()
    assert_zero_records(m, off, "masked rays")
    for k in ("t", "index") + RECORDS:
        assert np.array_equal(words(m[k][~off]), words(h[k][~off])), k
    # the live state enters as it enters query_closest
    vis = (np.arange(len(objs)) % 2).astype(np.uint8)
    cpu.set_visibility(vis)
    v = cpu.query_hits(rays)
    fresh = backend(R.with_visibility(objs, vis), rays).query_hits(rays)
    for k in ("t", "index") + RECORDS:
        assert np.array_equal(words(v[k]), words(fresh[k])), k
    assert not np.isin(v["index"][v["index"] >= 0], np.nonzero(vis == 0)[0]).any()


def test_an_empty_query():
    objs, rays = cloud(), cloud_rays(4, 1)
    h = backend(objs, rays).query_hits(rays[:0])
    assert h["t"].shape == (0,) and h["point"].shape == (0, 4) and h["reflected"].shape == (0,)
    with pytest.raises(ValueError):
        backend(objs, rays).query_hits(rays, np.zeros(3, dtype=np.int32))


# ---- 2. the link to verified code --------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c) with one rounding: the product of two float32 is exact in float64; the float64 sum is then rounded twice,
    which differs from one rounding only on a tie of the 29 dropped bits."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def reflection_by_hand(rays, point, normal):
    """reflect() and the next ray of the chain (shade_and_reflect_kernel.cl:68-70, :260-263) from the records, in the backend's
    association: dot and normalize left to right, the last step of reflect and the start contracted."""
    d, n = rays["direction"][:, :3].astype(F), normal[:, :3]
    with np.errstate(all="ignore"):
        k = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]) * F(-2.0)
        r = np.stack([fma32(k, n[:, c], d[:, c]) for c in range(3)], axis=1)
        length = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        u = r / length[:, None]
        k001 = np.full(len(rays), F(0.001))
        out = np.zeros(len(rays), dtype=R.RAY_DTYPE)
        out["start"][:, :3] = np.stack([fma32(u[:, c], k001, point[:, c]) for c in range(3)], axis=1)
        out["start"][:, 3] = point[:, 3]
        out["direction"][:, :3] = r
    return out


@pytest.mark.parametrize("name", ["scene_roundedCube_64_shade_and_reflect", "random_mixed100_shade_and_reflect"])
def test_the_first_reflected_ray_is_the_chains(name):
    fx = load_fixture(name)
    assert fx["kernel"] == 2
    objs, rays = fx["objs"], fx["rays"][:2048]
    cpu = CPURaytracer(objs, fx["lights"], rays[:1], fx["max_bounces"], kernel="shade_and_reflect")
    first, second = HT.chain(cpu.query_hits, rays, 2)
    hit = first["index"] >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 100
    by_hand = reflection_by_hand(rays[hit], first["point"][hit], first["normal"][hit])
    assert same_floats(floats(by_hand), floats(first["reflected"][hit]))
    t, index = cpu.query_closest(by_hand)
    assert np.array_equal(words(t), words(second["t"][hit])) and np.array_equal(index, second["index"][hit])
    assert (index >= 0).any()
    # the chain's mask: a ray that missed stays a zero record
    assert (second["index"][~hit] == -1).all() and (second["t"][~hit] == MAX_FLOAT).all()
    assert_zero_records(second, ~hit, "the second bounce of a miss")
    # the start leaves the surface by 0.001 along the reflection; the normal is a unit vector
    P, S = first["point"][hit, :3].astype(np.float64), first["reflected"]["start"][hit, :3].astype(np.float64)
    assert (np.linalg.norm(S - P, axis=1) <= 0.0011 * (1.0 + np.linalg.norm(P, axis=1))).all()
    n2 = (first["normal"][hit, :3].astype(np.float64) ** 2).sum(axis=1)
    assert np.isfinite(n2).all() and (np.abs(n2 - 1.0) <= 4 * U).all(), np.abs(n2 - 1.0).max() / U


# ---- 3. the definition against the float64 restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_hit_records_against_the_float64_restatement(seed, capsys):
    objs, rays = cloud(), cloud_rays(1000, seed)
    t, index = backend(objs, rays).query_closest(rays)
    fused = backend(objs, rays).hit_records(rays, t, index)
    plain = HT.hit_records(objs, rays, t, index)
    sc = f64.Scene(objs, lights())
    want_i, _, inter, normal, margin, _ = f64.cast(sc, rays["start"].astype(np.float64), rays["direction"].astype(np.float64))
    stable = (margin >= f64.TAU) & (want_i >= 0)
    assert np.array_equal(want_i[stable], index[stable])          # the winner is the restatement's wherever it commits itself
    assert stable.sum() >= 500
    scale = np.abs(centres(objs)).max()
    worst = {}
    for label, rec in (("hits.hit_records", plain), ("CPURaytracer.hit_records", fused)):
        dp = np.abs(rec["point"][stable, :3].astype(np.float64) - inter[stable, :3]).max() / scale
        dn = np.abs(rec["normal"][stable, :3].astype(np.float64) - normal[stable]).max()
        worst[label] = (dp, dn)
    with capsys.disabled():
        print(f"\n[hit records vs float64, seed {seed}: {int(stable.sum())} stable rays] " +
              "; ".join(f"{k}: point {v[0]:.3e} of the scale, normal {v[1]:.3e}" for k, v in worst.items()))
    for label, (dp, dn) in worst.items():
        assert dp <= TOL_POINT_REL and dn <= TOL_NORMAL_ABS, (label, dp, dn)
    # the reflected ray of the definition: direction = d - 2 (d . n) n of ITS normal, the start 0.001 along it
    hit = index >= 0
    d, n = rays["direction"][hit, :3].astype(np.float64), plain["normal"][hit, :3].astype(np.float64)
    r = d - 2.0 * (d * n).sum(axis=1, keepdims=True) * n
    got = plain["reflected"]["direction"][hit, :3].astype(np.float64)
    # (fp32 roundings, in units of 2^-24 |d|: three products and two sums of the dot <= 5, doubled by the -2; the product with n <= 2,
    #  the final sum <= 3 - 15 in all, under 8 * 2^-23)
    assert (np.abs(got - r) <= 8 * U * np.linalg.norm(d, axis=1, keepdims=True)).all()
    assert_zero_records(plain, ~hit, "misses")


# ---- 4. conditions on the inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_the_cloud_rays_meet_spheres_boxes_and_nothing(seed):
    objs, rays = cloud(), cloud_rays(1000, seed)
    _, index = backend(objs, rays).query_closest(rays)
    kind = objs["type"][np.maximum(index, 0)]
    spheres, boxes, misses = int(((index >= 0) & (kind == R.SPHERE)).sum()), int(((index >= 0) & (kind == R.BOX)).sum()), int((index < 0).sum())
    assert spheres >= 100 and boxes >= 50 and misses >= 100, (spheres, boxes, misses)


def test_the_tiny_far_box_has_nan_and_finite_normals():
    objs, rays = tiny_far_box()
    h = backend(objs, rays).query_hits(rays)
    hit = h["index"] >= 0
    nan_normal = np.isnan(h["normal"][:, :3]).all(axis=1)
    finite = np.isfinite(h["normal"][:, :3]).all(axis=1)
    assert (hit & nan_normal).sum() >= 16 and (hit & finite).sum() >= 16, (int((hit & nan_normal).sum()), int((hit & finite).sum()))
    assert ((nan_normal | finite)[hit]).all()
    # a NaN normal makes a NaN reflected ray (direction and start), the point stays finite
    refl = floats(h["reflected"])
    assert np.isnan(refl[hit & nan_normal][:, [0, 1, 2, 4, 5, 6]]).all() and np.isfinite(h["point"][hit]).all()
    # hits.hit_records has both kinds too (not on the same rays: the object-space point rounds differently without contraction)
    plain = HT.hit_records(objs, rays, h["t"], h["index"])
    plain_nan = np.isnan(plain["normal"][:, :3]).all(axis=1)
    assert (hit & plain_nan).sum() >= 16 and (hit & ~plain_nan).sum() >= 16


# ---- 5. names ----------------------------------------------------------------------------------------------------------------------
def test_names():
    from opencl_raytracer_amd import hip_raytracer
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert "dlsym of rt_query_hits_device" in header and "hit-record queries" in header
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in hip_raytracer.EXPORTS
    assert re.search(r"typedef struct rt_hits_t \{[^}]*float\*\s+t;[^}]*int32_t\*\s+index;[^}]*float\*\s+point;[^}]*float\*\s+normal;"
                     r"[^}]*void\*\s+reflected;[^}]*\} rt_hits_t;", header)
    assert ctypes.sizeof(hip_raytracer.RTHits) == 5 * ctypes.sizeof(ctypes.c_void_p)
    for method in ("query_hits", "pick_hit"):
        assert callable(getattr(hip_raytracer.HIPRaytracer, method)) and callable(getattr(hip_raytracer.MultiHIPRaytracer, method))
    assert callable(CPURaytracer.query_hits) and callable(CPURaytracer.hit_records)
    hpp = (ROOT / "opencl-raytracer_amd" / "host" / "HIPRaytracer.hpp").read_text()
    cpu_hpp = (ROOT / "opencl-raytracer_amd" / "host" / "CPURaytracer.hpp").read_text()
    assert "QueryHits" in hpp and "PickHit" in hpp and "QueryHits" in cpu_hpp and "HitRecords" in cpu_hpp
    assert "hip_raytracer_host_hits_test" in (ROOT / "opencl-raytracer_amd" / "host" / "Makefile").read_text()


def test_the_library_exports_the_entry_points():
    from opencl_raytracer_amd import hip_raytracer
    if not hip_raytracer.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = hip_raytracer.load_library()   # dlopen + declarations: needs no GPU
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rt_query_hits(None, None, 0, None, None) == -1   # a NULL context: RT_ERR_INVALID_ARGUMENT, nothing dereferenced
    assert lib.rt_query_hits_device(None, None, 0, None, None, None) == -1 and lib.rt_query_primary_hits(None, None, 0, None) == -1


# ---- 6. scene_tool pick ------------------------------------------------------------------------------------------------------------
def test_scene_tool_pick_prints_the_point_and_the_normal():
    import subprocess
    from helpers import SCENES
    from opencl_raytracer_amd import camera, scene_loader
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H = 96, 64
    scene_file = SCENES / "multipleSpheres.txt"
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    z_bits = format(int(np.float32(rays["direction"][0, 2]).view(np.uint32)), "x")
    h = CPURaytracer(objs, lts, rays[:1], 0, kernel="hittest").query_hits(rays)
    for i, j in ((48, 32), (0, 0)):   # a hit and a miss
        res = subprocess.run([str(tool), "pick", str(scene_file), str(W), str(H), str(i), str(j), "cpu", z_bits], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        point, normal, pick = (l.split() for l in res.stdout.strip().splitlines()[-3:])
        k = j * W + i
        assert point[0] == "point" and normal[0] == "normal" and pick[0] == "pick" and int(pick[1]) == h["index"][k]
        assert np.array_equal(np.array(point[1:], dtype=F), h["point"][k]) and np.array_equal(np.array(normal[1:], dtype=F), h["normal"][k, :3])
    assert h["index"][32 * W + 48] >= 0 and h["index"][0] == -1
