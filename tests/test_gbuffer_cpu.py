"""CPU: G-buffer frames (hip_raytracer.h, "G-buffer frames") without a GPU.

1. CPURaytracer.render_gbuffer is CPURaytracer.query_hits over the same primary rays plus the diffuse lookup, through the setters;
   it equals hits.hit_records where that is bit-defined (an axis-aligned scale-and-translate scene: every product with a zero is
   exact, so contraction changes nothing there but the last step, which is compared on the stable rays only).
2. the type-2 branch of hits.hit_records on hand-made triangle hits: the point is t d + s - one rounding of the exact value under the
   fused definition, product then sum under the unfused one - and the normal is a unit vector orthogonal to both edges.
3. names: the struct layouts, the three symbols of the built library, the fronts. These fail before the feature."""
import ctypes
import re
from fractions import Fraction
from pathlib import Path

import numpy as np

from helpers import R, random_scene
from opencl_raytracer_amd import hits as HT
from opencl_raytracer_amd import rays as RY
from opencl_raytracer_amd import tessellate
from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
from test_query_hits_cpu import cloud, cloud_rays

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
U = 2.0 ** -23
NAMES = ("rt_render_gbuffer_device", "rt_render_gbuffer", "rt_get_gbuffer_info")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def word(x) -> int:
    return int(np.float32(x).view(np.uint32))


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def lights_of(objs):
    return random_scene(1, 1, 2, seed=5)[1]


def expected_albedo(materials, index):
    want = np.zeros((len(index), 4), dtype=F)
    hit = index >= 0
    want[hit, :3] = materials["diffuse"][index[hit]][:, :3]
    want[hit, 3] = 1.0
    return want


# ---- 1. the CPU backend ------------------------------------------------------------------------------------------------------------
def test_cpu_render_gbuffer_is_query_hits_plus_the_diffuse_lookup():
    objs, rays = cloud(), cloud_rays(600, 3)
    cpu = CPURaytracer(objs, lights_of(objs), rays, 0, kernel="hittest")
    g, h = cpu.render_gbuffer(), cpu.query_hits(rays)
    assert list(g) == ["t", "index", "point", "normal", "albedo"]
    for k in ("t", "index", "point", "normal"):
        assert same_bits_or_nan(g[k].astype(F), h[k].astype(F)) if k != "index" else np.array_equal(g[k], h[k]), k
    hit = g["index"] >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 100
    assert np.array_equal(bits(g["albedo"]), bits(expected_albedo(R.materials_of(objs), g["index"])))
    assert not bits(g["albedo"][~hit]).any() and not bits(g["point"][~hit]).any() and not bits(g["normal"][~hit]).any()


def test_cpu_render_gbuffer_follows_the_setters():
    objs, rays = cloud(), cloud_rays(400, 4)
    cpu = CPURaytracer(objs, lights_of(objs), rays, 0, kernel="shade_and_reflect")
    before = cpu.render_gbuffer()
    # new colours (a NaN and an inf among them: moved, not computed with), half of the objects hidden, other rays
    mats = R.materials_of(objs)
    mats["diffuse"][:, :3] = np.linspace(0.0, 1.0, 3 * len(objs), dtype=F).reshape(-1, 3)
    winner = int(before["index"][before["index"] >= 0][0])
    mats["diffuse"][winner, 0] = np.nan
    mats["diffuse"][winner, 1] = np.inf
    cpu.set_materials(mats)
    recoloured = cpu.render_gbuffer()
    assert np.array_equal(recoloured["index"], before["index"]) and same_bits_or_nan(recoloured["point"], before["point"])
    assert same_bits_or_nan(recoloured["albedo"], expected_albedo(mats, recoloured["index"]))
    assert np.isnan(recoloured["albedo"][recoloured["index"] == winner, 0]).all()
    visible = (np.arange(len(objs)) % 2).astype(np.uint8)
    visible[winner] = 0
    cpu.set_visibility(visible)
    masked = cpu.render_gbuffer()
    assert not np.isin(masked["index"][masked["index"] >= 0], np.nonzero(visible == 0)[0]).any()
    assert not np.array_equal(masked["index"], before["index"])
    other = cloud_rays(400, 9)
    cpu.set_rays(other)
    h = cpu.query_hits(other)
    g = cpu.render_gbuffer()
    assert np.array_equal(g["index"], h["index"]) and same_bits_or_nan(g["normal"], h["normal"]) and same_bits_or_nan(g["t"], h["t"])
    # a pose: the rays are rays.posed_rays'
    W, H = 20, 20
    cpu.set_pose(W, H, -30.0, np.eye(3), (0.1, 0.2, 0.3))
    posed = RY.posed_rays(W, H, -30.0, np.eye(3), (0.1, 0.2, 0.3))
    assert np.array_equal(cpu.render_gbuffer()["index"], cpu.query_hits(posed)["index"])


def diagonal_scene():
    """Spheres and boxes scaled and translated by powers of two and small integers: mv and mvInverse have exact entries and zeros off
    the diagonal."""
    objs, _ = random_scene(6, 6, 1, seed=11)
    for k in range(len(objs)):
        s = [0.5, 1.0, 2.0][k % 3]
        c = np.array([(k % 4) * 2.0 - 3.0, (k // 4) * 2.0 - 2.0, -12.0 - (k % 3)], dtype=np.float64)
        mv = np.diag([s, s, s, 1.0])
        mv[:3, 3] = c
        inv = np.diag([1 / s, 1 / s, 1 / s, 1.0])
        inv[:3, 3] = -c / s
        objs["mv"][k] = mv.T.reshape(16).astype(F)
        objs["mvInverse"][k] = inv.T.reshape(16).astype(F)
        objs["mvInverseTranspose"][k] = inv.reshape(16).astype(F)
    return objs


def test_cpu_render_gbuffer_against_hits_hit_records_where_that_is_bit_defined():
    """(t, index) are the backend's; the record stage of hits.hit_records at those is product-then-sum throughout, the backend's
    contracts. On this scene every product but t * d' is exact (scales are powers of two, centres small integers, the rays start at
    the origin), so the two stages differ in ONE step: the object-space point t d' + s', one rounding in the backend, two in
    hits.hit_records. Where those agree - decided here from the exact value of t d' + s' - the point is bit-defined, and the records
    are compared bit for bit; everywhere they agree to a few units of 2^-23 of the scene's scale, and bit for bit on w, on the zero
    records and on the axis-aligned box normals."""
    objs = diagonal_scene()
    rng = np.random.default_rng(2)
    rays = np.zeros(8000, dtype=R.RAY_DTYPE)
    rays["start"][:, 3] = 1.0
    rays["direction"][:, :3] = np.stack([rng.uniform(-6, 6, 8000), rng.uniform(-5, 5, 8000), np.full(8000, -12.0)], axis=1).astype(F)
    cpu = CPURaytracer(objs, lights_of(objs), rays, 0, kernel="hittest")
    g = cpu.render_gbuffer()
    want = HT.hit_records(objs, rays, g["t"], g["index"])
    hit = g["index"] >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 50
    assert np.array_equal(bits(g["point"][:, 3]), bits(want["point"][:, 3]))
    assert not bits(g["point"][~hit]).any() and not bits(want["point"][~hit]).any()
    scale = 16.0
    assert np.abs(g["point"][hit, :3].astype(np.float64) - want["point"][hit, :3]).max() <= 8 * U * scale
    # the one step that differs, per component: fl(t d' + s') against fl(fl(t d') + s')
    o = objs[np.maximum(g["index"], 0)]
    inv = o["mvInverse"].reshape(-1, 16).astype(F)
    defined = hit.copy()
    for c in range(3):
        d_obj = (inv[:, 5 * c] * rays["direction"][:, c]).astype(F)          # a power of two times d: exact
        s_obj = inv[:, 12 + c]
        with np.errstate(all="ignore"):
            defined &= bits(HT._fma(g["t"], d_obj, s_obj)) == bits((g["t"] * d_obj).astype(F) + s_obj)
    assert defined.sum() >= 50 and (hit & ~defined).sum() >= 20              # both kinds of ray are in the batch
    assert np.array_equal(bits(g["point"][defined]), bits(want["point"][defined]))
    assert not np.array_equal(bits(g["point"][hit]), bits(want["point"][hit]))   # ... and the other rays do tell the two stages apart
    box = hit & (objs["type"][np.maximum(g["index"], 0)] == R.BOX)
    axis = box & (np.abs(want["normal"][:, :3]).sum(axis=1) == 1.0) & (np.abs(g["normal"][:, :3]).sum(axis=1) == 1.0)
    assert axis.sum() >= 20
    assert np.array_equal(bits(g["normal"][axis]), bits(want["normal"][axis]))


# ---- 2. the type-2 branch of hits.hit_records ------------------------------------------------------------------------------------------
def hand_made_triangles():
    v0 = np.array([[0.0, 0.0, -5.0], [1.25, -2.5, -9.0], [-3.0, 0.7, -20.0], [0.1, 0.2, -0.3], [100.0, -50.0, -400.0]])
    v1 = v0 + np.array([[1.0, 0.0, 0.0], [0.3, 1.7, -0.2], [2.0, 0.1, 3.0], [1e-3, 0.0, 2e-3], [7.0, 11.0, -13.0]])
    v2 = v0 + np.array([[0.0, 1.0, 0.0], [-1.1, 0.4, 0.9], [0.0, 5.0, 0.5], [0.0, 3e-3, 1e-3], [-5.0, 2.0, 17.0]])
    template = random_scene(1, 0, 1, seed=1)[0][0]
    return tessellate.triangle_records(v0, v1, v2, template)


def triangle_hits(seed=7):
    """Rays from (near) the origin to random points inside each hand-made triangle, with a time that is no round number."""
    tris = hand_made_triangles()
    v0, e1, e2 = (a.astype(np.float64) for a in HT.triangle_edges(tris))
    rng = np.random.default_rng(seed)
    n = 40
    index = (np.arange(n) % len(tris)).astype(np.int32)
    a, b = rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n)
    target = v0[index] + a[:, None] * e1[index] + b[:, None] * e2[index]
    rays = np.zeros(n, dtype=R.RAY_DTYPE)
    rays["start"][:, :3] = rng.uniform(-0.5, 0.5, (n, 3)).astype(F)
    rays["start"][:, 3] = 1.0
    t = rng.uniform(0.3, 3.0, n).astype(F)
    rays["direction"][:, :3] = ((target - rays["start"][:, :3]) / t[:, None].astype(np.float64)).astype(F)
    index[::8] = -1    # a few misses among them
    return tris, rays, t, index


def round_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the exact rational x, ties to even (normal range)."""
    if x == 0:
        return F(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = 0
    while a >= 2 ** 24:
        a, e = a / 2, e + 1
    while a < 2 ** 23:
        a, e = a * 2, e - 1
    m, frac = a.numerator // a.denominator, a - a.numerator // a.denominator
    if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return F(sign * float(Fraction(m) * Fraction(2) ** e))


def test_triangle_point_is_the_single_rounded_t_d_plus_s_under_the_fused_definition():
    tris, rays, t, index = triangle_hits()
    fused = HT.hit_records(tris, rays, t, index, fused=True)
    plain = HT.hit_records(tris, rays, t, index)
    hit = np.nonzero(index >= 0)[0]
    differs = 0
    for i in hit:
        for c in range(4):
            s, d = rays["start"][i, c], rays["direction"][i, c]
            exact = Fraction(float(t[i])) * Fraction(float(d)) + Fraction(float(s))
            assert word(fused["point"][i, c]) == word(round_to_f32(exact)), (i, c)
            two_steps = F(F(t[i] * d) + s)
            assert word(plain["point"][i, c]) == word(two_steps), (i, c)
            differs += int(word(two_steps) != word(round_to_f32(exact)))
    assert differs >= 5            # the two definitions are told apart by these hits
    assert (fused["point"][hit, 3] == 1.0).all()
    miss = index < 0
    assert miss.sum() >= 4
    for rec in (fused, plain):
        assert not bits(rec["point"][miss]).any() and not bits(rec["normal"][miss]).any()
    # `fused` contracts nothing of the normal
    assert np.array_equal(bits(fused["normal"]), bits(plain["normal"]))


def test_triangle_normal_is_a_unit_vector_orthogonal_to_both_edges():
    tris, rays, t, index = triangle_hits()
    rec = HT.hit_records(tris, rays, t, index)
    _, e1, e2 = (a.astype(np.float64) for a in HT.triangle_edges(tris))
    for i in np.nonzero(index >= 0)[0]:
        n = rec["normal"][i, :3].astype(np.float64)
        a, b = e1[index[i]], e2[index[i]]
        # the normalisation's own rounding: three squares, two sums, a root and a quotient, each within 2^-24 relative - under 4 * 2^-23
        assert abs(np.linalg.norm(n) - 1.0) <= 4 * U, i
        # each cross-product component is a difference of two rounded products: its error is at most 2^-23 of |a| |b|, which
        # turns n by at most 3 * 2^-23 |a||b| / |a x b|; the normalisation adds 4 * 2^-23
        tilt = (3 * U * np.linalg.norm(a) * np.linalg.norm(b) / np.linalg.norm(np.cross(a, b)) + 4 * U)
        assert abs(n @ a) <= tilt * np.linalg.norm(a) and abs(n @ b) <= tilt * np.linalg.norm(b), i
        assert n @ np.cross(a, b) > 0 and rec["normal"][i, 3] == 0.0
    # the executable definition's own steps, one IEEE operation each
    k = int(np.nonzero(index >= 0)[0][0])
    a, b = HT.triangle_edges(tris)[1][index[k]], HT.triangle_edges(tris)[2][index[k]]
    nx = F(F(a[1] * b[2]) - F(a[2] * b[1]))
    ny = F(F(a[2] * b[0]) - F(a[0] * b[2]))
    nz = F(F(a[0] * b[1]) - F(a[1] * b[0]))
    length = np.sqrt(F(F(F(nx * nx) + F(ny * ny)) + F(nz * nz)))
    assert np.array_equal(bits(rec["normal"][k, :3]), bits(np.array([nx / length, ny / length, nz / length], dtype=F)))


# ---- 3. names ----------------------------------------------------------------------------------------------------------------------
def test_struct_layouts():
    from opencl_raytracer_amd import hip_raytracer as hr
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    assert re.search(r"typedef struct rt_gbuffer_t \{[^}]*float\*\s+t;[^}]*int32_t\*\s+index;[^}]*float\*\s+point;[^}]*float\*\s+normal;"
                     r"[^}]*float\*\s+albedo;[^}]*\} rt_gbuffer_t;", header)
    assert re.search(r"typedef struct rt_gbuffer_info_t \{[^}]*uint64_t\s+n_items,\s*hits;[^}]*double\s+trace_ms,\s*records_ms;"
                     r"[^}]*uint32_t\s+wavefront,\s*reserved;[^}]*\} rt_gbuffer_info_t;", header)
    assert ctypes.sizeof(hr.RTGBuffer) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in hr.RTGBuffer._fields_] == list(hr.GBUFFER_FIELDS) == ["t", "index", "point", "normal", "albedo"]
    assert ctypes.sizeof(hr.RTGBufferInfo) == 40
    assert [(n, getattr(hr.RTGBufferInfo, n).offset) for n, _ in hr.RTGBufferInfo._fields_] == \
        [("n_items", 0), ("hits", 8), ("trace_ms", 16), ("records_ms", 24), ("wavefront", 32), ("reserved", 36)]


def test_the_built_library_exports_the_three_symbols():
    from opencl_raytracer_amd import hip_raytracer as hr
    if not hr.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(str(hr.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), name
    # NULL context: refused before anything is touched (needs no GPU)
    lib.rt_render_gbuffer.restype = lib.rt_render_gbuffer_device.restype = lib.rt_get_gbuffer_info.restype = ctypes.c_int
    lib.rt_render_gbuffer.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.rt_render_gbuffer_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.rt_get_gbuffer_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.rt_render_gbuffer(None, None) == -1 and lib.rt_render_gbuffer_device(None, None, None) == -1
    assert lib.rt_get_gbuffer_info(None, None) == -1


def test_names():
    from opencl_raytracer_amd import distributed, hip_raytracer as hr
    header = (ROOT / "include" / "hip_raytracer.h").read_text()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", header)
    assert "dlsym of rt_render_gbuffer_device" in header and "G-buffer frames" in header
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in hr.EXPORTS
    assert callable(hr.HIPRaytracer.render_gbuffer) and callable(hr.HIPRaytracer.gbuffer_info)
    assert callable(distributed.ShardedHIPRaytracer.render_gbuffer) and callable(CPURaytracer.render_gbuffer)
    host = ROOT / "opencl-raytracer_amd" / "host"
    assert "RenderGBuffer" in (host / "HIPRaytracer.hpp").read_text() and "GBufferInfo" in (host / "HIPRaytracer.hpp").read_text()
    assert "RenderGBuffer" in (host / "CPURaytracer.hpp").read_text()
    assert "hip_raytracer_host_gbuffer_test" in (host / "Makefile").read_text()
    csrc = (ROOT / "opencl-raytracer_amd" / "csrc" / "Makefile").read_text()
    assert csrc.count("rt_gbuffer.hip") >= 2 and "rt_gbuffer.o" in csrc and "rt_gbuffer.h" in csrc
    assert "gbuffer" in (host / "scene_tool.cpp").read_text()


def test_scene_tool_gbuffer_writes_the_two_pictures(tmp_path):
    """scene_tool gbuffer on the CPU backend: both files are ppm.format_p6 of the records CPURaytracer.render_gbuffer gives for the
    same grid - normals as 0.5 n + 0.5, depth as t over the largest finite t, a miss black."""
    import subprocess
    from helpers import SCENES
    from opencl_raytracer_amd import camera, ppm, scene_loader
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    W, H = 48, 32
    scene_file = SCENES / "multipleSpheres.txt"
    z = F(-H)
    res = subprocess.run([str(tool), "gbuffer", str(scene_file), str(W), str(H), str(tmp_path / "gb"), "cpu", f"{word(z):08x}"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    objs, lts = scene_loader.load_scene(str(scene_file))
    rays = camera.primary_rays(W, H)
    rays["direction"][..., 2] = z
    g = CPURaytracer(objs, lts, rays, 0, kernel="hittest").render_gbuffer()
    hit = g["index"] >= 0
    assert 0 < hit.sum() < W * H and res.stdout.strip().splitlines()[-1].startswith(f"gbuffer {int(hit.sum())} hits of {W * H}")
    normal = np.where(hit[:, None], F(0.5) * g["normal"][:, :3] + F(0.5), F(0.0)).astype(F)
    t_max = g["t"][hit & np.isfinite(g["t"])].max()
    with np.errstate(over="ignore"):
        depth = np.where(hit, g["t"] / t_max, F(0.0)).astype(F)
    assert (tmp_path / "gb_normal.ppm").read_bytes() == ppm.format_p6(W, H, normal)
    assert (tmp_path / "gb_depth.ppm").read_bytes() == ppm.format_p6(W, H, np.repeat(depth[:, None], 3, axis=1))
