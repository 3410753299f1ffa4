"""No GPU: the ray populations and gate cases that tests/test_live_grid_gpu.py gives to a LIVE context - a context whose grid was
built for other rays ("which box the radii are built for") - and the conditions under which they test something.

`population(kind, lo, hi, objs, n, seed)` fills the box lo..hi (on the GPU: rays_info()["box_lo"/"box_hi"] of the live context; here
an approximation of it, `approx_box`) with n rays; every start is rounded to float32 INWARDS, because the double of a face usually
rounds out of the box, and the gate compares doubles. `gate_cases(lo, hi, n)` moves one ray of a buffer that lies strictly inside
onto the last float32 inside each face and onto the first one beyond it. The conditions (no NaN time, hit share, miss share, rays
per pixel) come from the oracle alone: they are conditions on the inputs, not measurements of the HIP path. No population keeps its
starts out of the objects: the two that the GPU file also holds to the oracle (`fill_aimed`, `corners_aimed`) met its bars with the
starts that lie inside objects included, so there is no such input condition."""
import functools

import numpy as np
import pytest

from helpers import R, random_scene
from opencl_raytracer_amd import rays as RY
from test_frame_shapes_cpu import DEPTH, _behind_and_across, camera_z_for, pinhole_rays, scene
from test_set_rays_cpu import tri_box

F = np.float32
N = 96 * 96
KINDS = ("fill_random", "fill_aimed", "corners_aimed", "axis_parallel", "on_surfaces")
ORACLE_KINDS = ("fill_aimed", "corners_aimed")
LIVE_SCENES = ("s300", "s608", "tri")
MIN_HIT_SHARE, MIN_MISS_SHARE, MIN_RAYS_PER_PIXEL = 0.15, 0.01, 2.0
LENGTHS = (1e-2, 1.0, 50.0)
SCAN_TRIP = 1024 * 256          # csrc/rt_rays.hip: kScanMaxBlocks * kScanBlock rays per trip of the scan's grid-stride loop
GATE_PLACES = (0, 63, 64, -1)   # the moved ray, face by face (-1: the last ray)
FAR = 200.0                     # context B's creation rays start up to this far out

# aim offsets in units of the target's smallest extent: 0 goes through the centre, 0.5 and 1 graze the body, the rest pass the
# narrow side and meet what lies behind or nothing. The last entries are the tuning the conditions asked for: with (0, 0.5, 1, 2)
# alone the aimed populations of the dense scenes miss too rarely.
AIM_OFFSETS = (0.0, 0.5, 1.0, 2.0, 0.5, 1.0, 2.0, 6.0)


@functools.lru_cache(maxsize=None)
def live_scene(name):
    """s300 and tri of test_frame_shapes_cpu, and s608: the other side of kWavefrontMinObjects = 512 (rt_context.h), where an
    off-grid frame stays on the large-scene kernels."""
    if name != "s608":
        return scene(name)
    objs, lights = random_scene(400, 200, 3, seed=17, spread=8.0, zrange=(-40, -8))
    objs = np.concatenate([objs, _behind_and_across(104)])
    assert len(objs) == 608
    return objs, lights


def bodies(objs):
    """Per object in float64: centre (n, 3), smallest extent (n,), bounding radius (n,), the 3 x 3 instance matrix (n, 3, 3; the
    identity for a triangle) and whether it is a sphere. A triangle (type 2, tessellate.py) is its guard sphere."""
    n = len(objs)
    mv = objs["mv"].reshape(n, 4, 4).astype(np.float64).transpose(0, 2, 1)   # column-major storage
    A = mv[:, :3, :3].copy()
    centre = mv[:, :3, 3].copy()
    sv = np.linalg.svd(A, compute_uv=False)
    box = objs["type"] == R.BOX
    small = sv.min(axis=1) * np.where(box, 0.5, 1.0)
    radius = sv.max(axis=1) * np.where(box, np.sqrt(0.75), 1.0)
    tri = objs["type"] > R.BOX
    if tri.any():
        guard = objs["mvInverse"].reshape(n, 16)[:, :4].astype(np.float64)
        centre[tri], small[tri], radius[tri] = guard[tri, :3], guard[tri, 3], guard[tri, 3]
        A[tri] = np.eye(3)
    return centre, small, radius, A, objs["type"] == R.SPHERE


def approx_box(name):
    """About the box build_grid keeps for a context created with a camera: the origin united with every centre +- 1.01 R. Only the
    conditions of this file use it; the GPU tests read the library's own box."""
    if name == "tri":
        return tri_box()
    centre, _, radius, _, _ = bodies(live_scene(name)[0])
    return np.minimum(0.0, (centre - 1.01 * radius[:, None]).min(0)), np.maximum(0.0, (centre + 1.01 * radius[:, None]).max(0))


def inward(x, lo, hi):
    """float64 points -> float32, no coordinate outside lo..hi: clipped, rounded, and stepped one float32 towards the interior
    where rounding left the box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    f = np.clip(np.asarray(x, np.float64), lo, hi).astype(F)
    f = np.where(f.astype(np.float64) < lo, np.nextafter(f, F(np.inf)), f)
    f = np.where(f.astype(np.float64) > hi, np.nextafter(f, F(-np.inf)), f)
    assert ((f.astype(np.float64) >= lo) & (f.astype(np.float64) <= hi)).all()
    return f


def inside_an_object(starts, objs):
    """Per start: does it lie inside (or within 1 % of) some object's bounding sphere?"""
    centre, _, radius, _, _ = bodies(objs)
    s = np.asarray(starts, np.float64)[:, :3]
    out = np.zeros(len(s), bool)
    for k in range(0, len(s), 1024):
        d = np.linalg.norm(s[k:k + 1024, None, :] - centre[None], axis=2)
        out[k:k + 1024] = (d <= 1.01 * radius[None]).any(axis=1)
    return out


def cell_edges(lo, hi, n_objs):
    """build_grid's cell edge (rt_scene.cpp) and its refinements by 0.7: about three cells per object, at most 256 per axis."""
    ext = np.maximum(np.asarray(hi, np.float64) - np.asarray(lo, np.float64), 1e-6)
    cell = max(float(np.cbrt(ext.prod() / (3.0 * n_objs))), float(ext.max()) / 256.0)
    return [cell * 0.7 ** k for k in range(4)]


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _as_rays(starts, directions):
    rays = np.zeros(len(starts), dtype=R.RAY_DTYPE)
    rays["start"][:, :3] = starts
    rays["start"][:, 3] = 1.0
    rays["direction"][:, :3] = np.asarray(directions, np.float64).astype(F)
    return rays


def box_marks(lo, hi):
    """The eight corners, twelve edge midpoints and six face centres of a box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pts = [lo + np.array([i, j, k]) / 2.0 * (hi - lo) for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)]
    assert len(pts) == 26
    return np.array(pts)


def population(kind, lo, hi, objs, n, seed):
    """n rays with start.w = 1, direction.w = 0 and every start inside lo..hi (asserted in float64)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rng = np.random.default_rng(seed)
    centre, small, _, A, is_sphere = bodies(objs)
    k = np.arange(n)
    if kind == "corners_aimed":
        starts = box_marks(lo, hi)[k % 26]
    elif kind == "on_surfaces":
        j = rng.integers(0, len(objs), n)
        u = _unit(rng, n)
        # even rays: inside the object, up to half its smallest extent from the centre (a triangle: about its guard centre)
        starts = centre[j] + u * (rng.uniform(0.0, 0.5, n) * small[j])[:, None]
        spheres = np.flatnonzero(is_sphere)
        if len(spheres):   # odd rays: on a sphere's surface, then -4 .. +4 float32 steps along the axis the normal leans on most
            js = spheres[rng.integers(0, len(spheres), n)]
            surf = (centre[js] + np.einsum("nij,nj->ni", A[js], u)).astype(F)
            axis = np.abs(surf.astype(np.float64) - centre[js]).argmax(axis=1)
            steps = (k // 2) % 9 - 4
            for s in range(1, 5):
                for sign in (-1, 1):
                    rows = np.flatnonzero(steps == sign * s)
                    col = surf[rows, axis[rows]]
                    for _ in range(s):
                        col = np.nextafter(col, F(sign * np.inf))
                    surf[rows, axis[rows]] = col
            odd = (k % 2) == 1
            starts[odd] = surf[odd].astype(np.float64)
    else:
        starts = rng.uniform(lo, hi, size=(n, 3))
    if kind == "axis_parallel":   # every fourth start on whole cells from box_lo, for each candidate cell edge in turn
        cells = cell_edges(lo, hi, len(objs))
        rows = np.flatnonzero(k % 4 == 0)
        edge = np.array(cells)[(rows // 4) % len(cells)][:, None]
        starts[rows] = lo + np.floor((starts[rows] - lo) / edge) * edge
    starts = inward(starts, lo, hi)
    length = np.array(LENGTHS)[k % 3]
    if kind in ("fill_aimed", "corners_aimed"):
        j = rng.integers(0, len(objs), n)
        off = np.array(AIM_OFFSETS)[(k // 3) % len(AIM_OFFSETS)]
        d = centre[j] + _unit(rng, n) * (off * small[j])[:, None] - starts.astype(np.float64)
        d[np.linalg.norm(d, axis=1) < 1e-3] = (0.0, 0.0, -1.0)
        d *= np.array([0.5, 1.0, 2.0])[k % 3][:, None]   # the aimed point at t = 2, 1, 0.5
    elif kind == "axis_parallel":
        d = np.zeros((n, 3))
        d[k, (k // 6) % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0) * length
    else:
        d = _unit(rng, n) * length[:, None]
    return _as_rays(starts, d)


def far_creation_rays(objs, n, seed=29):
    """Context B is created from these: starts up to FAR units out (the first eight at the corners of that cube), aimed at the
    objects - its radii are built for a D and an S_max of a few hundred units."""
    cube = (np.full(3, -FAR), np.full(3, FAR))
    rays = population("fill_aimed", *cube, objs, n, seed)
    rays["start"][:8, :3] = box_marks(*cube)[[0, 2, 6, 8, 17, 19, 23, 25]].astype(F)
    assert np.array_equal(np.abs(rays["start"][:8, :3]), np.full((8, 3), F(FAR)))
    return rays


# ---- the gate's cases ---------------------------------------------------------------------------------------------------
def last_inside(face, side):
    """The largest (side "hi") or smallest ("lo") float32 that is not beyond the face, a double."""
    f = F(face)
    if side == "hi" and float(f) > face:
        f = np.nextafter(f, F(-np.inf))
    if side == "lo" and float(f) < face:
        f = np.nextafter(f, F(np.inf))
    return f


def first_outside(face, side):
    return np.nextafter(last_inside(face, side), F(np.inf if side == "hi" else -np.inf))


def gate_base(lo, hi, n, seed=53):
    """Strictly inside: starts in the middle half of the box, directions of the three lengths."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rng = np.random.default_rng(seed)
    starts = inward(rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(n, 3)), lo, hi)
    s = starts.astype(np.float64)
    assert ((s > lo) & (s < hi)).all()
    return _as_rays(starts, _unit(rng, n) * np.array(LENGTHS)[np.arange(n) % 3][:, None])


def gate_faces():
    return [(axis, side) for axis in range(3) for side in ("lo", "hi")]


def gate_cases(lo, hi, n):
    """[(label, rays, expected_inside)]. Per face "x.lo" .. "z.hi" the pair `face F inside, ray K` / `face F outside, ray K`: ray K
    of the base buffer with ONE coordinate on the last float32 inside the face, or on the next one; K goes through GATE_PLACES
    face by face. With n > SCAN_TRIP only the y.hi pair, at a ray of the scan's second grid-stride trip. Then -0.0 on every face
    that is 0, and two rays outside on different axes."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    base = gate_base(lo, hi, n)
    cases = []
    big = n > SCAN_TRIP
    for f, (axis, side) in enumerate(gate_faces()):
        if big and (axis, side) != (1, "hi"):
            continue
        at = SCAN_TRIP + 77 if big else GATE_PLACES[f % len(GATE_PLACES)] % n
        face = float((lo if side == "lo" else hi)[axis])
        for inside, value in ((True, last_inside(face, side)), (False, first_outside(face, side))):
            rays = base.copy()
            rays["start"][at, axis] = value
            cases.append((f"face {'xyz'[axis]}.{side} {'inside' if inside else 'outside'}, ray {at}", rays, inside))
        if face == 0.0 and not big:
            rays = base.copy()
            rays["start"][n // 2, axis] = F(-0.0)
            cases.append((f"-0.0 on face {'xyz'[axis]}.{side}, ray {n // 2}", rays, True))
    if not big:
        rays = base.copy()
        rays["start"][0, 0] = first_outside(float(hi[0]), "hi")
        rays["start"][n - 1, 1] = first_outside(float(lo[1]), "lo")
        cases.append((f"two rays outside: x.hi at ray 0, y.lo at ray {n - 1}", rays, False))
    return cases


def check_gate_cases(lo, hi, n, cases):
    """Every case is what its label says: ray_verdict reports the moved ray as the extreme of its axis, the expectation follows from
    the verdict's box and lo..hi as doubles, and the two cases of a face differ in exactly one float32 of one ray."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    by_face = {}
    for label, rays, expected in cases:
        v = RY.ray_verdict(rays)
        assert v["dir_w_zero"] and v["directions_in_domain"] and v["starts_ok"], label
        vlo, vhi = v["origin_lo"].astype(np.float64), v["origin_hi"].astype(np.float64)
        assert bool((vlo >= lo).all() and (vhi <= hi).all()) == expected, label
        if label.startswith("face "):
            face, kind = label.split()[1], label.split()[2].rstrip(",")
            axis, side, at = "xyz".index(face[0]), face[2:], int(label.rsplit(" ", 1)[1])
            assert (v["origin_lo"] if side == "lo" else v["origin_hi"])[axis] == rays["start"][at, axis], label
            others = np.delete(rays["start"][:, axis], at)
            assert rays["start"][at, axis] < others.min() if side == "lo" else rays["start"][at, axis] > others.max(), label
            by_face.setdefault(face, {})[kind] = rays
        elif label.startswith("-0.0"):
            face, at = label.split()[3].rstrip(","), int(label.rsplit(" ", 1)[1])
            axis = "xyz".index(face[0])
            assert np.signbit(rays["start"][at, axis]) and rays["start"][at, axis] == 0, label
            assert (v["origin_lo"] if face[2:] == "lo" else v["origin_hi"])[axis] == 0, label   # the extreme, as a NUMBER
    for face, pair in by_face.items():
        a, b = pair["inside"].view(np.uint32), pair["outside"].view(np.uint32)
        assert int((a != b).sum()) == 1, face
        word = int(np.flatnonzero((a != b).reshape(-1))[0])
        x, y = pair["inside"].view(F).reshape(-1)[word], pair["outside"].view(F).reshape(-1)[word]
        assert np.nextafter(x, y) == y, f"{face}: not neighbouring float32"
    return by_face


def sees_the_scene(want, n, kernel, label):
    """The conditions of this file on an oracle result; returns (hit share, rays per pixel)."""
    assert not np.isnan(want["hit_t"]).any(), f"{label}: the oracle reports a NaN time"
    hit = float((want["hit_index"] >= 0).mean())
    per_pixel = want["rays_ref"] / n
    assert hit >= MIN_HIT_SHARE and 1.0 - hit >= MIN_MISS_SHARE, (label, hit)
    if kernel == "shade_and_reflect":
        assert per_pixel >= MIN_RAYS_PER_PIXEL, (label, per_pixel)
    return hit, per_pixel


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_s608_lies_beyond_the_brute_force_threshold():
    objs, lights = live_scene("s608")
    assert len(objs) == 608 >= 512 and len(lights) == 3 and set(objs["type"]) == {R.SPHERE, R.BOX}
    lo, hi = approx_box("s608")
    assert (lo < 0).all() and (hi > 0).all()


def test_inward_rounding_keeps_every_corner_in_the_box():
    for name in LIVE_SCENES:
        lo, hi = approx_box(name)
        marks = box_marks(lo, hi)
        plain = marks.astype(F).astype(np.float64)
        got = inward(marks, lo, hi).astype(np.float64)
        assert ((got >= lo) & (got <= hi)).all()
        assert (np.abs(got - marks) <= np.spacing(np.abs(marks).astype(F)).astype(np.float64)).all()
        if name == "tri":   # the reason for `inward`: plain rounding leaves this box
            assert ((plain < lo) | (plain > hi)).any()
    assert inward(np.array([[0.0, -0.0, 1e-50]]), np.zeros(3), np.ones(3)).tolist() == [[0.0, 0.0, 0.0]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", LIVE_SCENES)
def test_every_population_fills_the_box_and_sees_the_scene(restatement, name, kind):
    objs, lights = live_scene(name)
    lo, hi = approx_box(name)
    label = f"{name} {kind}"
    rays = population(kind, lo, hi, objs, N, seed=7)
    s = rays["start"][:, :3].astype(np.float64)
    assert len(rays) == N and ((s >= lo) & (s <= hi)).all(), label
    assert (rays["start"][:, 3] == 1).all() and (rays["direction"][:, 3] == 0).all(), label
    v = RY.ray_verdict(rays)
    assert v["dir_w_zero"] and v["directions_in_domain"] and v["starts_ok"], label
    ext = hi - lo
    if kind in ("fill_random", "fill_aimed", "axis_parallel"):   # the starts do fill the box: each axis to within 1 % of both faces
        assert ((s.min(0) - lo) < 0.01 * ext).all() and ((hi - s.max(0)) < 0.01 * ext).all(), label
    if kind == "corners_aimed":   # every corner itself, to the last float32 inside
        corner = np.array([[last_inside(float((hi if (c >> a) & 1 else lo)[a]), "hi" if (c >> a) & 1 else "lo") for a in range(3)] for c in range(8)])
        assert all((rays["start"][:, :3] == corner[c]).all(axis=1).any() for c in range(8)), label
    if kind == "axis_parallel":
        d = rays["direction"][:, :3]
        assert ((d != 0).sum(axis=1) == 1).all() and (d < 0).any() and (d > 0).any(), label
        assert {float(x) for x in np.abs(d).max(axis=1)} == {float(F(x)) for x in LENGTHS}, label
        assert (d != 0).any(axis=0).all(), label
    if kind == "on_surfaces":
        assert inside_an_object(rays["start"], objs).mean() > 0.9, label
    want = restatement[True].render("shade_and_reflect", objs, lights, rays, DEPTH)
    hit, per_pixel = sees_the_scene(want, N, "shade_and_reflect", label)
    print(f"[live grid] {label}: hit share {hit:.3f}, rays per pixel {per_pixel:.2f}")


@pytest.mark.parametrize("kind", ORACLE_KINDS)
def test_populations_of_the_far_box_see_the_scene(restatement, kind):
    """Context B (s300): the box of its creation rays, FAR units out, united with the scene's."""
    objs, lights = live_scene("s300")
    create = far_creation_rays(objs, N)
    lo, hi = approx_box("s300")
    lo, hi = np.minimum(lo, create["start"][:, :3].min(0)), np.maximum(hi, create["start"][:, :3].max(0))
    assert (lo == -FAR).all() and (hi == FAR).all()
    sees_the_scene(restatement[True].render("shade_and_reflect", objs, lights, create, DEPTH), N, "shade_and_reflect", "the creation rays")
    rays = population(kind, lo, hi, objs, N, seed=7)
    hit, per_pixel = sees_the_scene(restatement[True].render("shade_and_reflect", objs, lights, rays, DEPTH), N, "shade_and_reflect", kind)
    print(f"[live grid] s300, far box, {kind}: hit share {hit:.3f}, rays per pixel {per_pixel:.2f}")


@pytest.mark.parametrize("name", LIVE_SCENES)
def test_gate_cases_are_what_their_labels_say(name):
    lo, hi = approx_box(name)
    cases = gate_cases(lo, hi, N)
    by_face = check_gate_cases(lo, hi, N, cases)
    assert sorted(by_face) == sorted(f"{'xyz'[a]}.{s}" for a, s in gate_faces())
    zero_faces = int((lo == 0).sum() + (hi == 0).sum())
    assert len(cases) == 12 + zero_faces + 1 and (zero_faces >= 1) == (name == "tri")
    assert {int(label.rsplit(" ", 1)[1]) for label, _, _ in cases if label.startswith("face ")} == {0, 63, 64, N - 1}
    assert [e for *_, e in cases].count(False) == 7   # six faces and the two-ray case


def test_gate_cases_beyond_the_scans_first_trip():
    lo, hi = approx_box("s300")
    n = SCAN_TRIP + 1000
    cases = gate_cases(lo, hi, n)
    assert [(label, e) for label, _, e in cases] == [(f"face y.hi inside, ray {SCAN_TRIP + 77}", True), (f"face y.hi outside, ray {SCAN_TRIP + 77}", False)]
    check_gate_cases(lo, hi, n, cases)


def test_a_gate_that_forgets_a_half_passes_no_case_list():
    """The cases are only as good as what they tell apart: a gate with one comparison dropped misjudges at least one of them."""
    lo, hi = approx_box("s300")
    cases = gate_cases(lo, hi, N)

    def verdicts(gate):
        out = []
        for _, rays, _e in cases:
            v = RY.ray_verdict(rays)
            out.append(gate(v["origin_lo"].astype(np.float64), v["origin_hi"].astype(np.float64)))
        return out
    want = [e for _, _, e in cases]
    assert verdicts(lambda a, b: bool((a >= lo).all() and (b <= hi).all())) == want
    assert verdicts(lambda a, b: bool((a >= lo).all())) != want                                     # only the minima
    assert verdicts(lambda a, b: bool((b <= hi).all())) != want                                     # only the maxima
    for axis in range(3):                                                                           # an axis dropped
        keep = [a for a in range(3) if a != axis]
        assert verdicts(lambda a, b: bool((a[keep] >= lo[keep]).all() and (b[keep] <= hi[keep]).all())) != want
    cell = cell_edges(lo, hi, 308)[0]                                                               # the padded grid box
    assert verdicts(lambda a, b: bool((a >= lo - cell).all() and (b <= hi + cell).all())) != want


def test_cpu_backend_set_rays_renders_the_oracles_frame(restatement):
    """CPURaytracer.set_rays with a buffer that fills the box, under the bars of test_set_rays_cpu.py: every value the oracle's."""
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    objs, lights = live_scene("s300")
    lo, hi = approx_box("s300")
    rays = population("fill_aimed", lo, hi, objs, N, seed=7)
    first = pinhole_rays(96, 96, camera_z_for("s300", 96, 96))
    for kernel in ("shade_and_reflect", "hittest"):
        rt = CPURaytracer(objs, lights, first, DEPTH, kernel=kernel)
        before = rt.Render()
        rt.set_rays(rays)
        got = rt.Render()
        want = restatement[True].render(kernel, objs, lights, rays, DEPTH)["out"]
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        assert same.all(), f"{kernel}: {int((~same).sum())} values differ from the oracle"
        assert not np.array_equal(got, before)
