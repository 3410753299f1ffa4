"""GPU: the block walk ends where a ray leaves the range of occupied cells (csrc/rt_walk_box.h; rt_get_block_range reports the
range), not where it leaves the grid box. Every result must be the one of the grid-box rule (RT_BLOCK_BOX_STOP=0: the same
kernels, the whole grid as the range), of the record walk (RT_WALK3=0: untouched code) and of brute force (grid=False), bit for
bit, under the fused, the unfused and the device-OpenCL arithmetic.

The scene is the 1 800-object cloud of test_block_walk_gpu.py plus six small sentinel spheres, one beyond each side. For caller
rays the cloud sits towards one corner of a box widened by the ray buffer's origins so that every side has a void of at least 10
block cells (RT_GRID_CELLS_PER_OBJECT, a knob results do not depend on, makes the cells small enough for that), and every
sentinel is put - from the grid a first context reports - in the middle of a cell two layers beyond everything else, so that it
alone makes the outermost occupied layer of its side (asserted from rt_get_block_range and the registration spheres): a range one
layer short or shifted loses the rays tangent to it. For frames the pinhole camera sits 12 cells in front of the cloud."""
import numpy as np
import pytest

from helpers import R, camera, instance, rotation, same_floats

pytestmark = pytest.mark.gpu

MODES = {"fused": {}, "unfused": {"fused": False}, "device-opencl": {"device_opencl": True}}
KNOBS = ("RT_BLOCK_BOX_STOP", "RT_WALK3", "RT_GRID_CELLS_PER_OBJECT")
LO, HI = np.array([-30.0, -30.0, -90.0]), np.array([30.0, 30.0, -25.0])   # where the cloud's centres lie (before `offset`)
SENTINEL_OUT, SENTINEL_R = 8.0, 0.5                                       # the sentinels: this far beyond LO / HI, this large
QUEUES = (1, 63, 64, 65, 257)


def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def _cloud(seed, offset=(0.0, 0.0, 0.0), reflection=0.0, lights=3, sentinel_centres=None):
    """test_block_walk_gpu._scene(rng, 1800, 4, 40), moved by `offset`, + six sentinels (the LAST six objects: -x +x -y +y -z +z;
    SENTINEL_OUT beyond the cloud's centres, or where `sentinel_centres` puts them)."""
    rng = np.random.default_rng(seed)
    offset = np.asarray(offset, dtype=np.float64)
    objs = []
    mat = lambda: R.Material(ambient=rng.uniform(0, 1, 3), diffuse=rng.uniform(0, 1, 3), specular=rng.uniform(0, 1, 3),
                             absorption=float(rng.choice([1.0, 0.5, 0.2])), reflection=reflection, shininess=float(rng.choice([1.0, 20.0])))
    for k in range(1800):
        pos = rng.uniform(LO, HI) + offset
        sc = np.full(3, rng.uniform(0.05, 0.6)) if k % 4 else rng.uniform(0.05, 0.6, 3)
        mv, inv = instance(pos, rotation(rng.normal(size=3), rng.uniform(0, 6)), sc)
        objs.append(R.make_object(R.BOX if k % 6 == 0 else R.SPHERE, mat(), mv, inv))
    for k in range(4):  # several cells across
        pos = rng.uniform([-25, -25, -85], [25, 25, -30]) + offset
        mv, inv = instance(pos, rotation(rng.normal(size=3), rng.uniform(0, 6)), np.full(3, rng.uniform(3.0, 9.0)))
        objs.append(R.make_object(R.SPHERE if k % 2 else R.BOX, mat(), mv, inv))
    centre = np.array([5.0, -4.0, -50.0]) + offset
    for k in range(40):  # dozens of objects through one cell
        mv, inv = instance(centre + rng.normal(scale=0.25, size=3), None, np.full(3, rng.uniform(0.2, 0.5)))
        objs.append(R.make_object(R.SPHERE, mat(), mv, inv))
    rng.shuffle(objs)
    mid = (LO + HI) / 2 + offset
    sentinels = []
    for a in range(3):
        for side, face in ((-1.0, LO), (1.0, HI)):
            c = mid.copy()
            c[a] = face[a] + offset[a] + side * SENTINEL_OUT
            if sentinel_centres is not None:
                c = np.asarray(sentinel_centres[len(sentinels)], dtype=np.float64)
            mv, inv = instance(c, None, np.full(3, SENTINEL_R))
            objs.append(R.make_object(R.SPHERE, mat(), mv, inv))
            sentinels.append(c)
    props = R.LightProperties((.1, .1, .1), (.5, .5, .5), (.5, .5, .5))
    ls = [R.make_light(props, position=(*(rng.uniform([-40, -40, 0], [40, 40, 15]) + offset), 1.0)) for _ in range(lights)]
    return R.objects_array(objs), R.lights_array(ls), np.array(sentinels)


def _ray_array(o, d):
    rays = np.zeros(len(o), dtype=R.RAY_DTYPE)
    rays["start"][:, :3] = np.asarray(o, dtype=np.float32)
    rays["start"][:, 3] = 1.0
    rays["direction"][:, :3] = np.asarray(d, dtype=np.float32)
    return rays


# The box of the caller-ray contexts: the cloud + 1.5 of its widths of void below, two above. A registration radius grows with
# the farthest possible ray origin (rt_grid.h: sqrt(3e-6) kappa D), here to some twelve units - two to three block cells - for the
# scene's most anisotropic objects, and the sentinels go two layers beyond that: 64 cells per axis (CELLS_PER_OBJECT) leave more
# than the ten cells of void beyond them on every side (asserted).
CLOUD_LO, CLOUD_HI = LO - SENTINEL_OUT - 1.0, HI + SENTINEL_OUT + 1.0
BOX_LO, BOX_HI = CLOUD_LO - 1.5 * (CLOUD_HI - CLOUD_LO), CLOUD_HI + 2.0 * (CLOUD_HI - CLOUD_LO)
CELLS_PER_OBJECT = "600"


def _box_rays(rng, n=64):
    """The buffer a caller-ray context is created with: its origins span the box (the eight corners first)."""
    corners = np.array([[(BOX_LO, BOX_HI)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    o = np.concatenate([corners, rng.uniform(BOX_LO, BOX_HI, (n - 8, 3))])
    return _ray_array(o, rng.uniform(CLOUD_LO, CLOUD_HI, (n, 3)) - o)


def _tangent_rays(sentinels, rng, per_side):
    """Rays that come from the void side and graze the sentinel of every side inside its true radius, next to the point of it
    that lies farthest out. Returns rays, the sentinel's number (0..5) per ray."""
    o, d, which = [], [], []
    for s, c in enumerate(sentinels):
        a, side = s // 2, (-1.0 if s % 2 == 0 else 1.0)
        for _ in range(per_side):
            u = np.zeros(3); u[(a + 1) % 3] = rng.normal(); u[(a + 2) % 3] = rng.normal()
            u /= np.linalg.norm(u)                       # the ray's direction across the face: perpendicular to the axis ...
            p = c.copy(); p[a] += side * SENTINEL_R * rng.uniform(0.90, 0.9995)   # ... through a point just inside the outermost one
            tilt = np.zeros(3); tilt[a] = -side * rng.uniform(0.0, 0.02)          # ... coming in from outside, a little or not at all
            dirn = u + tilt
            start = p - dirn * rng.uniform(20.0, 40.0)
            o.append(start); d.append(dirn * rng.uniform(0.5, 3.0)); which.append(s)
    return _ray_array(o, d), np.array(which)


def _case_rays(kind, n, rng, br, sentinels):
    """n caller rays of one kind; `br` = the reported range of the context they are for."""
    f_lo, f_hi = np.array(br["face_lo"], dtype=np.float64), np.array(br["face_hi"], dtype=np.float64)
    k = np.arange(n)
    if kind == "inside-out":      # from inside the cloud out through each face: axis-parallel, one zero component, any direction
        o = rng.uniform(LO, HI, (n, 3))
        d = rng.normal(size=(n, 3)) * rng.uniform(0.05, 20.0, (n, 1))
        axis, sign = (k // 2) % 3, np.where(k % 2 == 0, -1.0, 1.0)
        for i in range(n):
            if (i // 6) % 3 == 0:     # axis-parallel: out through face (axis, sign)
                d[i] = 0.0; d[i, axis[i]] = sign[i] * rng.uniform(0.05, 20.0)
            elif (i // 6) % 3 == 1:   # one component exactly zero (or -0), the leading one towards the face
                d[i, (axis[i] + 1) % 3] = 0.0 if i % 4 else -0.0
                d[i, axis[i]] = sign[i] * abs(d[i, axis[i]])
    elif kind == "void-in":       # from the void into the cloud
        o = _void_points(rng, n, br)
        d = (rng.uniform(LO, HI, (n, 3)) - o) * rng.uniform(0.2, 3.0, (n, 1))
    elif kind == "void-past":     # from the void past the cloud: aimed at a point of the void on another side, or away from it
        o = _void_points(rng, n, br)
        d = _void_points(rng, n, br) - o
        away = k % 3 == 0
        d[away] = (o - (LO + HI) / 2)[away]
    elif kind == "face-plane":    # in a face plane of the occupied range: that coordinate is the reported face, its direction 0
        o = rng.uniform(CLOUD_LO, CLOUD_HI, (n, 3))
        d = rng.uniform(LO, HI, (n, 3)) - o
        for i in range(n):
            a = i % 3
            o[i, a] = (f_lo, f_hi)[(i // 3) % 2][a]
            d[i, a] = 0.0
            if i % 5 == 0:        # ... from out in the void
                b = (a + 1) % 3
                o[i, b] = (BOX_LO[b] + CLOUD_LO[b]) / 2 if i % 2 else (BOX_HI[b] + CLOUD_HI[b]) / 2
                d[i, b] = (LO[b] + HI[b]) / 2 - o[i, b]
    else:
        raise ValueError(kind)
    rays = _ray_array(o, d)
    if kind == "face-plane":      # (the face is an fp32 number: keep its bits)
        for i in range(n):
            a = i % 3
            rays["start"][i, a] = np.float32((br["face_lo"], br["face_hi"])[(i // 3) % 2][a])
    return rays


def _void_points(rng, n, br):
    """Points of the box beyond the occupied range on at least one axis."""
    p = rng.uniform(BOX_LO, BOX_HI, (n, 3))
    for i in range(n):
        a = int(rng.integers(3))
        p[i, a] = rng.uniform(BOX_LO[a], br["face_lo"][a] - br["cell"]) if rng.random() < 0.4 else rng.uniform(br["face_hi"][a] + br["cell"], BOX_HI[a])
    return p


def _set_env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _assert_void(br, cells=10):
    assert br["built"] == 1 and br["whole_grid"] == 0, br
    for a in range(3):
        assert br["lo"][a] >= cells and br["cells"][a] - 1 - br["hi"][a] >= cells, br
        assert br["face_lo"][a] < br["face_hi"][a]


VARIANTS = (("box", {}, True), ("grid-box rule", {"RT_BLOCK_BOX_STOP": "0"}, True), ("records", {"RT_WALK3": "0"}, True), ("brute", {}, False))


def _corner_rays(rng, corners):
    """From the box's corners into the cloud: the rays whose origins widen a context's box."""
    o = np.array([[(BOX_LO, BOX_HI)[(c >> a) & 1][a] for a in range(3)] for c in corners])
    return _ray_array(o, (rng.uniform(LO, HI, (len(o), 3)) - o) * rng.uniform(0.5, 2.0, (len(o), 1)))


def _queue(n, br, sentinels):
    """A ray buffer of n rays: the eight corner rays, then the four kinds of caller rays in equal parts."""
    rng = np.random.default_rng(1000 + n)
    parts = [_corner_rays(rng, range(8))]
    kinds = ("inside-out", "void-in", "void-past", "face-plane")
    left = n - 8
    for j, kind in enumerate(kinds):
        m = left // 4 + (1 if j < left % 4 else 0)
        parts.append(_case_rays(kind, m, rng, br, sentinels))
    return np.concatenate(parts)


def _outermost_sentinels(probe):
    """Where the six sentinels go: the middle of the cell two layers beyond the range `probe` (rt_get_block_range of a context with
    the same box and object count) reports, on every side; the other two coordinates are the cloud's middle."""
    cell = float(probe["cell"])
    mid = (LO + HI) / 2
    centres = []
    for a in range(3):
        origin = float(probe["face_lo"][a]) - probe["lo"][a] * cell
        for layer in (probe["lo"][a] - 2, probe["hi"][a] + 2):
            c = mid.copy()
            c[a] = origin + (layer + 0.5) * cell
            centres.append(c)
    return np.array(centres)


def _assert_sentinels_alone_in_the_outermost_layers(br, spheres, sentinels):
    """Each sentinel's registration sphere (the block grid adds 0.01 cell to the fine grid's) lies inside the outermost occupied
    layer of its side, and nothing else reaches that layer."""
    cell = float(br["cell"])
    pad = 0.011 * cell
    others = spheres[:-6]
    for s in range(6):
        a, low = s // 2, s % 2 == 0
        c, r = spheres[len(spheres) - 6 + s, a], spheres[len(spheres) - 6 + s, 3] + pad
        assert abs(c - sentinels[s][a]) < 1e-3 and SENTINEL_R <= r < 0.45 * cell, (s, c, r, cell)
        if low:
            layer_lo, layer_hi = float(br["face_lo"][a]), float(br["face_lo"][a]) + cell
            assert np.all(others[:, a] - others[:, 3] - pad > layer_hi), (s, br)
        else:
            layer_lo, layer_hi = float(br["face_hi"][a]) - cell, float(br["face_hi"][a])
            assert np.all(others[:, a] + others[:, 3] + pad < layer_lo), (s, br)
        assert layer_lo < c - r and c + r < layer_hi, (s, c, r, layer_lo, layer_hi)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_caller_rays_from_in_and_around_a_cloud_in_a_wide_box(monkeypatch, mode):
    """A context's ray count is fixed and its box is made of its own origins, so every queue is a context of its own whose first
    eight rays start in the box's corners: the same box, grid and range for all of them (asserted). A queue of one cannot span
    a box: its ray starts in the low corner, and the three sides towards that corner have the void. Every queue length under
    every arithmetic: the three are three kernels."""
    _set_env(monkeypatch, {"RT_GRID_CELLS_PER_OBJECT": CELLS_PER_OBJECT})
    corner_rays = _corner_rays(np.random.default_rng(30), range(8))
    objs, lights, _ = _cloud(11)
    with hip(objs, lights, corner_rays, 0, kernel="hittest", **MODES[mode]) as rt:
        probe = rt.block_range()
    assert probe["built"] == 1
    sentinels = _outermost_sentinels(probe)
    objs, lights, _ = _cloud(11, sentinel_centres=sentinels)
    with hip(objs, lights, corner_rays, 0, kernel="hittest", **MODES[mode]) as rt:
        br = rt.block_range()
        spheres = rt.grid_spheres()
    _assert_void(br)
    assert br["cell"] == probe["cell"] and br["cells"] == probe["cells"], (br, probe)
    assert br["lo"] == [l - 2 for l in probe["lo"]] and br["hi"] == [h + 2 for h in probe["hi"]], (br, probe)
    _assert_sentinels_alone_in_the_outermost_layers(br, spheres, sentinels)
    tangent, which = _tangent_rays(sentinels, np.random.default_rng(32), 11)
    for s in range(6):   # the tangent rays stay in their sentinel's layer, from start to the point of contact and beyond
        a = s // 2
        layer_lo = float(br["face_lo"][a]) if s % 2 == 0 else float(br["face_hi"][a]) - float(br["cell"])
        o3, d3 = tangent["start"][which == s, :3].astype(np.float64), tangent["direction"][which == s, :3].astype(np.float64)
        contact = np.einsum("ij,ij->i", sentinels[s] - o3, d3) / np.einsum("ij,ij->i", d3, d3)
        for t in (0.0, contact):
            x = o3[:, a] + t * d3[:, a]
            assert np.all((x > layer_lo) & (x < layer_lo + float(br["cell"]))), s
    buffers = [("tangent", np.concatenate([_corner_rays(np.random.default_rng(33), range(8)), tangent]), br)]
    for n in QUEUES:
        if n == 1:
            past = _corner_rays(np.random.default_rng(35), [0])
            past["direction"][0, :3] = (1.0, -0.2, 0.1)   # ... and one that passes the cloud by
            buffers += [("one ray from the low corner", _corner_rays(np.random.default_rng(34), [0]), None), ("one ray past the cloud", past, None)]
        else:
            buffers.append((f"queue of {n}", _queue(n, br, sentinels), br))
    results = {}
    for label, rays, want_range in buffers:
        for name, env, grid in VARIANTS:
            _set_env(monkeypatch, dict(env, RT_GRID_CELLS_PER_OBJECT=CELLS_PER_OBJECT))
            with hip(objs, lights, rays, 0, kernel="hittest", grid=grid, **MODES[mode]) as rt:
                if grid:
                    info = rt.rays_info()
                    assert info["grid_in_use"] == 1 and info["literal"] == 0, (name, label, info)
                    got = rt.block_range()
                    if name == "grid-box rule":
                        assert got["built"] == 1 and got["whole_grid"] == 1 and got["lo"] == [0, 0, 0], (label, got)
                    elif want_range is not None:
                        assert got == want_range, (name, label, got)
                    else:   # one ray: the void lies towards its corner
                        assert got["built"] == 1 and got["whole_grid"] == 0 and min(got["lo"]) >= 10, (label, got)
                t, idx = rt.render_aux()
                assert rt.stats().wavefront == 1 and len(idx) == len(rays)
                results[label, name] = (t.copy(), idx.copy())
    for label, rays, _ in buffers:
        t0, i0 = results[label, "box"]
        for name, _, _ in VARIANTS[1:]:
            t1, i1 = results[label, name]
            assert np.array_equal(i0, i1), f"{mode}, {label} against {name}: {(i0 != i1).sum()} hit indices differ"
            assert same_floats(t0, t1), f"{mode}, {label} against {name}"
    # the cases are what they say: tangent rays meet their sentinel (inside the true radius, in double); of the other rays some
    # hit and many miss
    o = tangent["start"][:, :3].astype(np.float64); d = tangent["direction"][:, :3].astype(np.float64)
    c = sentinels[which]
    along = np.einsum("ij,ij->i", c - o, d) / np.einsum("ij,ij->i", d, d)
    dist = np.linalg.norm(o + along[:, None] * d - c, axis=1)
    assert np.all(dist < SENTINEL_R * 0.9999) and np.all(along > 0)
    idx = results["tangent", "box"][1][8:]
    assert np.all(idx >= 0)
    assert np.array_equal(idx, len(objs) - 6 + which)   # (nothing else lies in those layers)
    idx = results["queue of 257", "box"][1]
    assert (idx >= 0).sum() >= 8 and (idx < 0).sum() > 90   # (a thin cloud: 1 800 objects of size 0.05 .. 0.6 in 60 x 60 x 65)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_ray_from_inside_the_cloud_out_through_each_face(monkeypatch, mode):
    """Queues of one ray that leave the cloud through each of its six faces, axis-parallel. Such a context's box is the objects'
    own: the void beyond the range is the spare layers the grid keeps past its high faces, and none past the low ones."""
    objs, lights, _ = _cloud(16)
    rng = np.random.default_rng(61)
    results = {}
    for face in range(6):
        a, sign = face // 2, (-1.0 if face % 2 == 0 else 1.0)
        d = np.zeros(3); d[a] = sign * rng.uniform(0.2, 5.0)
        rays = _ray_array(rng.uniform(LO, HI, (1, 3)), d[None, :])
        for name, env, grid in VARIANTS:
            _set_env(monkeypatch, env)
            with hip(objs, lights, rays, 0, kernel="hittest", grid=grid, **MODES[mode]) as rt:
                if grid:
                    info = rt.rays_info()
                    assert info["grid_in_use"] == 1 and info["literal"] == 0, (name, face, info)
                    assert rt.block_range()["built"] == 1
                t, idx = rt.render_aux()
                assert rt.stats().wavefront == 1 and len(idx) == 1
                results[face, name] = (t.copy(), idx.copy())
    for face in range(6):
        for name, _, _ in VARIANTS[1:]:
            assert np.array_equal(results[face, name][1], results[face, "box"][1]), (mode, face, name)
            assert same_floats(results[face, name][0], results[face, "box"][0]), (mode, face, name)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_reflecting_frame_with_the_camera_twelve_cells_in_front(monkeypatch, mode):
    objs, lights, _ = _cloud(12, offset=(0.0, 0.0, -100.0), reflection=0.6)
    W = H = 64
    z = float(camera.camera_z(H, 40.0))
    frames = {}
    for name, env, grid in VARIANTS:
        _set_env(monkeypatch, env)
        with hip(objs, lights, None, 3, camera=(W, H, z), grid=grid, **MODES[mode]) as rt:
            if grid:
                info = rt.rays_info()
                assert info["grid_in_use"] == 1 and info["literal"] == 0, (name, info)
            if name == "box":
                br = rt.block_range()
                assert br["built"] == 1 and br["whole_grid"] == 0
                assert br["cells"][2] - 1 - br["hi"][2] >= 12, br   # the camera's side of the cloud: z towards 0
            frame = rt.Render()
            st = rt.count_rays()
            t, idx = rt.render_aux()
            frames[name] = (frame, (st.rays_reference, st.rays_traced, st.hit_pixels), t, idx)
    frame, counts, t, idx = frames["box"]
    assert counts[2] > 150 and counts[1] > W * H + 2 * counts[2]   # hits, and reflection rays behind them
    for name, _, _ in VARIANTS[1:]:
        assert frames[name][1] == counts, (mode, name, frames[name][1], counts)
        assert np.array_equal(frames[name][3], idx) and same_floats(frames[name][2], t), (mode, name)
        assert np.array_equal(frames[name][0].view(np.uint32), frame.view(np.uint32)), (mode, name)


def test_mesh_scene_against_the_record_walk(monkeypatch):
    from opencl_raytracer_amd import scene_loader, tessellate
    from helpers import SCENES
    objs, lights = scene_loader.load_scene(str(SCENES / "roundedCube.txt"))
    scene = tessellate.tessellate(objs, 16, 32, 14)
    scene["reflection"] = 0.5
    W, H = 96, 72
    z = float(camera.camera_z(H))
    frames = {}
    for name, env in (("box", {}), ("grid-box rule", {"RT_BLOCK_BOX_STOP": "0"}), ("records", {"RT_WALK3": "0"})):
        _set_env(monkeypatch, env)
        with hip(scene, lights, None, 3, camera=(W, H, z)) as rt:
            if name == "box":
                br = rt.block_range()
                assert br["built"] == 1 and br["whole_grid"] == 0, br   # (the camera's origin widens the box)
            frame = rt.Render()
            st = rt.count_rays()
            assert st.wavefront == 1 and rt.rays_info()["literal"] == 0
            frames[name] = (frame, (st.rays_reference, st.rays_traced, st.hit_pixels))
    assert frames["box"][1][2] > 500
    for name in ("grid-box rule", "records"):
        assert frames[name][1] == frames["box"][1], name
        assert np.array_equal(frames[name][0].view(np.uint32), frames["box"][0].view(np.uint32)), name


def test_a_sphere_moved_into_the_void_is_still_hit(monkeypatch):
    """rt_set_transforms puts the moved object on the list every ray tests: the range taken at rt_create stays valid."""
    _set_env(monkeypatch, {"RT_GRID_CELLS_PER_OBJECT": CELLS_PER_OBJECT})
    objs, lights, sentinels = _cloud(13)
    rng = np.random.default_rng(41)
    create_rays = _box_rays(rng, 257)
    moved = len(objs) - 1                                        # the +z sentinel goes far out into the void on the +x side
    target = np.array([CLOUD_HI[0] + 0.6 * (BOX_HI[0] - CLOUD_HI[0]), 0.0, (LO[2] + HI[2]) / 2])
    mv, inv = instance(target, None, np.full(3, 6.0))
    new = np.zeros(1, dtype=R.TRANSFORM_DTYPE)
    new["mv"][0] = np.asarray(mv, dtype=np.float32).reshape(16); new["mvInverse"][0] = np.asarray(inv, dtype=np.float32).reshape(16)
    n = 257
    o = rng.uniform(LO, HI, (n, 3))
    rays = _ray_array(o, (target + rng.normal(scale=2.5, size=(n, 3)) - o) * rng.uniform(0.3, 2.0, (n, 1)))
    with hip(objs, lights, create_rays, 0, kernel="hittest") as rt:
        _assert_void(rt.block_range())
        rt.set_transforms(new, first=moved)
        assert rt.geometry_info()["n_dynamic"] == 1
        rt.set_rays(rays)
        assert rt.rays_info()["grid_in_use"] == 1 and rt.rays_info()["literal"] == 0
        t, idx = rt.render_aux()
    with hip(R.with_transforms(objs, new, moved), lights, rays, 0, kernel="hittest", grid=False) as ref:
        t_ref, idx_ref = ref.render_aux()
    assert np.array_equal(idx, idx_ref) and same_floats(t, t_ref)
    assert (idx == moved).sum() > 40                             # rays that left the occupied range and met it out there


def test_hiding_the_outermost_layer_equals_brute_force(monkeypatch):
    """rt_set_visibility only patches types: hidden objects keep their cells, the range stays what it was."""
    _set_env(monkeypatch, {})
    objs, lights, _ = _cloud(14, offset=(0.0, 0.0, -100.0), reflection=0.6)
    W = H = 64
    z = float(camera.camera_z(H, 40.0))
    with hip(objs, lights, None, 3, camera=(W, H, z)) as rt:
        br = rt.block_range()
        assert br["built"] == 1 and br["whole_grid"] == 0
        sph = rt.grid_spheres()                                   # what the objects are registered with: centre, radius
        f_lo, f_hi, cell = np.array(br["face_lo"]), np.array(br["face_hi"]), br["cell"]
        reach_lo, reach_hi = sph[:, :3] - sph[:, 3:4], sph[:, :3] + sph[:, 3:4]
        outer = np.any((reach_lo < f_lo + 1.02 * cell) | (reach_hi > f_hi - 1.02 * cell), axis=1)   # whatever reaches an outermost cell
        for a in range(3):                                        # ... which on every side something does
            assert (reach_lo[:, a] < f_lo[a] + cell).any() and (reach_hi[:, a] > f_hi[a] - cell).any()
        assert 6 <= outer.sum() < len(objs) - 100
        visible = (~outer).astype(np.uint8)
        rt.set_visibility(visible)
        assert rt.rays_info()["grid_in_use"] == 1 and rt.rays_info()["literal"] == 0
        frame = rt.Render()
        st = rt.count_rays()
        counts = (st.rays_reference, st.rays_traced, st.hit_pixels)
        assert rt.block_range() == br
    with hip(R.with_visibility(objs, visible), lights, None, 3, camera=(W, H, z), grid=False) as ref:
        want = ref.Render()
        st = ref.count_rays()
        assert (st.rays_reference, st.rays_traced, st.hit_pixels) == counts
    assert counts[2] > 100
    assert np.array_equal(frame.view(np.uint32), want.view(np.uint32))


def test_a_box_the_objects_fill(monkeypatch):
    """Ray origins inside the cloud: the box is the objects' box and the range reaches its low faces and - short of the spare cells
    the grid keeps beyond the high ones - its high faces: next to nothing to gain, and nothing may change. The range that IS the
    whole grid is the RT_BLOCK_BOX_STOP=0 variant of every test in this file."""
    objs, lights, _ = _cloud(15)
    rng = np.random.default_rng(51)
    n = 4000
    o = rng.uniform(LO, HI, (n, 3))
    rays = _ray_array(o, rng.normal(size=(n, 3)) * rng.uniform(0.01, 50.0, (n, 1)))
    got = {}
    for name, env, grid in VARIANTS:
        _set_env(monkeypatch, env)
        with hip(objs, lights, rays, 0, kernel="hittest", grid=grid) as rt:
            if grid:
                br = rt.block_range()
                assert br["built"] == 1 and br["lo"] == [0, 0, 0] and all(h < c for h, c in zip(br["hi"], br["cells"])), (name, br)
                assert br["whole_grid"] == (1 if name == "grid-box rule" else int(br["hi"] == [c - 1 for c in br["cells"]]))
                assert rt.rays_info()["grid_in_use"] == 1
            got[name] = rt.render_aux()
    for name, _, _ in VARIANTS[1:]:
        assert np.array_equal(got[name][1], got["box"][1]) and same_floats(got[name][0], got["box"][0]), name
    assert (got["box"][1] >= 0).sum() > 200 and (got["box"][1] < 0).sum() > 500   # (a thin cloud: one ray in ten meets something)
