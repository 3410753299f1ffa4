"""GPU: supersampled frames (hip_raytracer.h, "supersampled frames"; csrc/rt_resolve.hip) through every layer. The specification
every frame is held to is resolve.box_filter (tests/test_supersample_cpu.py checks it against the written-out definition): a
context with factor s delivers box_filter of the sample frame the same context renders with factor 1, bit for bit."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import camera, expected_full, fixture_names, load_fixture, random_scene, same_floats
from test_packed_cpu import random_bit_patterns

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
FORMATS = (("rgba8", 4), ("rgb8", 3))
FACTORS = (2, 3, 4)


def _camera_colour_fixtures():
    names = []
    for n in fixture_names():
        z = np.load(ROOT / "tests" / "golden" / f"{n}.npz")
        if int(z["kernel"]) != 0 and "camera" in z.files and factors_of(int(z["camera"][0]), int(z["camera"][1])):
            names.append(n)
    return names




def hip(*a, **k):
    from opencl_raytracer_amd.hip_raytracer import HIPRaytracer
    return HIPRaytracer(*a, **k)


def box(frame, w, s):
    from opencl_raytracer_amd import resolve
    return resolve.box_filter(np.asarray(frame, F).reshape(-1, 4), w, s)


def qbytes(frame, channels):
    from opencl_raytracer_amd import ppm
    return ppm.quantise_bytes(np.asarray(frame, F).reshape(-1, 4))[:, :channels]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def factors_of(w, h):
    return [s for s in FACTORS if w % s == 0 and h % s == 0]


CAMERA_FIXTURES = _camera_colour_fixtures()


def oracle_bound(samples, s):
    """|dRGB| allowed between the filtered GPU frame and the filtered oracle frame: 1e-5 is the project's bar per sample, and a
    mean of samples within 1e-5 is within 1e-5; 2 s^2 2^-24 M bounds the roundings of s^2 - 1 additions and one multiplication on
    each side (each at most 2^-24 relative to a partial sum <= s^2 M, scaled by 1 / s^2), M the largest finite channel."""
    rgb = np.asarray(samples)[:, :3]
    finite = np.abs(rgb[np.isfinite(rgb)])
    M = float(finite.max()) if finite.size else 0.0
    return 1e-5 + 2.0 * s * s * 2.0 ** -24 * M


def filtered_error(got, want):
    from helpers import compare_frames
    return compare_frames(got, want)


def check_self_identity(rt, w, h, factors, label):
    """Render() with the factor == box_filter(Render() with factor 1) on the same context; rt_render_device into caller memory on a
    non-default stream gives the same bits. Returns the sample frame."""
    rt.set_supersampling(1)
    samples = rt.Render()
    assert samples.shape == (w * h, 4)
    side = torch.cuda.Stream()
    for s in factors:
        rt.set_supersampling(s)
        assert rt.supersampling == s and rt.local_pixels == w * h // (s * s) and rt.local_rays == w * h
        got = rt.Render()
        want = box(samples, w, s)
        assert got.shape == want.shape, (label, s)
        assert same_floats(got, want), (label, s, int(np.sum(bits(got) != bits(want))))
        out = torch.full((len(want) + 4, 4), -7.0, dtype=torch.float32, device="cuda")
        with torch.cuda.stream(side):
            rt.render_device(out.data_ptr(), side.cuda_stream)
            copy = out.clone()
        side.synchronize()
        dev = copy.cpu().numpy()
        assert same_floats(dev[: len(want)], want), (label, s, "render_device")
        assert np.all(dev[len(want):] == -7.0), (label, s, "written behind the last pixel")
    rt.set_supersampling(1)
    assert np.array_equal(bits(rt.Render()), bits(samples)), (label, "factor 1 after a factor > 1")
    return samples


# ---- 1 + 2. self-identity on every path, and against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("name", CAMERA_FIXTURES)
def test_fixture_self_identity_and_oracle(name):
    """every colour fixture with a camera, taken as a SAMPLE grid, for every factor that divides its width and height, through the
    monolithic and the large-scene path; the filtered frame against box_filter of the reference's own golden sample frame"""
    fx = load_fixture(name)
    w, h, fov = fx["camera"]
    factors = factors_of(w, h)
    cam = (w, h, float(camera.camera_z(h, fov)))
    want_samples = expected_full(fx, True)
    for path in ("monolithic", "wavefront"):
        with hip(fx["objs"], fx["lights"], None, fx["max_bounces"], kernel=fx["kernel"], camera=cam, path=path) as rt:
            check_self_identity(rt, w, h, factors, (name, path))
            for s in factors:
                rt.set_supersampling(s)
                err = filtered_error(rt.Render(), box(want_samples, w, s))
                print(f"{name} {path} s={s}: max |dRGB| = {err:.3e} (bound {oracle_bound(want_samples, s):.3e})")
                assert err <= oracle_bound(want_samples, s), (name, path, s, err)


def test_every_factor_is_covered_by_the_fixtures():
    seen = set()
    for name in CAMERA_FIXTURES:
        w, h, _ = load_fixture(name)["camera"]
        seen.update(factors_of(w, h))
    assert seen == set(FACTORS) and len(CAMERA_FIXTURES) >= 40


@pytest.mark.parametrize("kind", ["grid", "literal", "device_opencl", "triangles"])
def test_self_identity_on_the_other_paths(restatement, kind):
    """a synthetic scene above 96 objects through the grid, literal=True, device_opencl=True, a triangle scene: all three factors on
    a 96 x 72 sample grid; grid and literal against the oracle's filtered sample frame as well"""
    from opencl_raytracer_amd import synthetic, tessellate
    w, h, depth = 96, 72, 3
    z = float(camera.camera_z(h))
    kw = {}
    if kind == "grid":
        objs, lights = synthetic.spheres_and_lights(300, 3)
    elif kind == "triangles":
        base, lights = random_scene(3, 2, 2, seed=31, spread=3.0, zrange=(-14.0, -8.0))
        objs = tessellate.tessellate(base, 8, 16, 2)
    else:
        objs, lights = random_scene(14, 10, 3, seed=55, directional_lights=1)
        kw = {"literal": True} if kind == "literal" else {"device_opencl": True}
    with hip(objs, lights, None, depth, camera=(w, h, z), **kw) as rt:
        samples = check_self_identity(rt, w, h, FACTORS, kind)
        if kind in ("grid", "triangles"):
            assert rt.stats().wavefront == 1
        assert np.any(samples[:, :3] != 0)
        if kind in ("grid", "literal"):
            ref = restatement[True].render("shade_and_reflect", objs, lights, camera.grid_rays(w, h, z), depth, want_aux=False)["out"]
            for s in FACTORS:
                rt.set_supersampling(s)
                err = filtered_error(rt.Render(), box(ref, w, s))
                print(f"{kind} s={s}: max |dRGB| = {err:.3e} (bound {oracle_bound(ref, s):.3e})")
                assert err <= oracle_bound(ref, s), (kind, s, err)


def test_the_friendly_constructor():
    """HIPRaytracer(camera=(W, H, z), supersample=s): s^2 W H work-items, W H pixels, the frame of a context given the sample camera
    and the factor by hand"""
    objs, lights = random_scene(8, 6, 2, seed=12, directional_lights=1)
    W, H = 40, 30
    z = float(camera.camera_z(H))
    for s in FACTORS:
        sw, sh, sz = camera.supersampled(W, H, z, s)
        with hip(objs, lights, None, 2, camera=(W, H, z), supersample=s) as rt:
            assert rt.n_rays == sw * sh and rt.local_rays == sw * sh and rt.local_pixels == W * H and rt.supersampling == s
            st = rt.stats()
            assert (st.width, st.height) == (sw, sh)
            got = rt.Render()
            assert rt.count_rays().local_rays == sw * sh           # counters keep counting samples
        with hip(objs, lights, None, 2, camera=(sw, sh, float(sz))) as rt:
            samples = rt.Render()
        assert got.shape == (W * H, 4) and np.all(got[:, 3] == 1.0)
        assert same_floats(got, box(samples, sw, s))
    with pytest.raises(ValueError):
        hip(objs, lights, camera.primary_rays(8, 8), 2, supersample=2)


# ---- 3. bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["monolithic", "wavefront"])
def test_bytes_are_the_quantised_filtered_frame(path):
    """render_packed / render_device_packed for both formats == quantise_bytes(box_filter(float sample frame)), destinations 4, 8
    and 12 bytes behind a 16-byte boundary included, guard bytes behind the last pixel untouched"""
    objs, lights = random_scene(20, 12, 3, seed=77, directional_lights=1, spread=7.0)
    w, h = 120, 72
    with hip(objs, lights, None, 3, camera=(w, h, float(camera.camera_z(h))), path=path) as rt:
        samples = rt.Render()
        stream = torch.cuda.current_stream().cuda_stream
        for s in FACTORS:
            rt.set_supersampling(s)
            pixels = box(samples, w, s)
            n = len(pixels)
            for fmt, ch in FORMATS:
                want = qbytes(pixels, ch)
                got = rt.render_packed(fmt)
                assert got.shape == (n, ch) and np.array_equal(got, want), (s, fmt)
                for offset in (0, 4, 8, 12):
                    dst = torch.full((offset + n * ch + 80,), 0xA5, dtype=torch.uint8, device="cuda")
                    base = (-dst.data_ptr()) % 16 + offset
                    rt.render_device_packed(dst.data_ptr() + base, fmt, stream)
                    raw = dst.cpu().numpy()
                    assert np.array_equal(raw[base: base + n * ch].reshape(n, ch), want), (s, fmt, offset)
                    assert np.all(raw[:base] == 0xA5) and np.all(raw[base + n * ch:] == 0xA5), (s, fmt, offset, "guard bytes written")
        rt.set_supersampling(1)
        assert np.array_equal(rt.render_packed("rgba8"), qbytes(samples, 4))


# ---- 4. the pass alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [None, "pixel", "sample"])
def test_resolve_device_on_all_bit_patterns(monkeypatch, form):
    """rt_resolve_device on frames drawn over ALL fp32 bit patterns (NaN, inf, denormals, -0 in them), widths that are no multiples
    of 64 s, one-row and one-pixel frames, float and both byte outputs, odd 4-byte-aligned byte destinations: box_filter exactly
    (NaN where it has NaN), bytes = quantise_bytes of it, nothing written behind the last pixel. Both kernel forms (RT_RESOLVE_FORM,
    read per call) and the default."""
    if form: monkeypatch.setenv("RT_RESOLVE_FORM", form)
    else: monkeypatch.delenv("RT_RESOLVE_FORM", raising=False)
    pool = random_bit_patterns(1 << 20).copy()
    # half of the pool tamed to finite colours, so that many channels are plain numbers; the wild half keeps every kind of bit
    # pattern, and the values a draw of a million rarely holds are put in by hand all along it
    pool[::2] = np.random.default_rng(3).uniform(-0.5, 1.5, size=len(pool) // 2).astype(F)
    special = np.array([np.inf, -np.inf, -0.0, 0.0, np.nan, 1e-45, -1e-45, 1e-39, 3.4e38, -3.4e38, 1.0, 255.0 / 256.0], F)
    spots = np.arange(1, len(pool), 37)
    pool[spots] = special[np.arange(len(spots)) % len(special)]
    head = pool[: 4 * 12 * 43 * 12 * 5]                              # what the largest frame below reads
    assert np.isnan(head).sum() > 100 and np.isposinf(head).sum() > 10 and np.isneginf(head).sum() > 10
    assert np.sum((head != 0) & (np.abs(head) < np.finfo(F).tiny)) > 10 and np.sum(np.signbit(head) & (head == 0)) > 10
    src = torch.from_numpy(pool.view(np.int32).copy()).cuda()      # (as integers: no NaN canonicalisation on the way)
    assert src.data_ptr() % 16 == 0
    objs, lights = random_scene(1, 1, 1, seed=1)
    stream = torch.cuda.current_stream().cuda_stream
    with hip(objs, lights, camera.primary_rays(8, 8), 0) as rt:
        for s in FACTORS:
            shapes = [(s, s), (s * 5, s), (s, s * 7), (s * 21, s * 3), (s * 63, s * 2), (s * 64, s * 2), (s * 65, s * 5), (s * 100, s * 9),
                      (12 * 43, 12 * 5)]
            for w, rows in shapes:
                n_samples = w * rows
                assert n_samples * 4 <= len(pool)
                samples = pool[: n_samples * 4].reshape(-1, 4)
                want = box(samples, w, s)
                n = len(want)
                out = torch.full((n + 8, 4), -7.0, dtype=torch.float32, device="cuda")
                rt.resolve_device(src.data_ptr(), w, rows, s, out.data_ptr(), None, stream)
                got = out.cpu().numpy()
                assert np.all(got[n:] == -7.0), (s, w, rows, "written behind the last pixel")
                assert same_floats(got[:n], want), (s, w, rows, form, int(np.sum(~((got[:n] == want) | (np.isnan(got[:n]) & np.isnan(want))))))
                assert np.array_equal(np.isnan(got[:n]), np.isnan(want))
                for fmt, ch in FORMATS:
                    wantb = qbytes(want, ch)
                    for offset in (0, 4):
                        dst = torch.full((offset + n * ch + 80,), 0xA5, dtype=torch.uint8, device="cuda")
                        base = (-dst.data_ptr()) % 16 + offset
                        rt.resolve_device(src.data_ptr(), w, rows, s, dst.data_ptr() + base, fmt, stream)
                        raw = dst.cpu().numpy()
                        assert np.array_equal(raw[base: base + n * ch].reshape(n, ch), wantb), (s, w, rows, fmt, offset, form)
                        assert np.all(raw[:base] == 0xA5) and np.all(raw[base + n * ch:] == 0xA5), (s, w, rows, fmt, "guard bytes written")
        # s = 1: the samples themselves / their bytes
        out = torch.full((40, 4), -7.0, dtype=torch.float32, device="cuda")
        rt.resolve_device(src.data_ptr(), 8, 4, 1, out.data_ptr(), None, stream)
        assert np.array_equal(bits(out.cpu().numpy()[:32]), bits(pool[:128].reshape(-1, 4))) and np.all(out.cpu().numpy()[32:] == -7.0)


def test_resolve_device_refusals():
    from opencl_raytracer_amd.hip_raytracer import RTError
    objs, lights = random_scene(1, 1, 1, seed=1)
    src = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((64, 4), -7.0, dtype=torch.float32, device="cuda")
    with hip(objs, lights, camera.primary_rays(8, 8), 0) as rt:
        for args in ((8, 8, 0, None), (8, 8, 5, None), (8, 7, 2, None), (9, 8, 2, None), (8, 8, 2, 7)):
            w, rows, s, fmt = args
            with pytest.raises(RTError) as e:
                rt.resolve_device(src.data_ptr(), w, rows, s, out.data_ptr(), fmt, 0)
            assert e.value.code == -1, args
        for bad_src, bad_dst, fmt in ((src.data_ptr() + 4, out.data_ptr(), None), (src.data_ptr(), out.data_ptr() + 4, None),
                                      (src.data_ptr(), out.data_ptr() + 2, "rgba8"), (0, out.data_ptr(), None), (src.data_ptr(), 0, "rgb8")):
            with pytest.raises(RTError) as e:
                rt.resolve_device(bad_src, 8, 8, 2, bad_dst, fmt, 0)
            assert e.value.code == -1
        rt.resolve_device(0, 0, 0, 2, 0, None, 0)          # zero pixels: RT_OK, nothing launched
        rt.resolve_device(src.data_ptr(), 8, 0, 2, out.data_ptr(), None, 0)
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == -7.0)


# ---- 5. shards, passes, several contexts, several ranks --------------------------------------------------------------------------
@pytest.mark.parametrize("s,world,tile_rows", [(2, 2, 16), (2, 3, 8), (3, 2, 15), (3, 3, 48), (4, 3, 8)])
def test_shards_assemble_to_the_unsharded_filtered_frame(s, world, tile_rows):
    """whole-row tiles, a ragged last tile every time (108 sample rows): the shards' pixels assembled by sharding.assemble_frame
    equal the unsharded filtered frame; so do the byte shards"""
    from opencl_raytracer_amd import sharding, synthetic
    objs, lights = synthetic.spheres_and_lights(200, 3)
    w, h = 144, 108 if tile_rows != 48 else 120
    cam = (w, h, float(camera.camera_z(h)))
    tile = sharding.tile_rays_for_rows(w, sharding.whole_pixel_rows(tile_rows, s))
    assert (w * h) % tile != 0
    n_pix, tile_pix = w * h // (s * s), tile // (s * s)
    with hip(objs, lights, None, 3, camera=cam) as rt:
        rt.set_supersampling(s)
        whole = rt.Render()
        whole8 = rt.render_packed("rgb8")
        pieces, pieces8 = [], []
        for rank in range(world):
            rt.set_shard(tile, rank, world)
            assert rt.local_rays == sharding.local_rays(w * h, tile, rank, world) and rt.local_pixels == rt.local_rays // (s * s)
            pieces.append(rt.Render())
            pieces8.append(rt.render_packed("rgb8"))
            assert pieces[-1].shape == (rt.local_pixels, 4)
    assert np.array_equal(bits(sharding.assemble_frame(pieces, tile_pix, n_pix)), bits(whole))
    assert np.array_equal(sharding.assemble_frame(pieces8, tile_pix, n_pix), whole8)
    # the padding of the ragged last tile filters to the background exactly
    last = (sharding.n_tiles(w * h, tile) - 1) % world
    pad = pieces[last][len(pieces[last]) - (sharding.n_tiles(w * h, tile) * tile_pix - n_pix):]
    assert len(pad) and np.array_equal(pad, np.tile(np.array([0, 0, 0, 1], F), (len(pad), 1)))


@pytest.mark.parametrize("s", [2, 3])
def test_passes_do_not_change_the_frame(monkeypatch, s):
    """RT_RENDER_PASSES=2 against =1 on the large-scene path, float, RGBA8 and RGB8 (the 3-byte element is the one a pass's tile-byte
    arithmetic can get wrong while 4- and 16-byte elements pass), the default split and a split of three passes"""
    from opencl_raytracer_amd import synthetic
    objs, lights = synthetic.spheres_and_lights(900, 4)
    w, h = 168, 156            # 9.75 tiles of 16 rows, 3.25 of 48
    cam = (w, h, float(camera.camera_z(h)))
    monkeypatch.setenv("RT_RENDER_PASSES", "1")
    with hip(objs, lights, None, 3, camera=cam) as rt:
        samples = rt.Render()
        rt.set_supersampling(s)
        one, one8, one3 = rt.Render(), rt.render_packed("rgba8"), rt.render_packed("rgb8")
        assert rt.stats().wavefront == 1
    assert same_floats(one, box(samples, w, s)) and np.array_equal(one8, qbytes(one, 4)) and np.array_equal(one3, one8[:, :3])
    monkeypatch.setenv("RT_RENDER_PASSES", "2")
    with hip(objs, lights, None, 3, camera=cam) as rt:
        rt.set_supersampling(s)
        for split in (None, "1,1", "2,1,1"):
            if split: monkeypatch.setenv("RT_RENDER_SPLIT", split)
            for _ in range(2):
                assert np.array_equal(bits(rt.Render()), bits(one)), split
                assert np.array_equal(rt.render_packed("rgba8"), one8), split
                assert np.array_equal(rt.render_packed("rgb8"), one3), split
        monkeypatch.delenv("RT_RENDER_SPLIT")
        assert rt.local_rays == w * h and rt.local_pixels == w * h // (s * s)
        rt.set_supersampling(1)
        assert np.array_equal(bits(rt.Render()), bits(samples))      # the unfiltered frame through the same passes


@pytest.mark.parametrize("s", [2, 3, 4])
def test_multi_over_one_gpu(s):
    from opencl_raytracer_amd import synthetic
    from opencl_raytracer_amd.hip_raytracer import MultiHIPRaytracer, RTError
    objs, lights = synthetic.spheres_and_lights(200, 3)
    W, H = 48, 40 if s != 3 else 36            # sample rows 80, 108, 160: ragged against tiles of 16 / 48 rows
    z = float(camera.camera_z(H))
    with hip(objs, lights, None, 3, camera=(W, H, z), supersample=s) as rt:
        want, want8 = rt.Render(), rt.render_packed("rgba8")
    with MultiHIPRaytracer(objs, lights, None, 3, devices=(0, 0), camera=(W, H, z), supersample=s) as m:
        assert m.n_pixels == W * H and m.frame_pixels == m.frame_elems // (s * s) and m.frame_pixels >= W * H
        for _ in range(2):
            assert np.array_equal(bits(m.Render()), bits(want))
            assert np.array_equal(m.render_packed("rgba8"), want8)
            assert np.array_equal(m.render_packed("rgb8"), want8[:, :3])
        frame = torch.full((m.frame_pixels + 2, 4), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.render_device(frame.data_ptr())
        got = frame.cpu().numpy()
        assert np.array_equal(bits(got[: W * H]), bits(want)) and np.all(got[m.frame_pixels:] == -7.0)
        assert m.stats().local_rays >= s * s * W * H
    if s == 3:   # the derived tile of the C ABI (16 rows) holds no whole pixel rows for s = 3: refused, the multi stays as it was
        sw, sh, sz = camera.supersampled(W, H, z, 3)
        with MultiHIPRaytracer(objs, lights, None, 3, devices=(0, 0), camera=(sw, sh, float(sz))) as m:
            before = m.Render()
            with pytest.raises(RTError) as e:
                m.set_supersampling(3)
            assert e.value.code == -1 and m.supersample == 1 and m.frame_pixels == m.frame_elems
            assert np.array_equal(bits(m.Render()), bits(before))
            m.set_supersampling(2)
            assert same_floats(m.Render(), box(before, sw, 2))


@pytest.mark.parametrize("output", ["float", "rgba8"])
def test_ranks_sharing_one_gpu_over_gloo(output):
    """world 2 over gloo on the one GPU: ShardedHIPRaytracer(supersample=s) on rank 0 equals the single context with the same factor,
    synchronous and pipelined, s = 2 on the small-scene kernel and s = 3 on the grid path with a ragged last tile"""
    world = 2
    port = 32700 + (os.getpid() % 1500) + (0 if output == "float" else 9)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "tests" / "mp_supersample_worker.py"), output]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count(": ok") == 4 and "MISMATCH" not in res.stdout, res.stdout


# ---- 6. lifecycle and refusals -------------------------------------------------------------------------------------------------
def test_factor_walk_on_a_live_context():
    """factor 2 -> render -> 1 -> render -> 3 -> camera of another size -> render -> 4 with bytes: each frame equals a fresh
    context's"""
    objs, lights = random_scene(16, 10, 3, seed=91, directional_lights=1)
    n = 96 * 72

    def fresh(cam, s, packed=None):
        with hip(objs, lights, None, 3, camera=cam) as rt:
            rt.set_supersampling(s)
            return rt.render_packed(packed) if packed else rt.Render()

    cam_a = (96, 72, float(camera.camera_z(72)))
    cam_b = (72, 96, float(camera.camera_z(96)) * 1.25)
    cam_c = (144, 48, float(camera.camera_z(48)))
    with hip(objs, lights, None, 3, camera=cam_a) as rt:
        assert rt.n_rays == n
        rt.set_supersampling(2)
        assert np.array_equal(bits(rt.Render()), bits(fresh(cam_a, 2)))
        rt.set_supersampling(1)
        assert np.array_equal(bits(rt.Render()), bits(fresh(cam_a, 1)))
        rt.set_supersampling(3)
        rt.set_camera(*cam_b)
        assert np.array_equal(bits(rt.Render()), bits(fresh(cam_b, 3)))
        rt.set_supersampling(4)
        rt.set_camera(*cam_c)
        assert np.array_equal(rt.render_packed("rgb8"), fresh(cam_c, 4, "rgb8"))
        assert np.array_equal(bits(rt.Render()), bits(fresh(cam_c, 4)))
        rt.set_supersampling(1)
        assert np.array_equal(bits(rt.Render()), bits(fresh(cam_c, 1)))
        t, idx = rt.render_aux()                      # aux works again at factor 1
        assert len(t) == n and len(idx) == n


def test_refusals_leave_the_context_as_it_was():
    from opencl_raytracer_amd.hip_raytracer import RTError
    objs, lights = random_scene(6, 5, 2, seed=5)
    w, h = 48, 36
    cam = (w, h, float(camera.camera_z(h)))

    def refused(code, fn, *a):
        with pytest.raises(RTError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)

    def state(rt):
        st = rt.stats()
        return rt.supersampling, st.width, st.height, rt.local_rays, rt.local_pixels

    with hip(objs, lights, None, 2, camera=cam) as rt:
        rt.set_supersampling(2)
        before, s0 = rt.Render(), state(rt)
        for bad in (0, 5, 17):
            refused(-1, rt.set_supersampling, bad)                              # outside 1..4
        refused(-1, rt.set_camera, 27, 64, cam[2])                              # 27 % 2: a camera the factor does not divide
        refused(-1, rt.set_camera, 64, 27, cam[2])
        refused(-1, rt.set_shard, 3 * w, 0, 2)                                  # a tile of 3 sample rows holds no whole pixel rows
        refused(-1, rt.set_shard, w + 2, 1, 3)
        buf = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        refused(-5, _set_aux(rt), buf.data_ptr(), 0)                            # aux is per work-item
        refused(-5, rt.render_aux)
        assert state(rt) == s0
        assert np.array_equal(bits(rt.Render()), bits(before))
        # the shard comes first, then a factor that its tiles do not hold
        rt.set_supersampling(1)
        rt.set_shard(4 * w, 1, 2)
        s1, shard_before = state(rt), rt.Render()
        refused(-1, rt.set_supersampling, 3)                                    # 4 rows % 3
        assert state(rt) == s1 and np.array_equal(bits(rt.Render()), bits(shard_before))
        rt.set_supersampling(4)                                                  # 4 rows: one pixel row per tile
        assert rt.local_pixels == rt.local_rays // 16
        refused(-1, rt.set_camera, 36, 48, cam[2])                              # tile 4 * 48 rays is no multiple of 4 * 36
        assert state(rt)[:3] == (4, w, h)
    with hip(objs, lights, None, 2, camera=cam) as rt:                          # aux buffers set first: no factor
        buf = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        _set_aux(rt)(buf.data_ptr(), 0)
        refused(-5, rt.set_supersampling, 2)
        assert rt.supersampling == 1
        _set_aux(rt)(0, 0)
        rt.set_supersampling(2)
        assert rt.local_pixels == w * h // 4
    with hip(objs, lights, None, 0, camera=cam, kernel="hittest") as rt:        # a time is not a colour
        before = rt.Render()
        refused(-5, rt.set_supersampling, 2)
        refused(-1, rt.set_supersampling, 9)
        rt.set_supersampling(1)
        assert rt.supersampling == 1 and np.array_equal(bits(rt.Render()), bits(before))
    rays = camera.primary_rays(w, h)
    with hip(objs, lights, rays, 2, raygen=False) as rt:                        # rays from a buffer: no pinhole grid, no factor
        before = rt.Render()
        refused(-1, rt.set_supersampling, 2)
        assert rt.supersampling == 1 and np.array_equal(bits(rt.Render()), bits(before))
    with hip(objs, lights, rays, 2) as rt:                                      # the same buffer accepted as a pinhole grid: fine
        rt.set_supersampling(2)
        assert same_floats(rt.Render(), box(before, w, 2))


def _set_aux(rt):
    import ctypes

    def call(t_ptr, i_ptr):
        rt._check(rt._lib.rt_set_aux_device(rt._ctx, ctypes.c_void_p(t_ptr) if t_ptr else None, ctypes.c_void_p(i_ptr) if i_ptr else None))
    return call


def test_scene_tool_takes_ss(tmp_path):
    """scene_tool render / render8 --ss 2 on the GPU: the picture keeps its size and is the P3 / P6 of the Python frame"""
    from opencl_raytracer_amd import ppm, scene_loader
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    scene = ROOT / "scenes" / "simpleSphere.txt"
    W, H, s = 64, 48, 2
    z = camera.camera_z(H)
    zbits = f"{int(F(z).view(np.uint32)):08x}"
    objs, lights = scene_loader.load_scene(str(scene))
    with hip(objs, lights, None, 3, camera=(W, H, float(z)), supersample=s) as rt:
        floats, rgb = rt.Render(), rt.render_packed("rgb8")
    out = tmp_path / "a.ppm"
    res = subprocess.run([str(tool), "render", "--ss", "2", str(scene), str(W), str(H), "3", str(out), zbits], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert out.read_bytes() == ppm.format_p3(W, H, ppm.rgba_to_rgb(floats))
    res = subprocess.run([str(tool), "render8", str(scene), str(W), str(H), "3", str(out), zbits, "p6", "rgb8", "--ss", "2"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert out.read_bytes() == f"P6\n{W} {H}\n255\n".encode() + rgb.tobytes()
