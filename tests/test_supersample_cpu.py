"""No GPU: supersampled frames (hip_raytracer.h, "supersampled frames") - the definition in its executable form
(resolve.box_filter), the geometric claim behind it checked with the oracle, the CPU backend's own filter loop, the new symbols of
the C ABI, the sharding helper and the exchange of pixel-sized tiles (distributed.FrameGather over gloo)."""
import ctypes
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import camera, random_scene, same_floats

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "hip_raytracer.h"
NEW_SYMBOLS = ("rt_set_supersampling", "rt_supersampling", "rt_local_pixels", "rt_resolve_device", "rt_set_supersampling_multi",
               "rt_multi_frame_pixels")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def slow_box_filter(frame, w, s):
    """the definition written out pixel by pixel, channel by channel, with numpy float32 scalars"""
    frame = np.asarray(frame, F)
    h = len(frame) // w
    out = np.empty((w // s * (h // s), frame.shape[1]), F)
    k = F(1.0) / F(s * s)
    with np.errstate(all="ignore"):
        for j in range(h // s):
            for i in range(w // s):
                for c in range(frame.shape[1]):
                    acc = frame[(s * j) * w + s * i, c]
                    for b in range(s):
                        for a in range(s):
                            if a or b:
                                acc = F(acc + frame[(s * j + b) * w + s * i + a, c])
                    out[j * (w // s) + i, c] = F(acc * k)
    return out


# ---- 1. box_filter -------------------------------------------------------------------------------------------------------------
def test_factor_one_is_the_identity():
    from opencl_raytracer_amd import resolve
    x = np.random.default_rng(1).normal(size=(35, 4)).astype(F)
    got = resolve.box_filter(x, 7, 1)
    assert np.array_equal(bits(got), bits(x)) and got is not x


def test_the_order_of_the_additions_is_pinned():
    """(1e8 + 1) - 1e8 + 1 in fp32: the 1 added to 1e8 is lost (ulp 8), the last one survives - 1 * 0.25. Any order that adds the
    two 1s first, or a tree (1e8 + 1) + (-1e8 + 1), gives 0.5 or 0."""
    from opencl_raytracer_amd import resolve
    block = np.array([[1e8] * 4, [1] * 4, [-1e8] * 4, [1] * 4], F)     # (b, a) = (0,0), (0,1), (1,0), (1,1)
    assert np.array_equal(resolve.box_filter(block, 2, 2), np.full((1, 4), 0.25, F))
    # a then b swapped (column-major) would visit 1e8, -1e8, 1, 1 -> 0.5
    assert np.array_equal(resolve.box_filter(block[[0, 2, 1, 3]], 2, 2), np.full((1, 4), 0.5, F))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_box_filter_is_the_written_out_definition(s):
    from opencl_raytracer_amd import resolve
    rng = np.random.default_rng(40 + s)
    w, h = 12, 24
    x = (rng.normal(size=(w * h, 4)) * 10.0 ** rng.integers(-3, 6, size=(w * h, 4))).astype(F)
    got = resolve.box_filter(x, w, s)
    assert got.dtype == F and got.shape == (w * h // (s * s), 4)
    assert np.array_equal(bits(got), bits(slow_box_filter(x, w, s)))


def test_constants_w_and_special_values():
    from opencl_raytracer_amd import resolve
    # A constant frame stays that constant, bit for bit:
    #   s = 2 for EVERY fp32 value. v + v is exact; fl(3v) is off by 0, 1/4 or 1/2 ulp of 4v's binade, and the half-ulp case needs
    #         an even mantissa of v, for which round-to-even picks 4v itself; 4v * 0.25 is exact.
    #   s = 4 for values of at most 20 significant bits (every partial sum k v, k <= 16, is exact). NOT for every value: the
    #         definition adds sequentially, and 16 rounded additions of fl(0.1) give 0.10000002 - two ulps up. That is what the
    #         definition says, so it is asserted here too (against the written-out loop), not wished away.
    rng = np.random.default_rng(7)
    anyv = np.concatenate([np.array([0.1, 0.7, 1.0, 3.3e-5, 255.0 / 256.0, 1e-40, 3e38 / 4], F), rng.uniform(0, 2, 2000).astype(F),
                           (rng.integers(1 << 23, 1 << 24, 2000) * 2.0 ** -23).astype(F)])
    short = (rng.integers(1, 1 << 20, 2000) * 2.0 ** rng.integers(-30, 4, 2000)).astype(F)
    for s, values in ((2, anyv), (4, short), (4, np.array([0.5, 0.75, 1.0, 2.0, 255.0 / 256.0], F))):
        x = np.repeat(np.repeat(values.reshape(-1, 1, 1), s * s, axis=1), 4, axis=2).reshape(-1, 4)   # one pixel per value: rows of s samples
        frame = np.ascontiguousarray(x.reshape(len(values), s, s, 4).transpose(1, 0, 2, 3)).reshape(-1, 4)  # width len(values) * s, height s
        got = resolve.box_filter(frame, len(values) * s, s)
        assert np.array_equal(bits(got), bits(np.repeat(values.reshape(-1, 1), 4, axis=1))), s
    tenth = np.full((16, 4), 0.1, F)
    assert np.array_equal(bits(resolve.box_filter(tenth, 4, 4)), bits(slow_box_filter(tenth, 4, 4)))
    assert resolve.box_filter(tenth, 4, 4)[0, 0] == np.nextafter(np.nextafter(F(0.1), F(1)), F(1))
    for s in (2, 3, 4):                                # w = 1 on every sample -> exactly 1 (9 * fl(1/9) rounds to 1)
        x = np.zeros((12 * 12, 4), F)
        x[:, 3] = 1.0
        assert np.all(resolve.box_filter(x, 12, s)[:, 3] == F(1.0)), s
    x = np.zeros((4 * 2, 4), F)                        # two 2x2 pixels: NaN / inf propagate within their own pixel and channel only
    x[1, 0] = np.nan
    x[4, 1] = np.inf
    x[2, 2] = np.inf
    x[7, 2] = -np.inf
    got = resolve.box_filter(x, 4, 2)
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[0, 2] == 0 and got[0, 3] == 0
    assert got[1, 0] == 0 and got[1, 1] == 0 and np.isnan(got[1, 2])      # inf + -inf


def test_box_filter_refuses_what_the_library_refuses():
    from opencl_raytracer_amd import resolve
    x = np.zeros((12 * 6, 4), F)
    for w, s in ((12, 5), (12, 0), (12, 4), (10, 3), (7, 2)):       # 6 rows % 4; 72 samples are no rows of 10 / 7
        with pytest.raises(ValueError):
            resolve.box_filter(x, w, s)
    assert resolve.pixels(72, 3) == 8 and resolve.pixels(72, 1) == 72


def test_supersampled_camera():
    assert camera.supersampled(48, 36, -31.17, 1)[:2] == (48, 36)
    for s in (2, 3, 4):
        z = camera.camera_z(36)
        w, h, sz = camera.supersampled(48, 36, z, s)
        assert (w, h) == (48 * s, 36 * s) and sz.dtype == F and sz == F(F(s) * z)
    with pytest.raises(ValueError):
        camera.supersampled(4, 4, -1.0, 5)
    rays = camera.grid_rays(48, 36, camera.camera_z(36))
    assert rays.tobytes() == camera.primary_rays(48, 36).tobytes()


# ---- 2. what a sample is -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [101, 102, 103])
@pytest.mark.parametrize("s", [2, 4])
def test_the_corner_samples_are_the_unsampled_frame(restatement, seed, s):
    """directions are not normalised and scaling by a power of two is exact: the a = b = 0 samples of the (s W, s H, s z) frame are
    the (W, H, z) frame bit for bit - a supersampled frame refines the picture the reference renders, it does not move it"""
    W, H, depth = 48, 36, 5
    objs, lights = random_scene(10, 8, 3, seed=seed, directional_lights=1)
    z = camera.camera_z(H)
    base = restatement[True].render("shade_and_reflect", objs, lights, camera.grid_rays(W, H, z), depth, want_aux=False)["out"]
    sw, sh, sz = camera.supersampled(W, H, z, s)
    fine = restatement[True].render("shade_and_reflect", objs, lights, camera.grid_rays(sw, sh, sz), depth, want_aux=False)["out"]
    corner = fine.reshape(sh, sw, 4)[::s, ::s].reshape(-1, 4)
    assert np.any(base[:, :3] != 0)
    assert np.array_equal(bits(corner), bits(base))


# ---- 3. the CPU backend --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_cpu_backend_filters_its_own_samples(s):
    from opencl_raytracer_amd import resolve
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    W, H = 16, 12
    objs, lights = random_scene(6, 5, 2, seed=77, directional_lights=1)
    sw, sh, sz = camera.supersampled(W, H, camera.camera_z(H), s)
    rays = camera.grid_rays(sw, sh, sz)
    samples = CPURaytracer(objs, lights, rays, 2).Render()
    got = CPURaytracer(objs, lights, rays, 2, supersample=s, sample_width=sw).Render()
    assert got.shape == (W * H, 4) and np.any(got[:, :3] != 0)
    assert np.array_equal(bits(got), bits(resolve.box_filter(samples, sw, s)))
    assert np.all(got[:, 3] == 1.0)
    with pytest.raises(ValueError):
        CPURaytracer(objs, lights, rays, 2, supersample=s, sample_width=sw + 1).Render()
    with pytest.raises(ValueError):
        CPURaytracer(objs, lights, rays, 0, kernel="hittest", supersample=s, sample_width=sw).Render()


def test_scene_tool_cpu_takes_ss(tmp_path):
    """scene_tool render --ss 2 ... cpu: the picture keeps its size, and it is the P3 of box_filter over the Python CPU backend's
    sample frame"""
    import subprocess
    from opencl_raytracer_amd import ppm, resolve, scene_loader
    from opencl_raytracer_amd.cpu_raytracer import CPURaytracer
    tool = ROOT / "opencl-raytracer_amd" / "host" / "scene_tool"
    if not tool.exists():
        import __graft_entry__
        __graft_entry__.build()
    scene = ROOT / "scenes" / "simpleSphere.txt"
    W, H, s = 32, 24, 2
    z = camera.camera_z(H)
    out = tmp_path / "ss.ppm"
    res = subprocess.run([str(tool), "render", str(scene), str(W), str(H), "2", str(out), f"{int(F(z).view(np.uint32)):08x}", "cpu", "--ss", str(s)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    objs, lights = scene_loader.load_scene(str(scene))
    sw, sh, sz = camera.supersampled(W, H, z, s)
    samples = CPURaytracer(objs, lights, camera.grid_rays(sw, sh, sz), 2).Render()
    want = ppm.format_p3(W, H, ppm.rgba_to_rgb(resolve.box_filter(samples, sw, s)))
    assert out.read_bytes() == want


# ---- 4. the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_and_wrapper_declare_the_new_symbols():
    from opencl_raytracer_amd import hip_raytracer
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in hip_raytracer.h"
        assert name in hip_raytracer.EXPORTS
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", text)
    assert "supersampled frames" in HEADER.read_text()


def test_library_exports_the_new_symbols_and_refuses_null():
    from opencl_raytracer_amd import hip_raytracer
    if not hip_raytracer.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(str(hip_raytracer.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libhip_raytracer.so does not export {name}"
    lib.rt_abi_version.restype = ctypes.c_int
    assert lib.rt_abi_version() == 3
    lib.rt_set_supersampling.restype = ctypes.c_int
    lib.rt_set_supersampling.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.rt_set_supersampling(None, 2) == -1                 # RT_ERR_INVALID_ARGUMENT, no device needed
    lib.rt_supersampling.restype = ctypes.c_uint32
    lib.rt_supersampling.argtypes = [ctypes.c_void_p]
    assert lib.rt_supersampling(None) == 0
    lib.rt_local_pixels.restype = ctypes.c_uint64
    lib.rt_local_pixels.argtypes = [ctypes.c_void_p]
    assert lib.rt_local_pixels(None) == 0
    lib.rt_multi_frame_pixels.restype = ctypes.c_uint64
    lib.rt_multi_frame_pixels.argtypes = [ctypes.c_void_p]
    assert lib.rt_multi_frame_pixels(None) == 0
    lib.rt_set_supersampling_multi.restype = ctypes.c_int
    lib.rt_set_supersampling_multi.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.rt_set_supersampling_multi(None, 2) == -1
    lib.rt_resolve_device.restype = ctypes.c_int
    lib.rt_resolve_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]
    assert lib.rt_resolve_device(None, None, 4, 4, 2, 0, None, None) == -1


# ---- 5. shards of whole pixel rows, and their exchange -------------------------------------------------------------------------
def test_whole_pixel_rows():
    from opencl_raytracer_amd import sharding
    assert [sharding.whole_pixel_rows(16, s) for s in (1, 2, 3, 4)] == [16, 16, 18, 16]
    assert [sharding.whole_pixel_rows(r, 3) for r in (1, 3, 4, 48)] == [3, 3, 6, 48]
    assert sharding.whole_pixel_rows(7, 2) == 8 and sharding.whole_pixel_rows(1, 4) == 4
    with pytest.raises(ValueError):
        sharding.whole_pixel_rows(0, 2)
    for s, rows in ((2, 16), (3, 16), (4, 5)):
        w = 12 * s
        tile = sharding.tile_rays_for_rows(w, sharding.whole_pixel_rows(rows, s))
        assert tile % (s * w) == 0 and tile // (s * s) == (w // s) * (sharding.whole_pixel_rows(rows, s) // s)


def _pixel_gather_worker(rank, world, port, s, sw, sh, tile_rows, result_path):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import helpers  # noqa: F401  (loads the package)
        from opencl_raytracer_amd import resolve, sharding
        from opencl_raytracer_amd.distributed import FrameGather
        n_rays = sw * sh
        tile_rays = sharding.tile_rays_for_rows(sw, sharding.whole_pixel_rows(tile_rows, s))
        n_pix, tile_pix = n_rays // (s * s), tile_rays // (s * s)
        fg = FrameGather(n_pix, tile_pix, 4, torch.device("cpu"))
        assert fg.local_rays == sharding.local_rays(n_rays, tile_rays, rank, world) // (s * s)
        # the sample frame every rank knows; a rank filters ITS tiles, the ragged last one padded with the background as rt_set_shard pads it
        samples = np.random.default_rng(5).uniform(0, 2, size=(n_rays, 4)).astype(np.float32)
        samples[:, 3] = 1.0
        off = 0
        for t in sharding.local_tiles(n_rays, tile_rays, rank, world):
            tile = np.zeros((tile_rays, 4), np.float32)
            tile[:, 3] = 1.0
            chunk = samples[t * tile_rays:(t + 1) * tile_rays]
            tile[:len(chunk)] = chunk
            fg.local[off:off + tile_pix] = torch.from_numpy(resolve.box_filter(tile, sw, s))
            off += tile_pix
        frame = fg.gather()
        if rank == 0:
            want = resolve.box_filter(samples, sw, s)
            ok = tuple(frame.shape) == (n_pix, 4) and np.array_equal(frame.numpy().view(np.uint32), want.view(np.uint32))
            Path(result_path).write_text("ok" if ok else "mismatch")
        else:
            assert frame is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("s,sw,sh,tile_rows", [(2, 16, 20, 7), (3, 18, 24, 4), (4, 16, 24, 16)])
def test_gather_assembles_a_frame_of_pixel_tiles(tmp_path, s, sw, sh, tile_rows):
    """2 ranks over gloo, tiles of whole pixel rows counted in pixels, a ragged last tile every time (20 rows in tiles of 8, 24 in
    tiles of 6 is even - 4 tiles -, 24 in tiles of 16): the frame on rank 0 is box_filter of the whole sample frame"""
    port = 33500 + (os.getpid() % 2000) + 11 * s
    result = tmp_path / "result.txt"
    mp.spawn(_pixel_gather_worker, args=(2, port, s, sw, sh, tile_rows, str(result)), nprocs=2, join=True)
    assert result.read_text() == "ok"
