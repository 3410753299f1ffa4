"""No GPU: the specification of the 8-bit frame (ppm.quantise_bytes, the executable form of hip_raytracer.h's table and of
csrc/rt_pack.hip), its agreement with the reference's PPM expression on every colour fixture, the PPM sinks fed with bytes,
the new symbols of the C ABI, and the exchange of uint8 tiles (distributed.FrameGather over gloo)."""
import ctypes
import hashlib
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import fixture_names, load_fixture

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "hip_raytracer.h"
NEW_SYMBOLS = ("rt_packed_pixel_bytes", "rt_pack_device", "rt_render_device_packed", "rt_render_packed", "rt_render_multi_packed")
F = np.float32


def crafted_values():
    """(value, expected byte) pairs: the table of hip_raytracer.h ("8-bit frames") written out by hand. For k / 255 and its
    neighbours the expected level is floor(v * 255) evaluated exactly in float64 and then rounded to fp32 the way the one fp32
    multiplication rounds it (a float64 product of two fp32 numbers is exact, so its fp32 rounding IS the fp32 product)."""
    inf, nan = F(np.inf), F(np.nan)
    tiny = F(np.finfo(np.float32).tiny)
    denorm = np.uint32(1).view(F)            # smallest positive denormal
    below_256_255 = np.nextafter(F(256.0) / F(255.0), F(0))
    table = [(nan, 0), (np.uint32(0xffc00001).view(F), 0), (np.uint32(0x7f800001).view(F), 0),   # quiet, negative, signalling NaN
             (inf, 255), (-inf, 0), (F(0.0), 0), (F(-0.0), 0),
             (F(-1.0), 0), (F(-1e-30), 0), (F(-0.5), 0), (F(-3.4e38), 0), (-denorm, 0), (-tiny, 0),
             (denorm, 0), (tiny, 0), (F(1e-39), 0),
             (F(1.0), 255), (below_256_255, 255), (F(256.0) / F(255.0), 255), (F(2.0), 255), (F(3.4e38), 255),
             (F(0.5), 127), (np.nextafter(F(1.0), F(0)), 254), (F(1.0) / F(255.0), 1)]
    for k in range(256):
        v = F(k) / F(255.0)
        for x in (np.nextafter(v, F(-1)), v, np.nextafter(v, F(2))):
            p = F(np.float64(x) * 255.0)                       # the one fp32 multiplication
            want = 0 if not p >= 0 else min(255, int(np.floor(np.float64(p))))
            table.append((x, want))
    vals = np.array([t[0] for t in table], dtype=F)
    want = np.array([t[1] for t in table], dtype=np.uint8)
    return vals, want


def random_bit_patterns(n, seed=20261016):
    """n fp32 values drawn uniformly over ALL bit patterns: every exponent, so denormals, infinities and NaNs are in it"""
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(F)


def test_quantise_bytes_table():
    from opencl_raytracer_amd import ppm
    vals, want = crafted_values()
    got = ppm.quantise_bytes(vals)
    assert got.dtype == np.uint8 and got.shape == vals.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(vals[i], int(got[i]), int(want[i])) for i in bad[:10]]
    # the levels 0 .. 255 are all reached, and k / 255 itself never lands below k - 1
    assert set(want.tolist()) == set(range(256))


def test_quantise_bytes_is_the_reference_expression_where_that_is_a_byte():
    from opencl_raytracer_amd import ppm
    x = random_bit_patterns(1 << 20)
    with np.errstate(all="ignore"):
        ref = ppm.quantise(x)
    got = ppm.quantise_bytes(x)
    valid = (ref >= 0) & (ref <= 255)
    assert valid.sum() > 1000 and (~valid).sum() > 1000
    assert np.array_equal(got[valid], ref[valid].astype(np.uint8))
    assert set(np.unique(got[~valid]).tolist()) <= {0, 255}
    assert np.all(got[np.isnan(x)] == 0)


def _colour_fixtures():
    return [n for n in fixture_names() if int(np.load(ROOT / "tests" / "golden" / f"{n}.npz")["kernel"]) != 0]


def test_every_colour_fixture_quantises_like_the_reference():
    """quantise_bytes == quantise on the oracle's expected frame of every colour fixture, both flavours, NO pixel excluded: a
    future fixture with a NaN or negative channel must fail here, not be skipped."""
    from opencl_raytracer_amd import ppm
    names = _colour_fixtures()
    assert len(names) >= 81
    pixels = 0
    clamped = {"out_fused": 0, "out_unfused": 0}
    for name in names:
        fx = load_fixture(name)
        for key in clamped:
            rgb = np.asarray(fx[key], dtype=F)
            assert rgb.ndim == 2 and rgb.shape[1] == 3
            ref = ppm.quantise(rgb)
            assert ref.min(initial=0) >= 0 and ref.max(initial=0) <= 255, name
            assert np.array_equal(ppm.quantise_bytes(rgb), ref.astype(np.uint8)), name
            clamped[key] += int(np.any(np.floor(rgb * F(255.0)) > 255, axis=1).sum())   # min(255, .) really cuts
        pixels += len(fx["out_fused"])
    assert pixels >= 259584
    if len(names) == 81:   # today's fixture set: the figures of the issue
        assert pixels == 259584 and clamped == {"out_fused": 471, "out_unfused": 472}


def test_config1_p3_and_p6_from_bytes():
    from opencl_raytracer_amd import ppm
    fx = load_fixture("scene_simpleSphere_256_shade_and_reflect")
    for key in ("out_fused", "out_unfused"):
        q = ppm.quantise_bytes(fx[key])
        assert q.shape == (256 * 256, 3)
        p3 = ppm.format_p3(256, 256, q)
        assert len(p3) == 397825 and hashlib.md5(p3).hexdigest() == "28365bd12a502710be0c9a9a1a8057a9"
        assert p3 == ppm.format_p3(256, 256, fx[key].reshape(-1))      # the float route, as before
        rgba = np.concatenate([q, np.full((len(q), 1), 255, np.uint8)], axis=1)
        assert ppm.format_p3(256, 256, rgba) == p3                      # stride 4: the fourth byte is dropped
        p6 = ppm.format_p6(256, 256, q)
        head = b"P6\n256 256\n255\n"
        assert p6.startswith(head) and p6[len(head):] == q.tobytes()
        assert ppm.format_p6(256, 256, rgba) == p6 and ppm.format_p6(256, 256, fx[key].reshape(-1)) == p6


def test_export_functions_write_the_formatted_bytes(tmp_path):
    from opencl_raytracer_amd import ppm
    q = np.arange(24, dtype=np.uint8).reshape(8, 3)
    ppm.ExportP3(str(tmp_path / "a.ppm"), 4, 2, q)
    ppm.ExportP6(str(tmp_path / "b.ppm"), 4, 2, q)
    assert (tmp_path / "a.ppm").read_bytes() == ppm.format_p3(4, 2, q)
    assert (tmp_path / "b.ppm").read_bytes() == b"P6\n4 2\n255\n" + q.tobytes()
    with pytest.raises(ValueError):
        ppm.format_p3(4, 2, q[:7])


def test_header_exports_and_library_agree_on_the_new_symbols():
    from opencl_raytracer_amd import hip_raytracer
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in hip_raytracer.h"
        assert name in hip_raytracer.EXPORTS
    assert re.search(r"RT_PIXEL_RGBA8\s*=\s*1\b", text) and re.search(r"RT_PIXEL_RGB8\s*=\s*2\b", text)
    assert re.search(r"#define\s+RT_ABI_VERSION\s+3\b", text)
    assert (hip_raytracer.PIXEL_RGBA8, hip_raytracer.PIXEL_RGB8) == (1, 2)


def test_library_exports_the_new_symbols_and_answers_pixel_sizes():
    from opencl_raytracer_amd import hip_raytracer
    if not hip_raytracer.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(str(hip_raytracer.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"libhip_raytracer.so does not export {name}"
    lib.rt_abi_version.restype = ctypes.c_int
    assert lib.rt_abi_version() == 3
    lib.rt_packed_pixel_bytes.restype = ctypes.c_size_t
    lib.rt_packed_pixel_bytes.argtypes = [ctypes.c_int]
    assert [lib.rt_packed_pixel_bytes(f) for f in (1, 2, 0, 3, -1)] == [4, 3, 0, 0, 0]   # callable without a device
    # NULL handles are refused, not dereferenced
    lib.rt_render_packed.restype = ctypes.c_int
    lib.rt_render_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert lib.rt_render_packed(None, 1, None) == -1
    lib.rt_pack_device.restype = ctypes.c_int
    lib.rt_pack_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.rt_pack_device(None, None, 0, 1, None, None) == -1


def test_pixel_format_names():
    from opencl_raytracer_amd.hip_raytracer import pixel_format
    assert pixel_format("rgba8") == 1 and pixel_format("RGB8") == 2 and pixel_format(2) == 2
    with pytest.raises(ValueError):
        pixel_format("bgra8")


def _gather_worker(rank, world, port, tile_rays, n_rays, channels, result_path):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import helpers  # noqa: F401  (loads the package)
        from opencl_raytracer_amd import sharding
        from opencl_raytracer_amd.distributed import FrameGather
        fg = FrameGather(n_rays, tile_rays, channels, torch.device("cpu"), dtype=torch.uint8)
        assert fg.local_rays == sharding.local_rays(n_rays, tile_rays, rank, world)
        assert fg.local.dtype == torch.uint8 and fg.poison == 0x5A
        # the frame every rank knows: byte (7 i + 3 c + 1) mod 251 for pixel i, channel c; a rank fills in its own tiles, packed
        # back to back as rt_set_shard packs them (the ragged last tile's padding stays 0)
        whole = ((7 * np.arange(n_rays)[:, None] + 3 * np.arange(channels)[None, :] + 1) % 251).astype(np.uint8)
        off = 0
        for t in sharding.local_tiles(n_rays, tile_rays, rank, world):
            chunk = whole[t * tile_rays:(t + 1) * tile_rays]
            fg.local[off:off + len(chunk)] = torch.from_numpy(chunk)
            off += tile_rays
        frame = fg.gather()
        if rank == 0:
            ok = frame.dtype == torch.uint8 and tuple(frame.shape) == (n_rays, channels) and np.array_equal(frame.numpy(), whole)
            Path(result_path).write_text("ok" if ok else "mismatch")
        else:
            assert frame is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("world,tile_rays,n_rays", [(2, 32, 16 * 10 + 5), (3, 32, 16 * 14 + 9), (3, 64, 100)])
def test_gather_assembles_a_byte_frame(tmp_path, world, tile_rays, n_rays, channels):
    """uint8 tiles, 4 and 3 channels, worlds 2 and 3, a ragged last tile every time; (3, 64, 100): a rank with no tile at all"""
    port = 31500 + (os.getpid() % 2000) + tile_rays + 7 * world + channels
    result = tmp_path / "result.txt"
    mp.spawn(_gather_worker, args=(world, port, tile_rays, n_rays, channels, str(result)), nprocs=world, join=True)
    assert result.read_text() == "ok"
