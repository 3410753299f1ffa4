"""ASCII PPM sink. Mirrors `PPMExporter::ExportP3(path, width, height, vector<float> rgb)`
(PPMExporter.hpp:8, PPMExporter.cpp:7-30): header "P3\\n<W> <H>\\n255\\n", then one pixel per line,
each channel `min(255, (int)floorf(v * 255.f))` (no lower clamp), separated by single spaces.

8-bit frames (hip_raytracer.h, "8-bit frames"): `quantise_bytes` is the executable form of the byte a channel becomes on
the device; `format_p3` / `ExportP3` take such a `uint8` array as well, `format_p6` / `ExportP6` write the binary flavour.
"""
from __future__ import annotations

import numpy as np


def rgba_to_rgb(rgba: np.ndarray) -> np.ndarray:
    """float4 framebuffer (Render()'s return, IRaytracer.hpp:13) -> packed RGB floats, stride 3."""
    rgba = np.asarray(rgba, dtype=np.float32).reshape(-1, 4)
    return np.ascontiguousarray(rgba[:, :3]).reshape(-1)


def quantise(rgb: np.ndarray) -> np.ndarray:
    v = np.floor(np.asarray(rgb, dtype=np.float32) * np.float32(255.0))
    return np.minimum(255, v.astype(np.int64))


def quantise_bytes(values: np.ndarray) -> np.ndarray:
    """The byte a channel value becomes (the specification of csrc/rt_pack.hip): p = v * 255.0f as one fp32 multiplication,
    f = floorf(p); NaN or f < 0 -> 0, f >= 255 -> 255, else (uint8_t)f. Equal to `quantise` wherever that yields 0..255."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(values, dtype=np.float32) * np.float32(255.0))
        f = np.where(f >= np.float32(0.0), f, np.float32(0.0))      # NaN and negatives (-inf too) fail the comparison
        f = np.where(f >= np.float32(255.0), np.float32(255.0), f)  # +inf too
    return f.astype(np.uint8)


def _levels(width: int, height: int, pixels: np.ndarray) -> np.ndarray:
    """(W*H, 3) integer levels from float RGB (stride 3) or from a uint8 frame of stride 3 or 4 (the fourth byte is dropped)."""
    pixels = np.asarray(pixels)
    if pixels.dtype == np.uint8:
        stride = pixels.size // (width * height) if width * height else 3
        if stride not in (3, 4) or pixels.size != width * height * stride:
            raise ValueError("a uint8 frame is width * height pixels of 3 or 4 bytes")
        return pixels.reshape(width * height, stride)[:, :3]
    return quantise(pixels).reshape(width * height, 3)


def format_p3(width: int, height: int, rgb: np.ndarray) -> bytes:
    q = _levels(width, height, rgb)
    body = "".join(f"{r} {g} {b}\n" for r, g, b in q.tolist())
    return (f"P3\n{width} {height}\n255\n" + body).encode("ascii")


def format_p6(width: int, height: int, pixels: np.ndarray) -> bytes:
    """Binary PPM: header "P6\\n<W> <H>\\n255\\n", then 3 bytes per pixel. Float input goes through `quantise_bytes`."""
    pixels = np.asarray(pixels)
    if pixels.dtype != np.uint8:
        pixels = quantise_bytes(pixels)
    return f"P6\n{width} {height}\n255\n".encode("ascii") + np.ascontiguousarray(_levels(width, height, pixels)).tobytes()


def ExportP3(out_file: str, width: int, height: int, pixel_data) -> None:
    data = np.asarray(pixel_data)
    with open(out_file, "wb") as f:
        f.write(format_p3(width, height, data if data.dtype == np.uint8 else data.astype(np.float32)))


def ExportP6(out_file: str, width: int, height: int, pixel_data) -> None:
    with open(out_file, "wb") as f:
        f.write(format_p6(width, height, np.asarray(pixel_data)))
