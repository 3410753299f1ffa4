"""Supersampled frames - the executable form of hip_raytracer.h's definition ("supersampled frames").

A context with supersampling factor s renders its w x h SAMPLE grid as ever and delivers (w/s) x (h/s) pixels: the s x s
samples of a pixel added in fp32 in (b, a) order - sample row b outer, column a inner, starting from sample (0, 0) - and
multiplied ONCE by fl(1 / s^2). The order is part of the definition: csrc/rt_resolve.hip, host/CPURaytracer and this file
add in the same order, so that their results can be compared bit for bit. `box_filter` is what every test compares against.
"""
from __future__ import annotations

import numpy as np

F = np.float32
FACTORS = (1, 2, 3, 4)


def check_factor(s) -> int:
    if int(s) != s or int(s) not in FACTORS:
        raise ValueError(f"the supersampling factor is one of {FACTORS}, not {s!r}")
    return int(s)


def box_filter(frame: np.ndarray, sample_width: int, s: int) -> np.ndarray:
    """(n_samples, C) float32 samples in row-major order, rows of `sample_width` -> (n_samples / s^2, C) float32 pixels.
    Every channel by itself (w is filtered like a colour), explicit fp32 additions in (b, a) order, one multiplication by
    fl(1 / s^2); NaN and infinities propagate as IEEE says. s = 1 returns the samples (a copy)."""
    s = check_factor(s)
    frame = np.asarray(frame, dtype=F)
    if frame.ndim != 2:
        raise ValueError("a frame is (n_samples, channels)")
    if s == 1:
        return frame.copy()
    n, ch = frame.shape
    w = int(sample_width)
    if w <= 0 or n % w or w % s or (n // w) % s:
        raise ValueError(f"{n} samples are not whole rows of {w} with width and height multiples of {s}")
    grid = frame.reshape(n // w // s, s, w // s, s, ch)          # [j, b, i, a, channel]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = grid[:, 0, :, 0, :].copy()
        for b in range(s):
            for a in range(s):
                if a or b:
                    acc = (acc + grid[:, b, :, a, :]).astype(F)   # one rounded fp32 addition per sample
        out = (acc * (F(1.0) / F(s * s))).astype(F)
    return np.ascontiguousarray(out.reshape(-1, ch))


def pixels(n_samples: int, s: int) -> int:
    """Pixels that n_samples samples become (rt_local_pixels, rt_multi_frame_pixels)."""
    s = check_factor(s)
    return int(n_samples) // (s * s)
