"""Replaceable rays - the two executable definitions behind rt_set_rays_device / rt_set_rays (hip_raytracer.h).

ray_verdict(rays)  what the ray scan (csrc/rt_rays.hip) reports about a ray array: the predicates of rt_create's host loops,
                   in float32 with the same order of operations, and the box of the origins.
posed_rays(...)    a pinhole grid seen through a rotation, from a common origin: the rays of a panned, tilted, rolled or
                   moved camera, in a stated float32 order, so that a caller who computes them elsewhere (on the GPU) can
                   reproduce them bit for bit. rt_set_pose / rt_generate_rays_device (hip_raytracer.h, "posed cameras";
                   csrc/rt_raygen.hip; HIPRaytracer.set_pose, generate_rays) do: these rays, written on the device.
"""
from __future__ import annotations

import numpy as np

from .camera import grid_rays
from .records import RAY_DTYPE

F = np.float32


def ray_verdict(rays: np.ndarray) -> dict:
    """dir_w_zero, directions_in_domain, starts_ok (bool) and origin_lo / origin_hi (float32[3], None unless starts_ok).

    Per ray, float32, every operation rounded, left to right:
        direction.w == 0
        dd = (dx*dx + dy*dy) + dz*dz;  dd > 1e-30 and dd < 1e30        (a NaN fails)
        start.w == 1 and isfinite((sx + sy) + sz)                       (finite components whose sum overflows fail)
    and the numeric minimum / maximum of start.x, .y, .z (-0.0 and +0.0 are the same number)."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    d = rays["direction"].astype(F, copy=False)
    s = rays["start"].astype(F, copy=False)
    with np.errstate(all="ignore"):
        dd = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        dd = (dd + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        in_domain = bool(np.all((dd > F(1.0e-30)) & (dd < F(1.0e30))))
        ssum = ((s[:, 0] + s[:, 1]).astype(F) + s[:, 2]).astype(F)
        starts_ok = bool(np.all((s[:, 3] == F(1.0)) & np.isfinite(ssum)))
    out = dict(dir_w_zero=bool(np.all(d[:, 3] == F(0.0))), directions_in_domain=in_domain, starts_ok=starts_ok,
               origin_lo=None, origin_hi=None)
    if starts_ok and len(rays):
        out["origin_lo"] = s[:, :3].min(axis=0).astype(F)
        out["origin_hi"] = s[:, :3].max(axis=0).astype(F)
    return out


def posed_rays(width: int, height: int, z: float, rotation3x3, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The pinhole grid (width, height, z) - camera.grid_rays: direction (i - W/2, (H - j) - H/2, z) for work-item j W + i -
    with every direction multiplied by a float32 3 x 3 matrix M (row-major, M[r][c]) and every start set to `origin`:

        M = float32(rotation3x3);  d = the grid's direction
        direction[r] = fl(fl(fl(M[r][0] * d.x) + fl(M[r][1] * d.y)) + fl(M[r][2] * d.z)),   direction.w = 0
        start = (float32(origin), 1)

    every product and sum rounded to float32, nothing fused, left to right. With the identity and a zero origin the result is
    the grid itself, bit for bit (1 * x = x, x + 0 = x; a -0.0 cannot arise from the grid's x + 0)."""
    M = np.asarray(rotation3x3, dtype=np.float64).astype(F)
    if M.shape != (3, 3):
        raise ValueError("rotation3x3 must be a 3 x 3 matrix")
    rays = grid_rays(width, height, z)
    d = rays["direction"][:, :3].copy()
    out = np.empty_like(d)
    with np.errstate(all="ignore"):
        for r in range(3):
            acc = ((M[r, 0] * d[:, 0]).astype(F) + (M[r, 1] * d[:, 1]).astype(F)).astype(F)
            out[:, r] = (acc + (M[r, 2] * d[:, 2]).astype(F)).astype(F)
    rays["direction"][:, :3] = out
    rays["start"][:, :3] = np.asarray(origin, dtype=np.float64).astype(F)
    rays["start"][:, 3] = 1.0
    return rays
