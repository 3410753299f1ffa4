"""Replaceable rays - the two executable definitions behind rt_set_rays_device / rt_set_rays (hip_raytracer.h).

ray_verdict(rays)  what the ray scan (csrc/rt_rays.hip) reports about a ray array: the predicates of rt_create's host loops,
                   in float32 with the same order of operations, and the box of the origins.
query_route(...)   which of a ray query's rays (hip_raytracer.h, "ray queries"; csrc/rt_query.hip) the grid serves and which run the
                   ordered loop over all objects: the kernel's per-ray predicate, in float32 with the same order of operations.
query_shade_route(...)  the same for a shaded query (hip_raytracer.h, "shaded queries"; csrc/rt_query_shade.hip): the route of each
                   primary ray, and which paths run the literal loops.
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


def inward_box(box_lo, box_hi):
    """The float64 box box_lo .. box_hi (rays_info()) as float32 numbers that lie INSIDE it: lo rounded up, hi rounded down - what
    the query kernels compare origins with, so that an origin the double box excludes is never admitted."""
    lo64, hi64 = np.asarray(box_lo, dtype=np.float64), np.asarray(box_hi, dtype=np.float64)
    with np.errstate(all="ignore"):
        lo, hi = lo64.astype(F), hi64.astype(F)
        lo = np.where(lo.astype(np.float64) < lo64, np.nextafter(lo, F(np.inf)), lo).astype(F)
        hi = np.where(hi.astype(np.float64) > hi64, np.nextafter(hi, F(-np.inf)), hi).astype(F)
    return lo, hi


def query_route(rays: np.ndarray, box_lo, box_hi) -> np.ndarray:
    """bool per ray: True - the grid serves the ray of a query, False - it runs the ordered brute-force loop over all objects.

    box_lo / box_hi are rays_info()'s (float64[3]); None for a context whose grid serves no query: every ray is False. That is a
    context without a grid (grid_built == 0), one created with literal=True (RT_FLAG_LITERAL), and one that holds a degenerate
    instance (a singular or non-finite mvInverse) - there the result depends on the order of the loop, which only the ordered loop
    follows.
    Per ray, float32, every operation rounded, left to right - True iff all of
        every one of the eight components is finite
        start.w == 1 and direction.w == 0
        dd = (dx*dx + dy*dy) + dz*dz;  dd > 1e-30 and dd < 1e30
        lo[a] <= start[a] <= hi[a] for a = x, y, z, with (lo, hi) = inward_box(box_lo, box_hi)."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    if box_lo is None or box_hi is None:
        return np.zeros(len(rays), dtype=bool)
    lo, hi = inward_box(box_lo, box_hi)
    d = rays["direction"].astype(F, copy=False)
    s = rays["start"].astype(F, copy=False)
    with np.errstate(all="ignore"):
        finite = np.isfinite(s).all(axis=1) & np.isfinite(d).all(axis=1)
        dd = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        dd = (dd + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        in_domain = (dd > F(1.0e-30)) & (dd < F(1.0e30))
        inside = ((s[:, :3] >= lo) & (s[:, :3] <= hi)).all(axis=1)
    return finite & (s[:, 3] == F(1.0)) & (d[:, 3] == F(0.0)) & in_domain & inside


def query_in_domain(rays: np.ndarray) -> np.ndarray:
    """bool per ray: the DOMAIN part of query_route - every component finite, start.w == 1, direction.w == 0, dd in (1e-30, 1e30) -
    without the box. float32, every operation rounded, left to right."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    d = rays["direction"].astype(F, copy=False)
    s = rays["start"].astype(F, copy=False)
    with np.errstate(all="ignore"):
        finite = np.isfinite(s).all(axis=1) & np.isfinite(d).all(axis=1)
        dd = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        dd = (dd + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        in_domain = (dd > F(1.0e-30)) & (dd < F(1.0e30))
    return finite & (s[:, 3] == F(1.0)) & (d[:, 3] == F(0.0)) & in_domain


def query_shade_route(rays: np.ndarray, box_lo, box_hi, literal: bool = False, mask=None) -> dict:
    """The route of a shaded query's PRIMARY rays and the kind of their paths: a dict of bool arrays, one entry per ray -

        "traced"   the ray is traced at all (its `mask` entry is not negative; no mask: every ray)
        "grid"     traced, and query_route(rays, box_lo, box_hi) admits it: the grid walk finds its primary hit
        "brute"    traced, and not: the ordered loop over all objects does
        "literal"  traced, and its whole path runs the literal loops (the forward light loop, closest-hit shadow tests, no dead-ray
                   elimination): the context is literal (`literal`: created with literal=True, a degenerate instance, or
                   device_opencl's predicate on the lights) or the ray fails query_in_domain

    so that n_grid, n_brute and n_literal of query_shade_info() are their sums. box_lo / box_hi as for query_route (None: the grid
    serves no query). A primary ray that fails only the box test is "brute" and not "literal": the brute-force loop for that one ray,
    the default path behind it. Every LATER ray of a path - shadow, reflection - is routed by query_route's predicate again, by the
    lane that traces it; those rays start on surfaces, which lie inside the box."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    n = len(rays)
    traced = np.ones(n, dtype=bool) if mask is None else (np.asarray(mask).reshape(-1) >= 0)
    if len(traced) != n:
        raise ValueError("mask: one entry per ray")
    grid = query_route(rays, box_lo, box_hi) & traced
    lit = (np.ones(n, dtype=bool) if literal else ~query_in_domain(rays)) & traced
    return {"traced": traced, "grid": grid, "brute": traced & ~grid, "literal": lit}


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
