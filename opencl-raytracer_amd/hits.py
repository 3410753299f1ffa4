"""hits - the record stage of a hit-record query (hip_raytracer.h, "hit-record queries") in numpy, and the reflection chain.

hit_records(objects, rays, t, index): what raycast() leaves in the HitRecord of winner index[i] at time t[i], and the next ray of the
reflection chain, in float32 with ONE IEEE operation per step: the association is that of row4, materialise, normalize3 and
reflection_ray in csrc/rt_device.h, and nothing is fused - so this is the executable definition of the record stage under
RT_FLAG_UNFUSED, bit for bit (HIPRaytracer(..., fused=False).query_hits). A triangle winner (type 2, the extension of DESIGN.md
section 11; only a G-buffer frame delivers one, the queries refuse such contexts) takes materialise()'s type-2 branch: the point on
the ray itself and normalize(e1 x e2) of the record's edges, `fused=True` giving the point's single rounding. The default mode contracts the multiply-adds the OpenCL
front-end contracts (CPURaytracer.query_hits is its definition), RT_FLAG_DEVICE_OPENCL additionally uses the device's normalize().

chain(query, rays, bounces): follow a reflection chain with the mask, so that a miss is never traced again.
"""
from __future__ import annotations

import numpy as np

from .records import OBJECT_DTYPE, RAY_DTYPE, rays_of

F = np.float32


def scene_is_affine(objects) -> bool:
    """rt_create's predicate: every sphere / box has bottom rows (0, 0, 0, 1) exactly in mv and mvInverse - materialise() then
    takes w from the ray instead of fetching the two rows."""
    o = objects[objects["type"] <= 1]
    bottom = np.array([0.0, 0.0, 0.0, 1.0], dtype=F)
    return bool(all((o[m].reshape(len(o), 16)[:, 3::4] == bottom).all() for m in ("mv", "mvInverse")))


def _row4(m, r, x, y, z, w):
    """One row of transform(): column-major m[:, 16], row r - m[4 + r] * y first, then x, z, w added on (rt_device.h: row4)."""
    t = m[:, 4 + r] * y
    t = m[:, r] * x + t
    t = m[:, 8 + r] * z + t
    t = m[:, 12 + r] * w + t
    return t


def _normalize3(x, y, z):
    s = x * x
    s = s + y * y
    s = s + z * z
    length = np.sqrt(s)
    return x / length, y / length, z / length


def _fma(a, b, c):
    """fl(a * b + c) with ONE rounding, for float32 arrays: the product of two float32 is exact in float64, and the float64 sum
    is rounded to float32 by way of round-to-odd (the sum's error term decides the sticky bit), so no double rounding."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # two_sum: p + c == s + err exactly
    u = s.view(np.uint64) if s.ndim else np.array([s]).view(np.uint64)
    u = u.copy()
    finite = np.isfinite(s) & (err != 0) & ((u & np.uint64(1)) == 0)
    # round to odd: an inexact sum whose last bit is even moves one ulp towards the error
    up = finite & ((err > 0) == (s > 0))
    down = finite & ~up
    u[up] += np.uint64(1)
    u[down] -= np.uint64(1)
    fix = np.where(finite & (s == 0), s, u.view(np.float64).reshape(s.shape))
    return fix.astype(F)


def triangle_edges(objects):
    """(v0, e1, e2) float32[n, 3] of type-2 records as the kernels hold them (rt_device.h: HotObject of a triangle): the vertices are
    columns 0, 1, 2 of mv (x, y, z in elements 4 k .. 4 k + 2), e1 = v1 - v0 and e2 = v2 - v0 in float32."""
    mv = objects["mv"].reshape(-1, 16).astype(F)
    v0, v1, v2 = mv[:, 0:3], mv[:, 4:7], mv[:, 8:11]
    return v0, (v1 - v0).astype(F), (v2 - v0).astype(F)


def hit_records(objects, rays, t, index, affine=None, fused=False):
    """point float32[n, 4], normal float32[n, 4] (w = 0) and reflected RAY_DTYPE[n] as a dict, for winner index[i] at time t[i];
    zero records where index[i] < 0. `affine`: the scene's flag (None: scene_is_affine(objects)). A triangle winner: point =
    t * d + s per component (w included) - product then sum, or with `fused` one single-rounded fma, the fused modes' - and normal =
    normalize(e1 x e2), never contracted; `fused` touches nothing else."""
    objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
    rays = rays_of(rays)
    t = np.asarray(t, dtype=F).reshape(-1)
    index = np.asarray(index, dtype=np.int32).reshape(-1)
    n = len(rays)
    if len(t) != n or len(index) != n:
        raise ValueError("hit_records: t and index have one entry per ray")
    affine = scene_is_affine(objects) if affine is None else bool(affine)
    point, normal, reflected = np.zeros((n, 4), dtype=F), np.zeros((n, 4), dtype=F), np.zeros(n, dtype=RAY_DTYPE)
    sel = np.nonzero(index >= 0)[0]
    if sel.size == 0:
        return {"point": point, "normal": normal, "reflected": reflected}
    o = objects[index[sel]]
    inv, mv, kind = o["mvInverse"].reshape(-1, 16).astype(F), o["mv"].reshape(-1, 16).astype(F), o["type"]
    s, d, T = rays["start"][sel].astype(F), rays["direction"][sel].astype(F), t[sel]
    zero, k001 = F(0.0), F(0.001)
    with np.errstate(all="ignore"):
        so = [_row4(inv, r, s[:, 0], s[:, 1], s[:, 2], s[:, 3]) for r in range(3)]
        do = [_row4(inv, r, d[:, 0], d[:, 1], d[:, 2], d[:, 3]) for r in range(3)]
        # an affine scene takes w from the ray - where the ray's x, y, z are finite (then 0*x + 0*y + 0*z + 1*w IS w); a ray with an
        # inf or a NaN in it goes through the bottom rows like the reference's
        short = affine & np.isfinite(s[:, :3]).all(axis=1) & np.isfinite(d[:, :3]).all(axis=1)
        sw = np.where(short, s[:, 3], _row4(inv, 3, s[:, 0], s[:, 1], s[:, 2], s[:, 3]))
        dw = np.where(short, d[:, 3], _row4(inv, 3, d[:, 0], d[:, 1], d[:, 2], d[:, 3]))
        px, py, pz, pw = T * do[0] + so[0], T * do[1] + so[1], T * do[2] + so[2], T * dw + sw
        lim = F(0.4998)
        face = [np.where(p > lim, F(1.0), np.where(p < -lim, F(-1.0), zero)).astype(F) for p in (px, py, pz)]
        sphere = kind == 0
        ox, oy, oz = (np.where(sphere, p, f).astype(F) for p, f in zip((px, py, pz), face))
        P = [_row4(mv, r, px, py, pz, pw) for r in range(3)]
        Pw = np.where(short, pw, _row4(mv, 3, px, py, pz, pw))
        nx, ny, nz = _normalize3(*[_row4(mv, r, ox, oy, oz, zero) for r in range(3)])
        k2 = ((d[:, 0] * nx + d[:, 1] * ny) + d[:, 2] * nz) * F(-2.0)
        rx, ry, rz = k2 * nx + d[:, 0], k2 * ny + d[:, 1], k2 * nz + d[:, 2]
        ux, uy, uz = _normalize3(rx, ry, rz)
        point[sel] = np.stack([P[0], P[1], P[2], Pw], axis=1)
        normal[sel] = np.stack([nx, ny, nz, np.zeros_like(nx)], axis=1)
        start = np.stack([ux * k001 + P[0], uy * k001 + P[1], uz * k001 + P[2], zero * k001 + Pw], axis=1)
        direction = np.stack([rx, ry, rz, np.zeros_like(rx)], axis=1)
    reflected["start"][sel] = start
    reflected["direction"][sel] = direction
    tri = kind == 2
    if tri.any():   # materialise()'s type-2 branch (rt_device.h)
        k = sel[tri]
        _, e1, e2 = triangle_edges(o[tri])
        s3, d3, T3 = s[tri], d[tri], T[tri]
        with np.errstate(all="ignore"):
            if fused:
                P = np.stack([_fma(T3, d3[:, c], s3[:, c]) for c in range(4)], axis=1)
            else:
                P = np.stack([T3 * d3[:, c] + s3[:, c] for c in range(4)], axis=1)
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            nx, ny, nz = _normalize3(nx, ny, nz)
        point[k] = P.astype(F)
        normal[k] = np.stack([nx, ny, nz, np.zeros_like(nx)], axis=1)
        # (the reflected ray of a triangle winner is not part of any call: the record stays zero)
        reflected["start"][k] = 0
        reflected["direction"][k] = 0
    return {"point": point, "normal": normal, "reflected": reflected}


def chain(query, rays, bounces):
    """Follow a reflection chain: `query(rays, mask)` is a query_hits (HIPRaytracer's, CPURaytracer's, or a lambda around one); bounce
    k + 1 traces bounce k's reflected rays with bounce k's index as its mask, so a ray that has missed stays a zero record and is
    never traced again (its zero ray would take the ordered brute-force loop). Returns the list of the bounces' results."""
    out, mask = [], None
    for _ in range(int(bounces)):
        hit = query(rays, mask)
        out.append(hit)
        rays, mask = hit["reflected"], hit["index"]
    return out
