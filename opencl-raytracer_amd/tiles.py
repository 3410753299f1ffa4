"""Screen tiles of a posed camera - the executable definition behind the device builder (csrc/rt_tiles.hip).

pose_screen_tiles(spheres, width, height, z, M, origin)
    the depth-ordered tile lists wf_trace_primary_tiles walks for the rays of rays.posed_rays(width, height, z, M, origin):
    per 64 x 8 tile the objects whose registration sphere a ray of that tile can meet, each with a lower bound of the t it
    can report there, ascending by (key, index). csrc/rt_grid.h (ScreenTiles, "posed cameras") has the derivation; this file
    is the same arithmetic in numpy float64, in the order the device uses, and runs without a GPU.
bounding_spheres(objects)
    bounding spheres of OBJECT_DTYPE records (centre -A^-1 b, radius r0 sigma_max(A^-1)), geometric or with rt_grid.h's
    registration bound, for callers that have no context to ask (HIPRaytracer.grid_spheres() returns the spheres a live
    context registered its objects with).
"""
from __future__ import annotations

import numpy as np

F = np.float32
U = 2.0 ** -24            # unit roundoff of float32
SLACK = 2.0 ** -40        # relative slack for the builder's own double arithmetic
MAX_GLOBAL = 64           # whole-screen objects a table may hold
MAX_LIST = 1024           # entries one workgroup sorts in 8 KB of LDS
COL_SHIFT = 6             # tiles are 64 x 8 pixels: a posed frame's work-items are in linear order

# rt_tiles_info_t::refused, a bit per reason
REFUSED_NO_GRID = 1       # the grid does not serve the rays in use (origin outside its box, literal loops, no grid)
REFUSED_Z = 2             # z is not < 0
REFUSED_MATRIX = 4        # M is not finite or is singular
REFUSED_EPS = 8           # eps >= |z| / 2 or pad > 1
REFUSED_WIDTH = 16        # width % 64 != 0
REFUSED_GLOBAL = 32       # more than 64 whole-screen objects
REFUSED_BUDGET = 64       # more (object, tile) pairs than 256 n + 4096
REFUSED_LIST = 128        # a tile's list is longer than 1024 entries
REFUSED_TILES = 256       # more than 2^20 tiles
REFUSED_KNOB = 512        # RT_POSE_TILES said no


def sigma_max(N: np.ndarray) -> float:
    """sqrt of the largest eigenvalue of N N^T in closed form (object_bound's, csrc/rt_scene.cpp): padded by 1e-6 relative,
    never above the Frobenius bound or below a third of it."""
    S = N @ N.T
    fro2 = float(np.sum(N * N))
    lam_max = fro2
    q = (S[0, 0] + S[1, 1] + S[2, 2]) / 3.0
    p1 = S[0, 1] ** 2 + S[0, 2] ** 2 + S[1, 2] ** 2
    p2 = (S[0, 0] - q) ** 2 + (S[1, 1] - q) ** 2 + (S[2, 2] - q) ** 2 + 2.0 * p1
    pp = np.sqrt(p2 / 6.0)
    if pp > 0 and np.isfinite(pp):
        B = (S - q * np.eye(3)) / pp
        r = float(np.clip(np.linalg.det(B) / 2.0, -1.0, 1.0))
        lam = q + 2.0 * pp * np.cos(np.arccos(r) / 3.0)
        if np.isfinite(lam) and lam > 0:
            lam_max = lam * (1.0 + 1e-6)
    elif pp == 0:
        lam_max = q * (1.0 + 1e-6)
    lam_max = min(lam_max, fro2)
    lam_max = max(lam_max, fro2 / 3.0)
    return float(np.sqrt(lam_max))


def pose_constants(width: int, height: int, z: float, M, origin) -> dict:
    """What the host hands the device for one pose: N = M^-1, sigma_max(N), eps, pad, z - eps, and the refusals that need no
    object (refused = 0: the objects decide)."""
    M32 = np.asarray(M, dtype=np.float64).astype(F)
    o32 = np.asarray(origin, dtype=np.float64).astype(F)
    Md = M32.astype(np.float64)
    od = o32.astype(np.float64)
    zd = float(F(z))
    out = dict(refused=0, N=None, sigma=0.0, eps=0.0, pad=0.0, zme=0.0, z=zd, origin=od, M=Md)
    if width % (1 << COL_SHIFT) != 0:
        out["refused"] |= REFUSED_WIDTH
    if not (zd < 0):
        out["refused"] |= REFUSED_Z
    tiles_x, tiles_y = width >> COL_SHIFT, (height + 7) // 8
    if tiles_x * tiles_y > (1 << 20):
        out["refused"] |= REFUSED_TILES
    det = float(np.linalg.det(Md)) if np.all(np.isfinite(Md)) else float("nan")
    norm2 = float(np.sum(Md * Md))
    if not np.all(np.isfinite(od)) or not np.isfinite(det) or not (abs(det) > 1e-12 * norm2 ** 1.5):
        out["refused"] |= REFUSED_MATRIX
        return out
    N = np.linalg.inv(Md)
    if not np.all(np.isfinite(N)):
        out["refused"] |= REFUSED_MATRIX
        return out
    out["N"] = N
    out["sigma"] = sigma_max(N)
    if out["refused"] & REFUSED_Z:
        return out
    vmax = np.array([width / 2.0, height / 2.0, abs(zd)])
    # |v' - v|_inf <= eps: three roundings per component of d = fl(M v) (3.1 u covers gamma_3), carried through N; the second
    # term is what products that underflow can add (2^-149 absolute each)
    eps = 3.1 * U * float(np.max(np.abs(N) @ (np.abs(Md) @ vmax))) + 2.0 ** -140 * float(np.max(np.sum(np.abs(N), axis=1)))
    out["eps"] = eps
    if not np.isfinite(eps) or eps >= abs(zd) / 2.0:
        out["refused"] |= REFUSED_EPS
        return out
    pad = eps * (1.0 + max(width, height) / (2.0 * abs(zd))) / (1.0 - eps / abs(zd))
    out["pad"] = pad
    out["zme"] = zd - eps
    if not (pad <= 1.0):
        out["refused"] |= REFUSED_EPS
    return out


def _next_below(x: np.ndarray) -> np.ndarray:
    return np.nextafter(x.astype(F), F(-np.inf))


def _next_above(x: np.ndarray) -> np.ndarray:
    return np.nextafter(x.astype(F), F(np.inf))


def pose_rects(spheres: np.ndarray, width: int, height: int, k: dict) -> dict:
    """Per object: class (0 none, 1 listed, 2 whole screen), tile rectangle x0, x1, y0, y1 (inclusive) and depth key - the
    device's tile_rects pass. `k` = pose_constants(...) of a pose that was not refused."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    n = len(s)
    N, od, z = k["N"], k["origin"], k["z"]
    R = s[:, 3]
    with np.errstate(all="ignore"):
        usable = (R >= 0) & (R != np.inf)
        d = s[:, :3] - od
        cp = np.empty((n, 3))
        for r in range(3):
            cp[:, r] = (N[r, 0] * d[:, 0] + N[r, 1] * d[:, 1]) + N[r, 2] * d[:, 2]
        sig1 = k["sigma"] * (1.0 + SLACK)
        absk = SLACK * k["sigma"]
        o1 = (abs(od[0]) + abs(od[1])) + abs(od[2])
        Rp = R * sig1 + absk * (((np.abs(s[:, 0]) + np.abs(s[:, 1])) + np.abs(s[:, 2])) + o1)
        cz = cp[:, 2]
        finite = np.isfinite(cp).all(axis=1) & np.isfinite(Rp)
        behind = finite & (cz - Rp >= 0)
        reaches = ~finite | (cz + Rp >= 0)

        def extent(cu):
            a = cz * cz - Rp * Rp
            b = -2.0 * z * cu * cz
            c = (z * z) * (cu * cu - Rp * Rp)
            disc = b * b - 4.0 * a * c
            ok = (a > 0) & (disc >= 0)
            sq = np.sqrt(np.where(ok, disc, 0.0))
            u0 = (-b - sq) / (2.0 * a)
            u1 = (-b + sq) / (2.0 * a)
            lo, hi = np.minimum(u0, u1), np.maximum(u0, u1)
            lo = (lo - (1.0 + 1e-6 * np.abs(lo))) - k["pad"]
            hi = (hi + (1.0 + 1e-6 * np.abs(hi))) + k["pad"]
            lo = np.where(ok & ~reaches, _next_below(lo).astype(np.float64), -np.inf)
            hi = np.where(ok & ~reaches, _next_above(hi).astype(np.float64), np.inf)
            return lo, hi

        xlo, xhi = extent(cp[:, 0])
        ylo, yhi = extent(cp[:, 1])
        half_w, half_h, H = float(F(width) / F(2)), float(F(height) / F(2)), float(height)
        c0, c1 = xlo + half_w, xhi + half_w
        r0, r1 = (H - half_h) - yhi, (H - half_h) - ylo
        cx0 = np.where(c0 >= 0, np.floor(c0), 0.0)      # (a NaN keeps the screen's edge)
        ry0 = np.where(r0 >= 0, np.floor(r0), 0.0)
        cx1 = np.where(c1 <= width - 1, np.ceil(c1), width - 1.0)
        ry1 = np.where(r1 <= height - 1, np.ceil(r1), height - 1.0)
        on_screen = (cx0 <= cx1) & (ry0 <= ry1)
        listed = usable & ~behind & on_screen
        x0 = np.where(listed, cx0, 0).astype(np.int64) >> COL_SHIFT
        x1 = np.where(listed, cx1, 0).astype(np.int64) >> COL_SHIFT
        y0 = np.where(listed, ry0, 0).astype(np.int64) >> 3
        y1 = np.where(listed, ry1, 0).astype(np.int64) >> 3
        kd = (cz + Rp) / k["zme"]
        kd = kd - np.abs(kd) * SLACK
        key = np.where(np.isnan(kd), F(-np.inf), _next_below(kd)).astype(F)
    tiles_x, tiles_y = width >> COL_SHIFT, (height + 7) // 8
    covered = np.where(listed, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    cls = np.where(listed, 1, 0)
    if tiles_x * tiles_y > 1:
        cls = np.where(listed & (covered == tiles_x * tiles_y), 2, cls)
    edges = dict(c0=c0, c1=c1, r0=r0, r1=r1)
    return dict(cls=cls, x0=x0, x1=x1, y0=y0, y1=y1, key=key, covered=covered, edges=edges)


def pose_screen_tiles(spheres, width: int, height: int, z: float, M, origin=(0.0, 0.0, 0.0), grid_in_use: bool = True) -> dict:
    """The table of one pose. `spheres`: n x 4 float64 registration spheres (centre, R; R = inf: always tested, R < 0 or NaN:
    never hit - neither is in any list). Returns enabled, refused (REFUSED_* bits), eps, pad, tiles_x, tiles_y, col_shift and -
    when enabled - tile_start (uint32[tiles + 1]), entries (uint32[n_entries + n_global + 1, 2]: {index, key bits}, a tile's
    ascending by (key, index), the global list behind the last tile's, one zeroed entry behind that), n_entries, n_global,
    global_begin, max_list, and `rects` (pose_rects' per-object result)."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    n = len(s)
    k = pose_constants(width, height, z, M, origin)
    tiles_x, tiles_y = width >> COL_SHIFT, (height + 7) // 8
    out = dict(enabled=False, refused=k["refused"], eps=k["eps"], pad=k["pad"], tiles_x=tiles_x, tiles_y=tiles_y,
               col_shift=COL_SHIFT, n_entries=0, n_global=0, max_list=0)
    if not grid_in_use or n == 0:
        out["refused"] |= REFUSED_NO_GRID
    if out["refused"]:
        return out
    rects = pose_rects(s, width, height, k)
    out["rects"] = rects
    cls = rects["cls"]
    glob = np.nonzero(cls == 2)[0]
    total = int(rects["covered"][cls == 1].sum())
    n_tiles = tiles_x * tiles_y
    counts = np.zeros(n_tiles, dtype=np.int64)
    out["n_global"] = len(glob)
    out["n_entries"] = total
    if len(glob) > MAX_GLOBAL:
        out["refused"] |= REFUSED_GLOBAL
    if total > 256 * n + 4096:
        out["refused"] |= REFUSED_BUDGET
        return out
    pairs_obj, pairs_tile = [], []
    for i in np.nonzero(cls == 1)[0]:
        ys, xs = np.mgrid[rects["y0"][i]:rects["y1"][i] + 1, rects["x0"][i]:rects["x1"][i] + 1]
        t = (ys * tiles_x + xs).ravel()
        pairs_tile.append(t)
        pairs_obj.append(np.full(len(t), i, dtype=np.int64))
    po = np.concatenate(pairs_obj) if pairs_obj else np.zeros(0, dtype=np.int64)
    pt = np.concatenate(pairs_tile) if pairs_tile else np.zeros(0, dtype=np.int64)
    np.add.at(counts, pt, 1)
    out["max_list"] = int(counts.max()) if n_tiles else 0
    if out["max_list"] > MAX_LIST:
        out["refused"] |= REFUSED_LIST
    if out["refused"]:
        return out
    key = rects["key"]
    order = np.lexsort((po, key[po], pt))           # by tile, then key, then index (-0.0 == 0.0: the index decides)
    po = po[order]
    start = np.zeros(n_tiles + 1, dtype=np.uint32)
    start[1:] = np.cumsum(counts)
    entries = np.zeros((total + len(glob) + 1, 2), dtype=np.uint32)
    entries[:total, 0] = po
    entries[:total, 1] = key[po].view(np.uint32)
    entries[total:total + len(glob), 0] = glob
    out.update(enabled=True, tile_start=start, entries=entries, global_begin=total)
    return out


def bounding_spheres(objects: np.ndarray, reach: float | None = None) -> np.ndarray:
    """n x 4 float64 (centre, radius) of unit spheres (type 0) and unit boxes (type 1) instanced by mvInverse (column-major, as
    the records store it): centre -A^-1 b, radius r0 sigma_max(A^-1). Other types: radius -inf (never hit).

    reach = None: the geometric radius. reach = the largest distance of a ray origin from the world's origin: the radius an
    object is REGISTERED with for such rays, by the bound at the top of csrc/rt_grid.h evaluated the way build_grid does
    (u_eff = 2e-7, dist = |c| + reach):
        sqrt(R^2 (1 + 8u) + 14 u kappa^2 dist^2) + 10.4 u kappa (reach + |c|) + 9 u kappa^2 dist
    - the surface plus what the reference's fp32 arithmetic can add to a reported t. (A context's own radii also carry the
    walk's 0.01 cell; HIPRaytracer.grid_spheres() returns those.)"""
    out = np.zeros((len(objects), 4))
    u = 2.0e-7
    for i, o in enumerate(objects):
        m = np.asarray(o["mvInverse"], dtype=np.float64).reshape(16)
        A = np.array([[m[0], m[4], m[8]], [m[1], m[5], m[9]], [m[2], m[6], m[10]]])
        b = np.array([m[12], m[13], m[14]])
        t = int(o["type"])
        if t > 1:
            out[i, 3] = -np.inf
            continue
        inv = np.linalg.inv(A)
        sv = np.linalg.svd(inv, compute_uv=False)
        c = -inv @ b
        R = (1.0 if t == 0 else np.sqrt(0.75)) * sv[0]
        if reach is not None:
            kappa, cl = sv[0] / sv[-1], float(np.linalg.norm(c))
            dist = cl + reach
            R = np.sqrt(R * R * (1.0 + 8.0 * u) + 14.0 * u * kappa ** 2 * dist ** 2) + 10.4 * u * kappa * (reach + cl) + 9.0 * u * kappa ** 2 * dist
        out[i, :3] = c
        out[i, 3] = R
    return out
