"""Screen tiles of a posed camera - the executable definition behind the device builder (csrc/rt_tiles.hip).

pose_screen_tiles(spheres, width, height, z, M, origin)
    the depth-ordered tile lists wf_trace_primary_tiles walks for the rays of rays.posed_rays(width, height, z, M, origin):
    per 64 x 8 tile the objects whose registration sphere a ray of that tile can meet, each with a lower bound of the t it
    can report there, ascending by (key, index). csrc/rt_grid.h (ScreenTiles, "posed cameras") has the derivation; this file
    is the same arithmetic in numpy float64, in the order the device uses, and runs without a GPU.
pose_registration_spheres(bounds, grid_constants, origin)
    the registration spheres of a pose whose origin may lie OUTSIDE the grid's box (csrc/rt_tiles.hip: pose_spheres): the grid's
    own expressions (csrc/rt_grid_radii.h) with the farthest origin and the largest |origin| taken over the box and the pose's
    origin. pose_screen_tiles takes its output, with whole_r = 0.25 diag. grid_registration_spheres is the grid's own formula,
    object_bounds / grid_constants stand in for a context's bounds and constants, pose_within_reach is the FAR condition.
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
REFUSED_FAR = 1024        # a pose outside the grid's box whose origin is too far: 3e-6 (|o| + far) > 0.01 cell
REFUSED_SMALL = 2048      # a pose outside the grid's box on a frame of fewer than OUTSIDE_MIN_TILES tiles
OUTSIDE_MIN_TILES = 16    # 128 x 64 pixels


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


def pose_rects(spheres: np.ndarray, width: int, height: int, k: dict, whole_r: float = np.inf) -> dict:
    """Per object: class (0 none, 1 listed, 2 whole screen), tile rectangle x0, x1, y0, y1 (inclusive) and depth key - the
    device's tile_rects pass. `k` = pose_constants(...) of a pose that was not refused. A listed object whose radius is above
    `whole_r` is a whole-screen entry (a pose outside the grid's box: 0.25 of the box's diagonal)."""
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
    with np.errstate(invalid="ignore"):
        cls = np.where(listed & (R > whole_r), 2, cls)
    edges = dict(c0=c0, c1=c1, r0=r0, r1=r1)
    return dict(cls=cls, x0=x0, x1=x1, y0=y0, y1=y1, key=key, covered=covered, edges=edges)


def pose_screen_tiles(spheres, width: int, height: int, z: float, M, origin=(0.0, 0.0, 0.0), grid_in_use: bool = True,
                      whole_r: float = np.inf) -> dict:
    """The table of one pose. `spheres`: n x 4 float64 registration spheres (centre, R; R = inf: always tested, R < 0 or NaN:
    never hit - neither is in any list). Returns enabled, refused (REFUSED_* bits), eps, pad, tiles_x, tiles_y, col_shift and -
    when enabled - tile_start (uint32[tiles + 1]), entries (uint32[n_entries + n_global + 1, 2]: {index, key bits}, a tile's
    ascending by (key, index), the global list behind the last tile's, one zeroed entry behind that), n_entries, n_global,
    global_begin, max_list, and `rects` (pose_rects' per-object result). For a pose outside the grid's box `spheres` are
    pose_registration_spheres(...) and `whole_r` is 0.25 of the box's diagonal."""
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
    rects = pose_rects(s, width, height, k, whole_r)
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


# ---- poses outside the grid's box ---------------------------------------------------------------------------------------------------
def object_bounds(objects: np.ndarray) -> np.ndarray:
    """n x 6 float64 - centre, radius, kappa^2, type - of OBJECT_DTYPE records, for callers without a context (a context's own:
    HIPRaytracer.object_bounds()): bounding_spheres' centre and geometric radius, kappa = sigma_max / sigma_min of A^-1."""
    out = np.zeros((len(objects), 6))
    out[:, :4] = bounding_spheres(objects)
    for i, o in enumerate(objects):
        m = np.asarray(o["mvInverse"], dtype=np.float64).reshape(16)
        A = np.array([[m[0], m[4], m[8]], [m[1], m[5], m[9]], [m[2], m[6], m[10]]])
        out[i, 5] = int(o["type"])
        if int(o["type"]) <= 1:
            sv = np.linalg.svd(np.linalg.inv(A), compute_uv=False)
            out[i, 4] = (sv[0] / sv[-1]) ** 2
    return out


def grid_constants(bounds, origin_lo=(0.0, 0.0, 0.0), origin_hi=(0.0, 0.0, 0.0), cells_per_object: float = 3.0) -> dict:
    """A TEST STAND-IN for a context's constants (HIPRaytracer.grid_constants() returns the real ones; nothing in the library reads
    this): build_grid's constants (csrc/rt_scene.cpp) for a scene of these bounds whose create-time origins fill origin_lo .. origin_hi,
    WITHOUT the cell refinement of crowded scenes and with K2 = 1 as a placeholder:
    the box - the origins united with the bounds padded by 1 % -, its diagonal, the largest |corner| S_max, and the cell edge before
    the refinement build_grid applies to crowded scenes (a context's own: HIPRaytracer.grid_constants())."""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    lo, hi = np.array(origin_lo, dtype=np.float64), np.array(origin_hi, dtype=np.float64)
    ok = np.isfinite(b[:, 3])
    pad = b[ok, 3] * 1.01
    lo = np.minimum(lo, (b[ok, :3] - pad[:, None]).min(axis=0)) if ok.any() else lo
    hi = np.maximum(hi, (b[ok, :3] + pad[:, None]).max(axis=0)) if ok.any() else hi
    ext = hi - lo
    diag = float(np.sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]))
    corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
    S_max = float(np.sqrt((corners * corners).sum(axis=1)).max())
    e = np.maximum(ext, 1e-6)
    cell = float(np.cbrt(e[0] * e[1] * e[2] / (cells_per_object * len(b))))
    cell = max(cell, float(ext.max()) / 256.0)
    return dict(box_lo=lo, box_hi=hi, cell=cell, diag=diag, S_max=S_max, K2=1.0)


def _registration(b: np.ndarray, g: dict, D2: np.ndarray, S) -> np.ndarray:
    """csrc/rt_grid_radii.h: registration_terms' rg, in its order of operations."""
    c, r, k2, ty = b[:, :3], b[:, 3], b[:, 4], b[:, 5]
    with np.errstate(all="ignore"):
        kap = np.sqrt(k2)
        cl = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        a2 = r * r * (1.0 + 2e-6)
        L = 2.2e-6 * kap * (S + cl) + 2e-6 * k2 * np.sqrt(D2)
        reg = np.sqrt(a2 + 3e-6 * k2 * D2) + L
        tri = r * (1.0 + 1e-6) + 2e-6 * np.sqrt(D2) + 1e-6 * (S + cl)
        reg = np.where(ty == 2, tri, reg)
        return reg * (1.0 + 1e-6) + 0.01 * g["cell"]


def _farthest_corner2(b: np.ndarray, g: dict) -> np.ndarray:
    lo, hi = np.asarray(g["box_lo"], dtype=np.float64), np.asarray(g["box_hi"], dtype=np.float64)
    D2 = np.zeros(len(b))
    for a in range(3):
        d = np.maximum(np.abs(b[:, a] - lo[a]), np.abs(hi[a] - b[:, a]))
        D2 = D2 + d * d
    return D2


def _classes(b: np.ndarray, rg: np.ndarray, g: dict) -> np.ndarray:
    """grid_radii's classes: a bound of -inf is never hit (-1), one without a finite radius - or a sphere above a quarter of the
    box's diagonal - is tested by every ray (+inf: the always-list)."""
    r = b[:, 3]
    with np.errstate(invalid="ignore"):
        rg = np.where(~np.isfinite(rg) | (rg > 0.25 * g["diag"]), np.inf, rg)
    rg = np.where(~np.isfinite(r), np.inf, rg)
    return np.where(r == -np.inf, -1.0, rg)


def grid_registration_spheres(bounds, grid_constants: dict) -> np.ndarray:
    """n x 4 float64: the spheres build_grid registers these bounds with (grid_radii, csrc/rt_scene.cpp): every ray origin inside
    the box, i.e. at most D - the farthest corner - from the centre and S_max from the world's origin."""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    rg = _registration(b, grid_constants, _farthest_corner2(b, grid_constants), grid_constants["S_max"])
    return np.column_stack([b[:, :3], _classes(b, rg, grid_constants)])


def pose_registration_spheres(bounds, grid_constants: dict, origin, grid_spheres=None) -> np.ndarray:
    """n x 4 float64: (c, rg') for the rays of a pose at `origin` (fp32, converted exactly) - grid_radii's expressions with D^2
    replaced by max(D^2, |o - c|^2) and S_max by max(S_max, |o|). An origin inside the box reproduces the grid's spheres bit for
    bit. Objects the grid has in its always-list (+inf) or can never hit (negative) stay what they are: `grid_spheres`, a live
    context's own (HIPRaytracer.grid_spheres()), decides where given, else grid_registration_spheres. An rg' that is not finite
    becomes the largest double; pose_screen_tiles(..., whole_r = 0.25 diag) makes it, and every rg' above whole_r, a whole-screen
    entry."""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    g = grid_constants
    o = np.asarray(origin, dtype=np.float64).astype(F).astype(np.float64)
    base = grid_registration_spheres(b, g) if grid_spheres is None else np.asarray(grid_spheres, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        d = o[None, :] - b[:, :3]
        oc2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        D2 = _farthest_corner2(b, g)
        D2 = np.where(D2 < oc2, oc2, D2)
        ol = float(np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]))
        S = ol if g["S_max"] < ol else g["S_max"]
        rg = _registration(b, g, D2, S)
        rg = np.where(np.isfinite(rg), rg, np.finfo(np.float64).max)
        keep = ~((base[:, 3] >= 0) & (base[:, 3] != np.inf))
    out = base.copy()
    out[:, 3] = np.where(keep, base[:, 3], rg)
    return out


GROWTH_CELLS = 0.9        # (pose_growth_ok)


def pose_growth_ok(bounds, grid_constants: dict, origin, grid_spheres=None) -> bool:
    """Not enforced by the library (DESIGN.md 4.1 names the limit): does no listed object's rg' exceed its rg by more than GROWTH_CELLS
    cells, so that every point a primary ray can report - inside (c, rg') - lies inside the grid's own box (padded by rg + one cell)?"""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    base = grid_registration_spheres(b, grid_constants) if grid_spheres is None else np.asarray(grid_spheres, dtype=np.float64).reshape(-1, 4)
    mine = pose_registration_spheres(b, grid_constants, origin, grid_spheres=base)
    listed = (base[:, 3] >= 0) & np.isfinite(base[:, 3])
    return bool(np.all(mine[listed, 3] <= base[listed, 3] + GROWTH_CELLS * grid_constants["cell"]))


def pose_within_reach(grid_constants: dict, origin) -> bool:
    """The FAR condition: 3e-6 (|o| + far) <= 0.01 cell, far = the largest distance from o to a corner of the box."""
    g = grid_constants
    o = np.asarray(origin, dtype=np.float64).astype(F).astype(np.float64)
    lo, hi = np.asarray(g["box_lo"], dtype=np.float64), np.asarray(g["box_hi"], dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.maximum(np.abs(o - lo), np.abs(hi - o))
        lhs = 3e-6 * (float(np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])) + float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    return bool(np.isfinite(lhs) and lhs <= 0.01 * g["cell"])
