"""Light tiles - the executable definition (numpy, float64) of what csrc/rt_light_tiles.hip builds on the device for
rt_set_lights, and csrc/rt_light_setup.cpp's build_light_tiles on the host for rt_create (csrc/rt_grid.h: LightTiles).

Shadow rays towards one positional light L all lie on lines through L. In the light-local frame (x', y', z') - a signed
permutation of p - L in which every object lies at z' < 0 - an object's registration sphere (c, r0), padded by kPad, covers a
rectangle in the gnomonic coordinates (u, v) = (x', y') / -z'; a T x T table over the bounding rectangle lists, per tile, the
objects that reach it, ordered by a key that is a lower bound on the distance from L to anything of the object.

The table is a culling structure: the builders pad every rectangle (1e-5 (1 + |x|) per bound, 0.01 tile when binning), so a built
table lies between two rectangles defined here - MUST (the exact tangent span, no padding, no slack) and MAY (padded by
2e-5 (1 + |x|), 0.02 tile of slack) - and a test can hold any builder against them without asking for its last bits.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
K_FRONT = 0.05            # every object at least this far in front of the plane through the light (beyond its radius + kPad)
ANGLE_LIMIT = 1.5533      # rad: a tangent beyond 89 degrees of the axis is no usable tangent
MAX_LIST = 1024           # entries one workgroup sorts in 8 KB of LDS
MAX_CANDIDATES = 7        # tile counts of the halving rule

# rt_light_tiles_info_t::refused (include/hip_raytracer.h: RT_LTILES_REFUSED_*)
REFUSED_NO_GRID = 0x1     # no grid, literal loops, kernel not shade_and_reflect, no lights, objects on the always-list
REFUSED_LIGHT = 0x2       # the last light is directional or not finite
REFUSED_PLANE = 0x4       # no separating axis-aligned plane through the light
REFUSED_TANGENT = 0x8     # an object without a usable tangent
REFUSED_BOUNDS = 0x10     # the rectangles' bounds are empty or not finite
REFUSED_BUDGET = 0x20     # more than 64 n + 4096 pairs, or 32-bit byte offsets exceeded
REFUSED_LIST = 0x40       # a list longer than 1024 entries
REFUSED_BLOCKS = 0x80     # block form impossible
REFUSED_KNOB = 0x100      # switched off in the environment


def _usable(spheres: np.ndarray) -> np.ndarray:
    r = spheres[:, 3]
    return (r >= 0) & np.isfinite(r)


def light_constants(spheres: np.ndarray, light) -> dict:
    """kPad, cut_pad, and the projection axis and sign (axis None: no separating plane) for registration spheres (n x 4 float64:
    centre, radius; inf or negative: in no list) and a light position (3 floats, taken as float32)."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    L = np.asarray(light, dtype=np.float64)[:3].astype(F).astype(np.float64)
    ok = _usable(s)
    c, r = s[ok, :3], s[ok, 3]
    coord_max = float(np.sqrt((L * L).sum()))
    reach_max = 0.0
    if len(c):
        coord_max = max(coord_max, float((np.sqrt((c * c).sum(axis=1)) + r).max()))
        reach_max = max(reach_max, float((np.sqrt(((c - L) ** 2).sum(axis=1)) + r).max()))
    scale = 4e-7 * (2.0 * coord_max + reach_max)
    k_pad = max(1e-3, scale)
    axis, sign, best = None, 0, 0.0
    for a in range(3):
        for sg in (-1.0, 1.0):
            if not len(c):
                continue
            clear = float((sg * (c[:, a] - L[a]) - r).min()) - k_pad
            if clear > K_FRONT and math.isfinite(clear) and clear > best:
                best, axis, sign = clear, a, int(sg)
    return {"light": L, "k_pad": k_pad, "cut_pad": float(F(max(1e-4, scale))), "axis": axis, "sign": sign,
            "coord_max": coord_max, "reach_max": reach_max}


def _span(cx, cz, r, pad):
    """tan of [phi - alpha, phi + alpha] for the disc (cx, cz; r) seen from the origin, each bound padded by pad (1 + |x|);
    ok False: no usable tangent."""
    rho = np.sqrt(cx * cx + cz * cz)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = np.arctan2(cx, -cz)
        alpha = np.arcsin(np.minimum(1.0, r / rho))
        ok = (rho > r) & (np.abs(phi) + alpha < ANGLE_LIMIT)
        lo, hi = np.tan(phi - alpha), np.tan(phi + alpha)
    lo = lo - pad * (1.0 + np.abs(lo))
    hi = hi + pad * (1.0 + np.abs(hi))
    return lo, hi, ok


def spans(spheres: np.ndarray, k: dict, pad: float) -> dict:
    """Per object the (u, v) span of (c, r0 + kPad) with the given relative padding, `listed` (usable radius) and `ok` (usable
    tangents in both directions)."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    listed = _usable(s)
    az = k["axis"]
    ax, ay = (az + 1) % 3, (az + 2) % 3
    q = s[:, :3] - k["light"]
    qz = -k["sign"] * q[:, az]
    r = np.where(listed, s[:, 3], 0.0) + k["k_pad"]
    u0, u1, oku = _span(q[:, ax], qz, r, pad)
    v0, v1, okv = _span(q[:, ay], qz, r, pad)
    return {"u0": u0, "u1": u1, "v0": v0, "v1": v1, "listed": listed, "ok": oku & okv}


def tile_candidates(n: int, factor: float = 1.6) -> list:
    """The tile counts the halving rule can choose from: T0 = clamp(1.6 sqrt(n), 16, 1024), T0 / 2, ... down to the first <= 16."""
    T = int(min(1024.0, max(16.0, factor * math.sqrt(float(n)))))
    out = [T]
    while T > 16 and len(out) < MAX_CANDIDATES:
        T //= 2
        out.append(T)
    return out


def tile_rule(n: int, total_of) -> int:
    """T as a function of the pair total: the first candidate whose total (total_of(T)) is at most 24 n + 4096, else the last."""
    cands = tile_candidates(n)
    for T in cands:
        if total_of(T) <= 24 * n + 4096 or T <= 16:
            return T
    return cands[-1]


def tile_frame(U0: float, U1: float, V0: float, V1: float, T: int):
    """(u0, v0, inv_du, inv_dv) as float32 for bounds U0..V1 and T tiles per axis - the builders' rule."""
    du = (U1 - U0) / T * (1.0 + 1e-6)
    dv = (V1 - V0) / T * (1.0 + 1e-6)
    ninf = F(-np.inf)
    return np.nextafter(F(U0), ninf), np.nextafter(F(V0), ninf), F(1.0 / du), F(1.0 / dv)


def _tiles(lo, hi, base, inv, T, slack):
    a = np.floor((lo - float(base)) * float(inv) - slack)
    b = np.floor((hi - float(base)) * float(inv) + slack)
    return np.clip(a, 0, T - 1).astype(np.int64), np.clip(b, 0, T - 1).astype(np.int64)


def rectangles(spheres: np.ndarray, k: dict, u0, v0, inv_du, inv_dv, T: int) -> dict:
    """Per object the MUST and the MAY rectangle in tile units (a0, a1, b0, b1 inclusive; columns from u, rows from v) for the
    table (u0, v0, inv_du, inv_dv, T). MUST: the exact tangent span of (c, r0 + kPad), no padding, no slack. MAY: the span padded
    by 2e-5 (1 + |x|), 0.02 tile of slack. `listed`: the object is in the table at all."""
    m = spans(spheres, k, 0.0)
    y = spans(spheres, k, 2e-5)
    out = {"listed": m["listed"] & m["ok"]}
    for name, sp, slack in (("must", m, 0.0), ("may", y, 0.02)):
        a0, a1 = _tiles(sp["u0"], sp["u1"], u0, inv_du, T, slack)
        b0, b1 = _tiles(sp["v0"], sp["v1"], v0, inv_dv, T, slack)
        out[name] = np.stack([a0, a1, b0, b1], axis=1)
    return out


def pair_total(rect: np.ndarray, listed: np.ndarray) -> int:
    r = rect[listed]
    return int(((r[:, 1] - r[:, 0] + 1) * (r[:, 3] - r[:, 2] + 1)).sum())


def keys(spheres: np.ndarray, k: dict) -> np.ndarray:
    """Per object the float32 key: |c - L| - (r0 + kPad), scaled by 1 - 1e-6, then one float below."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    q = s[:, :3] - k["light"]
    d = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) - (s[:, 3] + k["k_pad"])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.nextafter((d * (1.0 - 1e-6)).astype(F), F(-np.inf))


def lattice_decode(q16: np.ndarray, lat_lo, lat_step) -> np.ndarray:
    """The centre a block entry decodes to: fma(float(q), lat_step, lat_lo) in float32, per component."""
    q = np.asarray(q16).astype(np.longdouble)
    return (q * np.longdouble(F(lat_step)) + np.asarray(lat_lo, dtype=F).astype(np.longdouble)).astype(F)


def block_radius(spheres: np.ndarray, pre: np.ndarray, lat_lo, lat_step, alpha: float, box_diagonal: float) -> np.ndarray:
    """Per object the exact block-form radius wq: the pre-test radius |pre| widened by the centre's quantisation error d on the
    16-bit lattice, with the cross term of the distance-dependent tolerance:
        w'^2 = (w + d)^2 + 2 d sqrt(a) D + a (2 d D + d^2),   wq = w' (1 + 2e-6)."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    lo = np.asarray(lat_lo, dtype=F).astype(np.float64)
    step = float(F(lat_step))
    u = np.floor((s[:, :3] - lo) / step + 0.5)
    dec = lattice_decode(u, lat_lo, lat_step).astype(np.float64)
    d = np.sqrt(((s[:, :3] - dec) ** 2).sum(axis=1))
    w = np.abs(np.asarray(pre, dtype=F).astype(np.float64))
    a, D = float(alpha), float(box_diagonal)
    w2 = (w + d) * (w + d) + 2.0 * d * math.sqrt(a) * D + a * (2.0 * d * D + d * d)
    return np.sqrt(w2) * (1.0 + 2e-6)


def unpack_entries(entries: np.ndarray, info: dict) -> dict:
    """What the kernels decode from a block entry's two words (read_light_tiles' columns 1 and 2): centre, radius, key."""
    lo, hi = entries[:, 1].astype(np.uint32), entries[:, 2].astype(np.uint32)
    q = np.stack([lo & 0xffff, lo >> 16, hi & 0xffff], axis=1)
    centre = lattice_decode(q, info["lat_lo"], info["lat_step"])
    r8, k8 = (hi >> 16) & 0xff, hi >> 24
    return {"index": entries[:, 0].astype(np.int64), "centre": centre, "radius": r8.astype(F) * F(info["rstep"]),
            "key": k8.astype(F) * F(info["kstep"]), "q": q, "r8": r8, "k8": k8}


def build(spheres: np.ndarray, light, directional: bool = False, rect: str = "must") -> dict:
    """The table of the definition for one light: refusal bits, constants, T, the tile frame, and per tile the list of objects
    (ascending by (key, index)) whose `rect` rectangle ("must" or "may") holds the tile. The bounds and T follow the builders'
    rule (spans padded by 1e-5 (1 + |x|), 0.01 tile of slack)."""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    n = len(s)
    out = {"refused": 0, "lists": None}
    pos = np.asarray(light, dtype=np.float64)
    if directional or (len(pos) > 3 and pos[3] == 0.0) or not np.isfinite(F(pos[0]) + F(pos[1]) + F(pos[2])):
        out["refused"] = REFUSED_LIGHT
        return out
    k = light_constants(s, pos)
    out.update(k)
    if k["axis"] is None:
        out["refused"] = REFUSED_PLANE
        return out
    b = spans(s, k, 1e-5)
    if np.any(b["listed"] & ~b["ok"]):
        out["refused"] = REFUSED_TANGENT
        return out
    on = b["listed"]
    if not on.any():
        out["refused"] = REFUSED_BOUNDS
        return out
    U0, U1, V0, V1 = b["u0"][on].min(), b["u1"][on].max(), b["v0"][on].min(), b["v1"][on].max()
    if not (U1 > U0 and V1 > V0 and np.isfinite(U0 + U1 + V0 + V1)):
        out["refused"] = REFUSED_BOUNDS
        return out

    def builder_total(T):
        u0, v0, iu, iv = tile_frame(U0, U1, V0, V1, T)
        a0, a1 = _tiles(b["u0"], b["u1"], u0, iu, T, 0.01)
        b0, b1 = _tiles(b["v0"], b["v1"], v0, iv, T, 0.01)
        return pair_total(np.stack([a0, a1, b0, b1], axis=1), on)

    T = tile_rule(n, builder_total)
    total = builder_total(T)
    out.update({"T": T, "n_entries": total, "bounds": (U0, U1, V0, V1)})
    if total > 64 * n + 4096 or total * 32 >= 0xffffffff:
        out["refused"] = REFUSED_BUDGET
        return out
    u0, v0, iu, iv = tile_frame(U0, U1, V0, V1, T)
    out.update({"u0": u0, "v0": v0, "inv_du": iu, "inv_dv": iv})
    rc = rectangles(s, k, u0, v0, iu, iv, T)
    key = keys(s, k)
    out["rect"], out["key"] = rc, key
    lists = [[] for _ in range(T * T)]
    for i in np.nonzero(rc["listed"])[0]:
        a0, a1, b0, b1 = rc[rect][i]
        for row in range(b0, b1 + 1):
            for col in range(a0, a1 + 1):
                lists[row * T + col].append(int(i))
    for lst in lists:
        lst.sort(key=lambda i: (float(key[i]), i))
    out["lists"] = lists
    out["max_list"] = max(len(lst) for lst in lists)
    # the length that counts for the refusal is the builder's (padded) list: MAY bounds it from above, MUST from below
    if rect == "must" and out["max_list"] > MAX_LIST:
        out["refused"] = REFUSED_LIST
    return out


def tile_of(point, k: dict, u0, v0, inv_du, inv_dv, T: int):
    """Tile index of the line from `point` towards the light (float64), or None outside the table."""
    az = k["axis"]
    ax, ay = (az + 1) % 3, (az + 2) % 3
    p = np.asarray(point, dtype=np.float64) - k["light"]
    qz = -k["sign"] * p[az]
    if not qz < 0:
        return None
    fu = (p[ax] / -qz - float(u0)) * float(inv_du)
    fv = (p[ay] / -qz - float(v0)) * float(inv_dv)
    if not (0 <= fu < T and 0 <= fv < T):
        return None
    return int(fv) * T + int(fu)
