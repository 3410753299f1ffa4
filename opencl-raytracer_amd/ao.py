"""Ambient-occlusion frames (hip_raytracer.h, "ambient-occlusion frames"): the executable definition of rt_ao* / rt_render_ao*.

rays()    the n * K occlusion rays of n items and which items are live - float32, every product and sum rounded, nothing contracted;
reduce()  occlusion answers per ray -> the unoccluded count (uint8) and ao (float32) per item;
directions()  a cosine-weighted direction table made with numpy - a convenience only, no part of exactness: the library takes any table
          and neither normalises nor scales a direction (its length is the occlusion radius).

filter()  the edge-aware box blur of the counts over a (2r + 1)^2 window ("filtered ambient occlusion"): taps, sum, ao and grey per item.

unoccluded = reduce(query_occluded(rays(...)), live, K) on the same context is what the GPU pass delivers, bit for bit; so is filter()
of rt_ao_filter* / rt_render_ao_filtered*."""
from __future__ import annotations

import numpy as np

F = np.float32
SAMPLES = (1, 2, 4, 8, 16, 32, 64)
MAX_SETS = 4096
HASH = 0x9E3779B1
RADII = (1, 2, 3, 4)


def check(samples: int, n_sets: int, bias: float):
    """What the library refuses of the three scalars (RT_ERR_INVALID_ARGUMENT there, ValueError here)."""
    if samples not in SAMPLES:
        raise ValueError(f"samples is one of {SAMPLES}")
    if not 1 <= n_sets <= MAX_SETS:
        raise ValueError(f"n_sets is 1 .. {MAX_SETS}")
    if not (np.isfinite(F(bias)) and F(bias) >= 0):
        raise ValueError("bias must be finite and not negative")


def table(dirs, samples: int) -> np.ndarray:
    """The direction table as the library reads it: a contiguous float32 (n_sets * samples, 4) array from an array of 3 or 4 columns
    (w is ignored; a missing one is 0), any leading shape. Raises ValueError where it holds no whole set."""
    d = np.asarray(dirs, dtype=F)
    if d.ndim < 2 or d.shape[-1] not in (3, 4):
        raise ValueError("dirs: float32 with 3 or 4 columns, n_sets * samples rows")
    d = d.reshape(-1, d.shape[-1])
    if len(d) == 0 or len(d) % samples:
        raise ValueError("dirs: a whole number of sets of `samples` directions, at least one")
    out = np.zeros((len(d), 4), dtype=F)
    out[:, :d.shape[1]] = d
    return out


def item_sets(items, n_sets: int) -> np.ndarray:
    """The set of every global work-item number: h = (uint32)g * 0x9E3779B1 (mod 2^32), set = (h >> 16) % n_sets. Integers only."""
    g = np.asarray(items, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    h = (g * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(16)) % np.uint64(n_sets)).astype(np.int64)


def live_items(point, normal, index=None) -> np.ndarray:
    """bool per item: index >= 0 (where an index is given) and point.xyz, normal.xyz all finite."""
    p, n = np.asarray(point, dtype=F).reshape(-1, 4), np.asarray(normal, dtype=F).reshape(-1, 4)
    live = np.isfinite(p[:, :3]).all(axis=1) & np.isfinite(n[:, :3]).all(axis=1)
    if index is not None:
        live &= np.asarray(index).reshape(-1) >= 0
    return live


def rays(point, normal, index, dirs, samples: int, bias: float, items=None):
    """(rays, live): float32 (n * samples, 8) - start.xyzw, direction.xyzw; ray i * samples + k is sample k of item i - and bool[n].

    point, normal: float32 (n, 4) as render_gbuffer / query_hits deliver them; index: int32[n] or None (every item may be live);
    dirs: the table (table()); items: the global work-item number of every item (None: 0 .. n - 1).
    Sample k of a live item, all float32:  d = dirs[set * K + k].xyz;  s = (d.x * n.x + d.y * n.y) + d.z * n.z;  s < 0: d = -d (a NaN or
    zero s keeps d);  start.c = p.c + (bias * n.c), start.w = 1;  direction = (d, 0). The rays of a dead item are all-zero records and
    must not be traced: reduce() ignores their answers."""
    dirs = table(dirs, samples)
    n_sets = len(dirs) // samples
    check(samples, n_sets, bias)
    p, nrm = np.asarray(point, dtype=F).reshape(-1, 4), np.asarray(normal, dtype=F).reshape(-1, 4)
    n = len(p)
    if len(nrm) != n or (index is not None and np.asarray(index).size != n):
        raise ValueError("point, normal and index have one entry per item")
    g = np.arange(n, dtype=np.uint64) if items is None else np.asarray(items).reshape(-1)
    if len(g) != n:
        raise ValueError("items: one global work-item number per item")
    live = live_items(p, nrm, index)
    out = np.zeros((n, samples, 8), dtype=F)
    b = F(bias)
    with np.errstate(all="ignore"):
        d = dirs[(item_sets(g, n_sets) * samples)[:, None] + np.arange(samples)[None, :], :3]          # (n, K, 3)
        nx, ny, nz = (nrm[:, None, c] for c in range(3))
        s = ((d[..., 0] * nx).astype(F) + (d[..., 1] * ny).astype(F)).astype(F)
        s = (s + (d[..., 2] * nz).astype(F)).astype(F)
        d = np.where((s < F(0))[..., None], -d, d)
        start = (p[:, :3] + (b * nrm[:, :3]).astype(F)).astype(F)
    out[..., 0:3] = start[:, None, :]
    out[..., 3] = F(1)
    out[..., 4:7] = d
    out[~live] = F(0)
    return out.reshape(n * samples, 8), live


def reduce(occluded, live, samples: int):
    """(unoccluded uint8[n], ao float32[n]) from one occlusion answer per ray of rays(): K - the occluded samples of a live item; a
    dead item reads K and 1.0 whatever its entries hold. ao = float32(unoccluded) * float32(1 / K), exact for these K."""
    live = np.asarray(live, dtype=bool).reshape(-1)
    occ = (np.asarray(occluded).reshape(len(live), samples) != 0).sum(axis=1)
    unoccluded = np.where(live, samples - occ, samples).astype(np.uint8)
    return unoccluded, (unoccluded.astype(F) * (F(1.0) / F(samples))).astype(F)


def directions(samples: int, n_sets: int, radius: float, seed: int = 0) -> np.ndarray:
    """A table of n_sets * samples directions of length `radius`, float32 (n_sets * samples, 4) with w = 0: cosine-weighted about +z
    (the pass mirrors a direction to the normal's side, so the weighting holds only loosely for other normals - rotate a table of
    your own for more). Made with numpy on the host from `seed`."""
    check(samples, n_sets, 0.0)
    rng = np.random.default_rng(seed)
    u, v = rng.random(n_sets * samples), rng.random(n_sets * samples)
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    d = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u)), np.zeros_like(u)], axis=1) * float(radius)
    d[:, 3] = 0.0
    return d.astype(F)


def check_filter(samples: int, radius: int, plane_max: float):
    """What the library refuses of the filter's scalars (RT_ERR_INVALID_ARGUMENT there, ValueError here); normal_min is any float."""
    if samples not in SAMPLES:
        raise ValueError(f"samples is one of {SAMPLES}")
    if radius not in RADII:
        raise ValueError(f"radius is one of {RADII}")
    if not (np.isfinite(F(plane_max)) and F(plane_max) >= 0):
        raise ValueError("plane_max must be finite and not negative")


def grey_of(ao) -> np.ndarray:
    """The byte of the table of "8-bit frames" for every float32 value: p = v * 255.0f, f = floorf(p); a NaN or f < 0: 0; f >= 255: 255."""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(ao, dtype=F) * F(255.0)).astype(F))
        f = np.where(np.isnan(f) | (f < 0), F(0), np.where(f >= 255, F(255), f))
    return f.astype(np.uint8)


def filter(unoccluded, point, normal, index, width: int, samples: int, radius: int, normal_min: float, plane_max: float):
    """{"ao": float32[n], "grey": uint8[n], "taps": uint8[n], "sum": uint32[n]} of a row-major array of `width` columns; n a multiple of
    `width`. Item p is live as live_items() says. A live p accepts itself untested and every live q != p of its window (|dcol| <=
    radius, |drow| <= radius, inside the array) with, all float32, every product and sum rounded and nothing contracted,
        c = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_min   and
        d = P_q - P_p,  e = (n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z,  |e| <= plane_max            (a comparison with a NaN is false);
    taps: the accepted items, sum: their `unoccluded` bytes added as integers (not clamped to `samples`),
    ao = float32(sum) / float32(taps * samples), one correctly rounded division; grey = grey_of(ao). A dead p: taps 0, sum 0, ao 1, grey 255."""
    check_filter(samples, radius, plane_max)
    u = np.asarray(unoccluded).reshape(-1)
    if u.dtype != np.uint8:
        raise ValueError("unoccluded: uint8, one per item")
    p, nr = np.asarray(point, dtype=F).reshape(-1, 4), np.asarray(normal, dtype=F).reshape(-1, 4)
    n, width, r = len(u), int(width), int(radius)
    if len(p) != n or len(nr) != n or (index is not None and np.asarray(index).size != n):
        raise ValueError("unoccluded, point, normal and index have one entry per item")
    if n == 0:
        return {"ao": np.zeros(0, F), "grey": np.zeros(0, np.uint8), "taps": np.zeros(0, np.uint8), "sum": np.zeros(0, np.uint32)}
    if width < 1 or n % width:
        raise ValueError("width: at least 1, and the items are whole rows of it")
    rows = n // width
    live = live_items(p, nr, index).reshape(rows, width)
    P, N, U = p[:, :3].reshape(rows, width, 3), nr[:, :3].reshape(rows, width, 3), u.reshape(rows, width).astype(np.uint32)
    taps, total = live.astype(np.uint32), np.where(live, U, 0).astype(np.uint32)
    nm, pm = F(normal_min), F(plane_max)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if (dx == 0 and dy == 0) or abs(dy) >= rows or abs(dx) >= width:
                    continue
                pr, qr = slice(max(0, -dy), rows - max(0, dy)), slice(max(0, dy), rows - max(0, -dy))      # rows of p, rows of q = p + dy
                pc, qc = slice(max(0, -dx), width - max(0, dx)), slice(max(0, dx), width - max(0, -dx))
                Np, Nq, Pp, Pq = N[pr, pc], N[qr, qc], P[pr, pc], P[qr, qc]
                c = ((Np[..., 0] * Nq[..., 0]).astype(F) + (Np[..., 1] * Nq[..., 1]).astype(F)).astype(F)
                c = (c + (Np[..., 2] * Nq[..., 2]).astype(F)).astype(F)
                d = (Pq - Pp).astype(F)
                e = ((Np[..., 0] * d[..., 0]).astype(F) + (Np[..., 1] * d[..., 1]).astype(F)).astype(F)
                e = (e + (Np[..., 2] * d[..., 2]).astype(F)).astype(F)
                ok = live[pr, pc] & live[qr, qc] & (c >= nm) & (np.abs(e) <= pm)
                taps[pr, pc] += ok
                total[pr, pc] += np.where(ok, U[qr, qc], 0).astype(np.uint32)
        ao = np.where(live, total.astype(F) / np.maximum(taps * np.uint32(samples), 1).astype(F), F(1.0)).astype(F)
    ao = ao.reshape(-1)
    return {"ao": ao, "grey": grey_of(ao), "taps": taps.reshape(-1).astype(np.uint8), "sum": total.reshape(-1)}
