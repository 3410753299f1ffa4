"""TEST INFRASTRUCTURE - a float64 restatement of oracle/rt_oracle.c, with a per-pixel decision margin.

Vectorised over rays with numpy; needs no GPU and nothing from oracle/_ref. It restates the OPERATION of the reference
kernels (sphere, box slabs, the triangle extension of DESIGN.md section 11, closest hit with its tie rules, the light loop
with the quirks the golden fixtures pin, shadow rays, the reflection loop and its tail) in float64 from the float32
inputs, with every fp32 constant written as its float32 value. It is an independent check of the fp32 paths, and it says
which pixels two conforming fp32 builds may legitimately disagree on:

  margin  the smallest relative margin of any discrete decision on the pixel's path - radical against 0, the roots'
          signs and the fmin/fmax choice they drive, the slab enter/exit comparisons, the box-normal thresholds, the
          triangle's guard / det / barycentric / t tests, the nearest-versus-next candidate gap, a shadow hit's t against
          the light (t = 1), nDotL against 0 on a lit light, absorption against 0.999 once it has been computed. A NaN
          or inf anywhere on the path gives margin 0. Decisions on float32 inputs taken as they are (no arithmetic
          before the comparison) are exact in every build and do not count.

A pixel is STABLE when margin >= TAU. TAU was fixed on the CPU (tests/test_f64_reference.py measures what it excludes
and checks that every pixel a 1-ulp nudge of its ray flips is excluded) before any comparison with a GPU build.
"""
from __future__ import annotations

import numpy as np

TAU = 1e-4

MAX_FLOAT = float(np.float32(3.402823466e+38))
F_0999 = float(np.float32(0.999))
F_04998 = float(np.float32(0.4998))
F_001 = float(np.float32(0.01))
F_0001 = float(np.float32(0.001))

SPHERE, BOX, TRIANGLE = 0, 1, 2
_TINY = 1e-300
# a candidate farther than this (relative) from the winning / light distance cannot change the outcome: its own
# decisions are not on the pixel's path
_NEAR = 1e-3
# object x ray pairs evaluated at once
_PAIR_BLOCK = 1 << 21
_EPS32 = 2.0 ** -24
# a ray parameter's sign is trusted when |t| is this many times its estimated fp32 error
_SAFETY = 16.0


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _rel(x, scale):
    """|x| / scale with 0 / 0 = an exact decision (inf) and NaN -> 0."""
    x = np.abs(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(scale > 0, x / np.maximum(scale, _TINY), np.inf)   # no scale: every term was 0, an exact decision
    return np.where(np.isnan(m), 0.0, m)


def _sign_margin(t, dt):
    """Margin of a sign test of a ray parameter t whose fp32 value is uncertain by about dt: TAU exactly when
    |t| = _SAFETY dt."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(dt > 0, TAU * np.abs(t) / (_SAFETY * np.maximum(dt, _TINY)), np.inf)
    return np.where(np.isnan(m), 0.0, m)


def _unit(v):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / n


class Scene:
    """float64 copies of the records, split by primitive type."""

    def __init__(self, objs, lights):
        o = np.asarray(objs)
        self.n = len(o)
        self.type = o["type"].astype(np.int64) if self.n else np.zeros(0, np.int64)
        self.mv = _f64(o["mv"]).reshape(-1, 4, 4) if self.n else np.zeros((0, 4, 4))     # [col][row]
        self.inv = _f64(o["mvInverse"]).reshape(-1, 4, 4) if self.n else np.zeros((0, 4, 4))
        self.amb = _f64(o["ambient"])[:, :3] if self.n else np.zeros((0, 3))
        self.dif = _f64(o["diffuse"])[:, :3] if self.n else np.zeros((0, 3))
        self.spec = _f64(o["specular"])[:, :3] if self.n else np.zeros((0, 3))
        self.absorb = _f64(o["absorption"]) if self.n else np.zeros(0)
        self.shine = _f64(o["shininess"]) if self.n else np.zeros(0)
        li = np.asarray(lights)
        self.l_amb = _f64(li["ambient"])[:, :3]
        self.l_dif = _f64(li["diffuse"])[:, :3]
        self.l_spec = _f64(li["specular"])[:, :3]
        self.l_pos = _f64(li["position"])
        self.groups = {t: np.nonzero(self.type == t)[0] for t in (SPHERE, BOX, TRIANGLE)}


def _object_sd(inv, S, d, serr):
    """A ray parameter's fp32 error in object space: the start's error and the transform's own rounding, carried
    through mvInverse (whose norm grows with a small or non-uniform scale), over |d| in object space."""
    n3 = np.sqrt((inv[:, :3, :3] ** 2).sum((1, 2)))                    # Frobenius norm of the 3x3 part
    tr = np.sqrt((inv[:, 3, :3] ** 2).sum(1))
    s_len = np.sqrt((S[:, :3] ** 2).sum(1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        err = n3[None, :] * (serr + 4 * _EPS32 * s_len)[:, None] + 4 * _EPS32 * tr[None, :]
        return err / np.maximum(np.sqrt((d[..., :3] ** 2).sum(-1)), _TINY)


def _xform(M, v):
    """M (k,4,4) column-major [col][row], v (m,k,4) -> (m,k,4)."""
    return np.einsum("kcr,mkc->mkr", M, v)


def _spheres(sc, idx, S, D, serr):
    inv = sc.inv[idx]
    s = _xform(inv, np.broadcast_to(S[:, None, :], (len(S), len(idx), 4)))
    d = _xform(inv, np.broadcast_to(D[:, None, :], (len(D), len(idx), 4)))
    sd = _object_sd(inv, S, d, serr)
    A = (d[..., :3] ** 2).sum(-1)
    B = 2.0 * (s[..., :3] * d[..., :3]).sum(-1)
    C = (s[..., :3] ** 2).sum(-1) - 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rad = B * B - 4.0 * A * C
        m_rad = _rel(rad, B * B + 4.0 * A * np.abs(C) + 4.0 * A)
        root = np.sqrt(np.maximum(rad, 0.0))
        den = 2.0 * A
        t1 = (-B - root) / den
        t2 = (root - B) / den
        m_t1 = _sign_margin(t1, sd)
        # the far root's sign; for a near miss (rad < 0) with sqrt|rad| standing in for the root, so that a sphere
        # wholly behind the origin is a robust miss whatever the radical does
        root_a = np.sqrt(np.abs(rad))
        t2a = (root_a - B) / den
        m_t2 = _sign_margin(t2a, sd)
        t = np.where(t1 >= 0, t1, t2)
        hit = (rad >= 0) & (t2 >= 0)
        m_hit = np.minimum(np.minimum(m_rad, m_t2), m_t1)
        m_miss = np.maximum(np.where(rad < 0, m_rad, 0.0), np.where(root_a - B < 0, m_t2, 0.0))
        m = np.where(hit, m_hit, m_miss)
        t_est = np.where(hit, t, -B / den)
        p = s + t[..., None] * d
        # near tangency the fp32 t carries an error ~ eps / sqrt(radical margin): the amplification of this hit
        amp = 1.0 / np.sqrt(np.maximum(m_rad, _EPS32))
    return hit, t, t_est, m, p, p[..., :3], amp


def _boxes(sc, idx, S, D, serr):
    inv = sc.inv[idx]
    s = _xform(inv, np.broadcast_to(S[:, None, :], (len(S), len(idx), 4)))
    d = _xform(inv, np.broadcast_to(D[:, None, :], (len(D), len(idx), 4)))
    sd = _object_sd(inv, S, d, serr)
    lo = np.full(s.shape[:2], -np.inf)
    hi = np.full(s.shape[:2], np.inf)
    inside_ok = np.ones(s.shape[:2], bool)
    m_inside = np.full(s.shape[:2], np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(3):
            si, di = s[..., i], d[..., i]
            zero = di == 0
            a = (-0.5 - si) / di
            b = (0.5 - si) / di
            lo = np.maximum(lo, np.where(zero, -np.inf, np.minimum(a, b)))
            hi = np.minimum(hi, np.where(zero, np.inf, np.maximum(a, b)))
            inside_ok &= ~zero | (np.abs(si) < 0.5)
            m_inside = np.minimum(m_inside, np.where(zero, _rel(0.5 - np.abs(si), 0.5), np.inf))
        # an infinite end (a zero direction component inside its slab) takes part in no rounded comparison
        scale = np.where(np.isfinite(hi), np.abs(hi), 0.0) + np.where(np.isfinite(lo), np.abs(lo), 0.0)
        m_span = np.where(np.isfinite(hi) & np.isfinite(lo), _rel(hi - lo, scale), np.inf)
        m_lo = np.where(np.isfinite(lo), _sign_margin(lo, sd), np.inf)
        m_hi = np.where(np.isfinite(hi), _sign_margin(hi, sd), np.inf)
        t = np.where(lo >= 0, lo, hi)
        hit = inside_ok & (hi >= lo) & (hi >= 0)
        p = s + t[..., None] * d
        m_norm = np.min(_rel(np.abs(p[..., :3]) - F_04998, 0.5), axis=-1)
        m_hit = np.minimum.reduce([m_inside, m_span, m_hi, m_lo, m_norm])
        m_miss = np.maximum.reduce([np.where(~inside_ok, m_inside, 0.0), np.where(hi < lo, m_span, 0.0),
                                    np.where(hi < 0, m_hi, 0.0)])
        m = np.where(hit, m_hit, m_miss)
        t_est = np.where(hit, t, np.where(np.isfinite(lo), lo, np.inf))
        n = np.where(p[..., :3] > F_04998, 1.0, np.where(p[..., :3] < -F_04998, -1.0, 0.0))
    return hit, t, t_est, m, p, n, np.ones_like(t)


def _triangles(sc, idx, S, D, serr):
    sd = ((serr + 4 * _EPS32 * np.sqrt((S[:, :3] ** 2).sum(1))) / np.maximum(np.sqrt((D[:, :3] ** 2).sum(1)), _TINY))[:, None]
    mv = sc.mv[idx]
    v0, v1, v2 = mv[:, 0, :3], mv[:, 1, :3], mv[:, 2, :3]
    c, R = sc.inv[idx, 0, :3], sc.inv[idx, 0, 3]
    s, d = S[:, None, :3], D[:, None, :3]
    e1, e2 = (v1 - v0)[None], (v2 - v0)[None]
    tv = s - v0[None]
    oc = c[None] - s
    nrm = lambda x: np.sqrt((x * x).sum(-1))  # noqa: E731
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = np.cross(oc, d)
        gg, rr = dot(g, g), (R * R)[None] * dot(d, d)
        ok = [gg <= rr]
        ms = [_rel(gg - rr, gg + rr)]
        p = np.cross(d, e2)
        det = dot(e1, p)
        ok.append(det != 0)
        ms.append(_rel(det, nrm(e1) * nrm(p)))
        inv = 1.0 / det
        su = nrm(tv) * nrm(p) * np.abs(inv)
        u = dot(tv, p) * inv
        q = np.cross(tv, e1)
        sv = nrm(d) * nrm(q) * np.abs(inv)
        v = dot(d, q) * inv
        st = nrm(e2) * nrm(q) * np.abs(inv)
        t = dot(e2, q) * inv
        h = s + t[..., None] * d - c[None]
        hh = dot(h, h)
        r2 = (R * R)[None]
        ok += [u >= 0, u <= 1, v >= 0, u + v <= 1, t >= 0, hh <= r2]
        ms += [_rel(u, su), _rel(u - 1, su + 1), _rel(v, sv), _rel(1 - u - v, su + sv + 1), np.minimum(_rel(t, st), _sign_margin(t, sd)),
               _rel(hh - r2, hh + r2)]
        hit = np.logical_and.reduce(ok)
        m_hit = np.minimum.reduce(ms)
        m_miss = np.maximum.reduce([np.where(~o, mm, 0.0) for o, mm in zip(ok, ms)])
        m = np.where(hit, m_hit, m_miss)
        t_est = np.where(np.isfinite(t), t, np.inf)
        n = np.broadcast_to(np.cross(e1, e2), h.shape)
    return hit, t, t_est, m, None, n, np.ones_like(t)


def cast(sc, S, D, shadow=False, serr=None):
    """Closest hit of rays S, D (m,4) over every object, in float64.

    Returns (idx (-1 miss), t (MAX_FLOAT miss), inter (m,4), normal (m,3, unit), margin (m,)). For a shadow cast only the
    nearest t matters (against 1, the light), and only candidates nearer than the light count. serr (m,): the estimated
    fp32 error of the starts (view units; 0 for the camera's); the returned tuple ends with that of the hit points."""
    m = len(S)
    best_t = np.full(m, np.inf)
    best_i = np.full(m, -1, np.int64)
    inter = np.zeros((m, 4))
    normal = np.zeros((m, 3))
    cands = []  # (t_est, margin, t_hit or inf, object index, is_sphere) per type block, gathered for the gap / near test
    if sc.n == 0 or m == 0:
        return best_i, np.full(m, MAX_FLOAT), inter, normal, np.full(m, np.inf), np.zeros(m)
    fn = {SPHERE: _spheres, BOX: _boxes, TRIANGLE: _triangles}
    # a ray parameter's fp32 error from the start's (its inherited error and its own rounding), in units of |D|: what
    # a sign test of some t (a secondary ray meeting the surface it leaves, an origin on a box face) is measured against
    s_len = np.sqrt((S[:, :3] ** 2).sum(1))
    d_len = np.maximum(np.sqrt((D[:, :3] ** 2).sum(1)), _TINY)
    if serr is None:
        serr = np.zeros(m)
    sd = ((serr + 4 * _EPS32 * s_len) / d_len)[:, None]
    best_amp = np.ones(m)
    for typ, idx_all in sc.groups.items():
        if not len(idx_all):
            continue
        step = max(1, _PAIR_BLOCK // max(m, 1))
        for k0 in range(0, len(idx_all), step):
            idx = idx_all[k0:k0 + step]
            hit, t, t_est, mg, p, n_obj, amp = fn[typ](sc, idx, S, D, serr)
            th = np.where(hit, t, np.inf)
            cands.append((t_est, mg, th, idx))
            # the closest-hit rule per block (ties: the last sphere wins, otherwise the first object); merged below
            j = np.argmin(th, axis=1)
            tj = th[np.arange(m), j]
            if typ == SPHERE:
                # last index with the minimal t
                jr = th.shape[1] - 1 - np.argmin(th[:, ::-1], axis=1)
                j = np.where(np.isfinite(tj), jr, j)
            kj = idx[j]
            better = (tj < best_t) | ((tj == best_t) & np.isfinite(tj) & (
                (typ == SPHERE) & ((sc.type[np.maximum(best_i, 0)] != SPHERE) | (kj > best_i)) |
                (typ != SPHERE) & (sc.type[np.maximum(best_i, 0)] != SPHERE) & (kj < best_i)))
            if not better.any():
                continue
            rows = np.nonzero(better)[0]
            jj = j[rows]
            best_t[rows] = tj[rows]
            best_i[rows] = kj[rows]
            best_amp[rows] = amp[rows, jj]
            if typ == TRIANGLE:
                inter[rows] = S[rows] + tj[rows, None] * D[rows]
                normal[rows] = _unit(n_obj[rows, jj])
            else:
                mvk = sc.mv[kj[rows]]
                pk = p[rows, jj]
                inter[rows] = np.einsum("kcr,kc->kr", mvk, pk)
                n4 = np.concatenate([n_obj[rows, jj], np.zeros((len(rows), 1))], axis=1)
                normal[rows] = _unit(np.einsum("kcr,kc->kr", mvk, n4)[:, :3])
    # margins: the decisions of every candidate that could matter, and the gap to the runner-up
    scale = s_len / d_len
    limit = np.where(shadow, 1.0, np.where(np.isfinite(best_t), best_t, np.inf))
    margin = np.full(m, np.inf)
    second = np.full(m, np.inf)
    for t_est, mg, th, idx in cands:
        near = ~(t_est > limit[:, None] * (1 + _NEAR) + _NEAR * scale[:, None]) | np.isnan(t_est)
        margin = np.minimum(margin, np.where(near, mg, np.inf).min(axis=1))
        other = np.where(idx[None, :] == best_i[:, None], np.inf, th)
        second = np.minimum(second, other.min(axis=1))
    with np.errstate(invalid="ignore"):
        if shadow:
            dec = _rel(best_t - 1.0, 1.0 + scale)
            margin = np.minimum(margin, np.where(np.isfinite(best_t), dec, np.inf))
        else:
            gap = _rel(second - best_t, second + scale)
            margin = np.minimum(margin, np.where(np.isfinite(best_t) & np.isfinite(second), gap, np.inf))
    bad = np.isnan(best_t) | ~np.isfinite(inter).all(1) | ~np.isfinite(normal).all(1)
    margin = np.where(bad & (best_i >= 0), 0.0, margin)
    with np.errstate(invalid="ignore", over="ignore"):
        ierr = serr + 4 * _EPS32 * (s_len + np.abs(best_t) * d_len * best_amp)
    return best_i, np.where(np.isfinite(best_t), best_t, MAX_FLOAT), inter, normal, margin, np.where(best_i >= 0, ierr, 0.0)


def _shade_lights(sc, P4, N, obj, accumulate, perr):
    """The light loop at hit points P4 (m,4) with normals N (m,3) of objects obj (m,). Returns (rgb (m,3), margin (m,))."""
    m = len(P4)
    P = P4[:, :3]
    color = np.zeros((m, 3))
    spec = np.zeros((m, 3))
    margin = np.full(m, np.inf)
    nv = _unit(N)
    vv = _unit(-P)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for li in range(len(sc.l_pos)):
            pos = sc.l_pos[li]
            lv = pos[None, :3] - P if pos[3] != 0 else np.broadcast_to(-pos[None, :3], P.shape)
            nl = _unit(lv)
            S = np.concatenate([P + F_001 * nl, np.ones((m, 1))], axis=1)
            D = np.concatenate([lv, np.zeros((m, 1))], axis=1)
            _, ts, _, _, ms, _ = cast(sc, S, D, shadow=True, serr=perr)
            margin = np.minimum(margin, ms)
            lit = (ts >= 1.0) | (ts < 0)
            ndl = (nv * nl).sum(1)
            rv = _unit(-nl + 2.0 * (nl * nv).sum(1, keepdims=True) * nv)
            rdv = np.maximum((rv * vv).sum(1), 0.0)
            amb = sc.amb[obj] * sc.l_amb[li]
            dif = np.where(lit[:, None], sc.dif[obj] * sc.l_dif[li] * np.maximum(ndl, 0.0)[:, None], 0.0)
            pw = np.power(rdv, np.maximum(sc.shine[obj], 1.0))
            new_spec = sc.spec[obj] * sc.l_spec[li] * pw[:, None]
            spec = np.where((lit & (ndl > 0))[:, None], new_spec, np.where(lit[:, None], spec, 0.0))
            margin = np.minimum(margin, np.where(lit, _rel(ndl, 1.0), np.inf))
            color = (color + amb + dif + spec) if accumulate else (amb + dif + spec)
    return color, margin


def _reflect(D, N):
    return D[:, :3] - 2.0 * (D[:, :3] * N).sum(1, keepdims=True) * N


def render(kernel, objs, lights, rays, max_bounces=0):
    """float64 render. Returns dict(out, hit_index, hit_t, margin, stable).

    out: hittest -> t per ray (MAX_FLOAT on a miss); shade / shade_and_reflect -> (n,3) colour (0 where the primary ray
    misses: the pixel keeps the host's background)."""
    kid = {"hittest": 0, "shade": 1, "shade_and_reflect": 2}.get(kernel, kernel)
    sc = Scene(objs, lights)
    rays = np.asarray(rays)
    S0, D0 = _f64(rays["start"]), _f64(rays["direction"])
    n = len(rays)
    idx, t, inter, normal, margin, ierr = cast(sc, S0, D0)
    hit = idx >= 0
    if kid == 0:
        return _finish(dict(out=t.copy(), hit_index=idx, hit_t=t, margin=margin))
    rgb = np.zeros((n, 3))
    rows = np.nonzero(hit)[0]
    obj = idx[rows]
    col, ms = _shade_lights(sc, inter[rows], normal[rows], obj, accumulate=(kid == 1), perr=ierr[rows])
    margin[rows] = np.minimum(margin[rows], ms)
    if kid == 1:
        rgb[rows] = col
        return _finish(dict(out=rgb, hit_index=idx, hit_t=t, margin=margin))

    absorb = col * sc.absorb[obj][:, None]
    ap = sc.absorb[obj].copy()
    ap_exact = np.ones(len(rows), bool)
    reflc = np.zeros((len(rows), 3))
    bounces = np.full(len(rows), np.uint32(max_bounces) & 0xFFFFFFFF, dtype=np.uint64)
    refl = _reflect(D0[rows], normal[rows])
    cur_inter = inter[rows]
    cur_err = ierr[rows]
    active = np.ones(len(rows), bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while active.any():
            a = np.nonzero(active)[0]
            before = bounces[a].copy()
            bounces[a] = (bounces[a] - 1) & 0xFFFFFFFF  # unsigned post-decrement, whether or not the test passes
            go = before > 0
            a_go = a[go]
            active[a[~go]] = False
            if not len(a_go):
                break
            nd = _unit(refl[a_go])
            S = np.concatenate([cur_inter[a_go, :3] + F_0001 * nd, cur_inter[a_go, 3:4]], axis=1)
            D = np.concatenate([refl[a_go], np.zeros((len(a_go), 1))], axis=1)
            ri, _, rint, rn, rm, rerr = cast(sc, S, D, serr=cur_err[a_go])
            margin[rows[a_go]] = np.minimum(margin[rows[a_go]], rm)
            got = ri >= 0
            active[a_go[~got]] = False
            b = a_go[got]
            ri, rint, rn, D, rerr = ri[got], rint[got], rn[got], D[got], rerr[got]
            # absorptionPercent <= 0.999f: exact while it is still an input value
            m_ap = np.where(ap_exact[b], np.inf, _rel(ap[b] - F_0999, 1.0))
            margin[rows[b]] = np.minimum(margin[rows[b]], m_ap)
            cont = ap[b] <= F_0999
            active[b[~cont]] = False
            c = b[cont]
            ri, rint, rn, D, rerr = ri[cont], rint[cont], rn[cont], D[cont], rerr[cont]
            if not len(c):
                continue
            col, ms = _shade_lights(sc, rint, rn, ri, accumulate=False, perr=rerr)
            margin[rows[c]] = np.minimum(margin[rows[c]], ms)
            reflc[c] = col
            ra = (1.0 - ap[c]) * sc.absorb[ri]
            absorb[c] = absorb[c] + ra[:, None] * col
            ap[c] = ap[c] + ra
            ap_exact[c] = False
            refl[c] = _reflect(D, rn)
            cur_inter[c] = rint
            cur_err[c] = rerr
        tail = (bounces == 0) & (ap < 1.0)
        absorb[tail] = absorb[tail] + (1.0 - ap[tail])[:, None] * reflc[tail]
    rgb[rows] = absorb
    return _finish(dict(out=rgb, hit_index=idx, hit_t=t, margin=margin))


def _finish(res):
    out = res["out"]
    bad = ~np.isfinite(out) if out.ndim == 1 else ~np.isfinite(out).all(1)
    bad &= res["hit_index"] >= 0
    res["margin"] = np.where(bad | np.isnan(res["margin"]), 0.0, res["margin"])
    res["stable"] = res["margin"] >= TAU
    return res
