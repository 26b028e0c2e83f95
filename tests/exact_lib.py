"""A plain float64 reference of the sphere extension with derived rounding bounds.  No pytest, no scenes,
and nothing of the oracle: it is written from the wording of include/esctp1_rt.h (esc_scene_add_spheres,
esc_intersect_rays, esc_occluded_rays, esc_shade_rays) and main.cpp:740-789, not from oracle/rt_oracle.c.

The fp32 inputs are taken as the exact real numbers they are; every difference of two fp32 numbers, and
every product of two, is exact in float64 (24 + 24 <= 53 bits), so float64 only rounds in the sums, the
divide and the square root.  exact_check() shows on 256 pairs, in rationals, that this costs less than the
bounds allow for it.

The documented operation
  ray-sphere   the roots of  a t^2 + 2 b t + cc = 0,  a = d.d,  b = (o - c).d,  cc = |o - c|^2 - r^2;
               D = b^2 - a cc;  near (-b - sqrt D)/a, far (-b + sqrt D)/a;  the near root unless it is < eps,
               then the far root;  rejected when < eps;  rejected when >= tmax.  eps = FLT_EPSILON.
  closest hit  triangles geometry by geometry and face by face, then spheres by index; the first of equals wins
  occlusion    any accepted primitive under tmax
  colour       one light, ks = 0: N = normalize(o + d t - c) (spheres) or the face normal; light point P =
               the light's vertex[face] (quirk S2); hit point o + d (t - eps); L = P - hit; shadow bound
               |L| - eps; a light that is occluded, or has N.L <= 0, adds nothing (main.cpp:772-778: both are
               `continue` before the pixel is touched); otherwise it adds (ka*0.5 + ke)/nl + kd (N.L)/nl.

Running error bounds, u = 2^-24, first order.  A hat marks the fp32 value, E_x bounds |x^ - x|.  One line per
operation of the fp32 chain (a dot is sum = 0; sum += x_i*y_i for i = 0, 1, 2: term 0 and 1 meet one product
and two roundings of the sum, term 2 one product and one):
  oc = o - c                 E_oc_i   = u |oc_i|
  b = dot(oc, d)             E_b      = u (4 |oc_0 d_0| + 4 |oc_1 d_1| + 3 |oc_2 d_2|)
  dot(oc, oc)                E_S      = u (5 oc_0^2 + 5 oc_1^2 + 4 oc_2^2)
  r*r                        E_rr     = u r^2
  cc = dot(oc, oc) - r*r     E_cc     = E_S + E_rr + u |cc|
  b*b                        E_bb     = 2 |b| E_b + u b^2
  disc = b*b - cc            E_disc   = E_bb + E_cc + u |b^2 - cc| + |a - 1| |cc|
        the chain takes a == 1: it computes b^2 - cc where the quadratic has D = b^2 - a cc
  sq = sqrtf(disc)           E_sq     = E_disc / (sqrt D + sqrt max(D - E_disc, 0)) + u sqrt(D + E_disc)
        (not first order: sqrt is not differentiable at 0; for D < 0 <= disc^ the value sqrt 0 is compared)
  t2 = -b -+ sq              E_t      = E_b + E_sq + u |a t| + |a - 1| |t|
        the chain returns a t where the quadratic has t
  p = o + d*t                E_p_i    = E_t |d_i| + u (|d_i t| + |o_i + d_i t|)
  p - c                      E_P_i    = E_p_i + u |P_i|
  N = normalize(P)           E_N      = |E_P| / |P| + 3.5 u      (dot 3u/2 after the root, the root u/2 + u,
                                                                  the divide u: 3.5 u on a unit vector)
  scan_row's sphere branch then takes
  hit = o + d*(t - eps)      E_h_i    = (E_t + u |t|) |d_i| + u (|d_i t| + |hit_i|)
  L = P_light - hit          E_L_i    = E_h_i + u |L_i|
  len = length(L)            E_len    = |E_L| + 2.5 u len;   shadow bound len - eps: E_len + u len
  L = normalize(L)           E_Ldir   = |E_L| / len + 3.5 u
  d = dot(N, L)              E_NL     = E_N + E_Ldir + 3 u
  colour                     E_rgb    = kd E_NL / nl + 4 u rgb
Every bound is multiplied by 1 + 2^-20: the terms of second order (some tens of u^2, relative) and float64's
own error (a few 2^-53 of the same magnitudes, 2^-29 of the bound) are both far below that.

A shadow ray of the fp32 chain does not start where the exact one does: its origin differs by up to |E_h|, its
direction by E_Ldir, its bound by E_len.  The pair functions take these as `do`, `dd`, `dtmax` and add what
they can move to each bound (|d| do + |oc| dd to E_b, 2 |oc| do to E_cc, 2 dd to |a - 1|, do + |t| dd to E_t).

Ill-conditioned: an exact compared quantity within its bound of its threshold -- D against 0, a root against
eps, the accepted root against tmax, N.L against 0.  The fp32 code may decide such a pair either way;
everything else it must decide as the exact arithmetic does.

Triangles (the floor and the light of the synthetic scenes) are restated with the same reject rules in float64
(|det| < eps, u < eps, u > 1, v < eps, u + v > 1, t < eps, t >= tmax), each with a margin of 8 u times the
sum of the magnitudes that enter it; a ray within a margin is ill-conditioned.  Their own accuracy is not
judged here: the triangle arithmetic is pinned to the reference bit for bit elsewhere.

Out of scope, because nothing bounded here covers them: several lights (quirk S3 makes a light's hit point
depend on which occluder the previous light's loop met first, a choice of index order and not of geometry),
ks != 0 (powf: the device's and the host's differ, and its condition number is Ns), bounces and refraction.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -23  # FLT_EPSILON
FLT_MAX = float(np.finfo(np.float32).max)
SLACK = 1.0 + 2.0 ** -20
HIT, MISS, ILL = 1, 0, -1
CHUNK = 128


def f64(x):
    return np.ascontiguousarray(x, np.float64)


def _per_ray(x, n):
    return np.broadcast_to(f64(x), (n,))[:, None]


# ---- pairs ----------------------------------------------------------------------------------------------
def sphere_pairs(o, d, sph, tmax=None, do=0.0, dd=0.0, dtmax=0.0, paired=False):
    """rays (n, 3) x spheres (k, 4) -> dict of (n, k) arrays (paired: ray i against sphere i alone, (n, 1)): the exact discriminant "D" and its bound "ED",
    both roots "near", "far" (NaN where D < 0) and their bounds "Enear", "Efar", the accepted root "t" with
    "Et" (NaN unless state is HIT), "state" (HIT / MISS / ILL) and "tlow": the smallest t the fp32 chain could
    accept for the pair (inf where it must miss)."""
    o, d, sph = f64(o), f64(d), f64(sph)
    n = o.shape[0]
    tmax = _per_ray(FLT_MAX if tmax is None else tmax, n)
    do, dd, dtmax = _per_ray(do, n), _per_ray(dd, n), _per_ray(dtmax, n)
    with np.errstate(all="ignore"):
        oc = (o - sph[:, :3])[:, None, :] if paired else o[:, None, :] - sph[None, :, :3]
        dv = d[:, None, :]
        a = (d * d).sum(1)[:, None]
        a1 = np.abs(a - 1.0) + 2.0 * dd
        loc = np.sqrt((oc * oc).sum(2))
        ld = np.sqrt(a)
        ap = np.abs(oc * dv)
        b = (oc * dv).sum(2)
        Eb = U * (4 * ap[..., 0] + 4 * ap[..., 1] + 3 * ap[..., 2]) + ld * do + loc * dd
        o2 = oc * oc
        r2 = (sph[:, 3] * sph[:, 3])[:, None] if paired else (sph[:, 3] * sph[:, 3])[None, :]
        cc = o2.sum(2) - r2
        Ecc = U * (5 * o2[..., 0] + 5 * o2[..., 1] + 4 * o2[..., 2] + r2 + np.abs(cc)) + 2 * loc * do
        D = b * b - a * cc
        ED = (2 * np.abs(b) * Eb + U * b * b + Ecc + U * np.abs(b * b - cc) + a1 * np.abs(cc)) * SLACK
        Dp = np.maximum(D, 0.0)
        sq = np.sqrt(Dp)
        Esq = ED / (sq + np.sqrt(np.maximum(D - ED, 0.0))) + U * np.sqrt(Dp + ED)
        Esq = np.where(D > ED, Esq, np.sqrt(Dp + ED) * (1 + U))  # at the rim: sq^ <= sqrt(D + ED) (1 + u)
        near, far = (-b - sq) / a, (-b + sq) / a
        En = (Eb + Esq + U * np.abs(a * near) + a1 * np.abs(near) + do + np.abs(near) * dd) * SLACK
        Ef = (Eb + Esq + U * np.abs(a * far) + a1 * np.abs(far) + do + np.abs(far) * dd) * SLACK
        rim = np.abs(D) <= ED
        miss = D < -ED
        near_ok, near_no = near > EPS + En, near < EPS - En
        far_ok, far_no = far > EPS + Ef, far < EPS - Ef
        take_near = ~rim & ~miss & near_ok
        take_far = ~rim & ~miss & near_no & far_ok
        t = np.where(take_near, near, np.where(take_far, far, np.nan))
        Et = np.where(take_near, En, np.where(take_far, Ef, np.nan))
        miss |= ~rim & near_no & far_no
        Etm = Et + dtmax
        beyond = (take_near | take_far) & (t > tmax + Etm)
        inside = (take_near | take_far) & (t < tmax - Etm)
        state = np.where(miss | beyond, MISS, np.where(inside, HIT, ILL)).astype(np.int8)
        # what an undecided pair could still return: nothing under its smallest root's lower end
        lo_near = (-b - np.sqrt(Dp + ED) * (1 + U)) / a - (Eb + a1 * np.abs(near) + do) * 2
        tlow = np.where(state == MISS, np.inf, np.where(state == HIT, t - Et,
                                                        np.where(lo_near > EPS, lo_near, -np.inf)))
        near = np.where(D < 0, np.nan, near)
        far = np.where(D < 0, np.nan, far)
    return {"D": D, "ED": ED, "near": near, "far": far, "Enear": En, "Efar": Ef, "t": t, "Et": Et,
            "state": state, "tlow": tlow, "b": b, "a": a}


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def _cross_mag(x, y):
    x, y = np.abs(x), np.abs(y)
    return np.stack([x[..., 1] * y[..., 2] + x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] + x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] + x[..., 1] * y[..., 0]], axis=-1)


def _len(x):
    return np.sqrt((x * x).sum(-1))


def triangle_pairs(o, d, tri, tmax=None, do=0.0, dd=0.0, dtmax=0.0):
    """rays (n, 3) x triangles (k, 3, 3) -> {"t", "Et", "state", "tlow"}: ray_triangle.h's rejects in float64,
    each with a margin (module docstring)"""
    o, d, tri = f64(o), f64(d), f64(tri).reshape(-1, 3, 3)
    n = o.shape[0]
    tmax = _per_ray(FLT_MAX if tmax is None else tmax, n)
    do, dd, dtmax = _per_ray(do, n), _per_ray(dd, n), _per_ray(dtmax, n)
    K = 8 * U
    with np.errstate(all="ignore"):
        v0 = tri[None, :, 0]
        e1, e2 = (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
        dv = np.broadcast_to(d[:, None, :], (n, tri.shape[0], 3))
        pv, mpv = _cross(dv, e2), _cross_mag(dv, e2)
        det = (e1 * pv).sum(2)
        Edet = K * (np.abs(e1) * mpv).sum(2) + _len(e1) * _len(e2) * dd
        tv = o[:, None, :] - v0
        un = (tv * pv).sum(2)
        Eun = K * (np.abs(tv) * mpv).sum(2) + do * _len(pv) + _len(tv) * _len(e2) * dd
        qv, mqv = _cross(tv, e1), _cross_mag(tv, e1)
        vn = (dv * qv).sum(2)
        Evn = K * (np.abs(dv) * mqv).sum(2) + dd * _len(qv) + _len(dv) * _len(e1) * do
        tn = (e2 * qv).sum(2)
        Etn = K * (np.abs(e2) * mqv).sum(2) + _len(e2) * _len(e1) * do
        ad = np.abs(det)
        u, v, t = un / det, vn / det, tn / det
        Eu = ((Eun + np.abs(u) * Edet) / ad + 2 * U * np.abs(u)) * SLACK
        Ev = ((Evn + np.abs(v) * Edet) / ad + 2 * U * np.abs(v)) * SLACK
        Et = ((Etn + np.abs(t) * Edet) / ad + 2 * U * np.abs(t)) * SLACK
        Euv = Eu + Ev + U * np.abs(u + v)
        Etm = Et + dtmax
        no = (ad < EPS - Edet) | (u < EPS - Eu) | (u > 1 + Eu) | (v < EPS - Ev) | (u + v > 1 + Euv) | \
             (t < EPS - Et) | (t > tmax + Etm)
        yes = (ad > EPS + Edet) & (u > EPS + Eu) & (u < 1 - Eu) & (v > EPS + Ev) & (u + v < 1 - Euv) & \
              (t > EPS + Et) & (t < tmax - Etm)
        state = np.where(no, MISS, np.where(yes, HIT, ILL)).astype(np.int8)
        lo = t - Et
        tlow = np.where(state == MISS, np.inf, np.where(np.isfinite(lo) & (lo > EPS), lo, -np.inf))
    return {"t": np.where(state == HIT, t, np.nan), "Et": np.where(state == HIT, Et, np.nan), "state": state,
            "tlow": tlow}


# ---- a scene's primitives in tie order --------------------------------------------------------------------
def primitives(d):
    """scene dict -> {"tri" (m, 3, 3), "geom" (m + k), "prim" (m + k), "sph" (k, 4)}: triangles geometry by
    geometry and face by face, then the spheres; geom is -1 for a sphere"""
    tri, geom, prim = [], [], []
    for gi, g in enumerate(d["geometry"]):
        T = f64(g["vertex"])[np.asarray(g["face_index"], np.int64)]
        tri.append(T)
        geom += [gi] * len(T)
        prim += list(range(len(T)))
    k = len(d["spheres"])
    geom += [-1] * k
    prim += list(range(k))
    tri = np.concatenate(tri) if tri else np.zeros((0, 3, 3))
    return {"tri": tri, "sph": f64(d["spheres"]).reshape(-1, 4), "geom": np.array(geom, np.int32),
            "prim": np.array(prim, np.int32)}


def _pairs(P, o, d, tmax, do, dd, dtmax):
    n = o.shape[0]
    out = {k: [] for k in ("t", "Et", "state", "tlow")}
    for fn, what in ((triangle_pairs, P["tri"]), (sphere_pairs, P["sph"])):
        if len(what):
            r = fn(o, d, what, tmax, do, dd, dtmax)
            for k in out:
                out[k].append(r[k])
    if not out["t"]:
        return {"t": np.zeros((n, 0)), "Et": np.zeros((n, 0)), "state": np.zeros((n, 0), np.int8),
                "tlow": np.zeros((n, 0))}
    return {k: np.concatenate(v, axis=1) for k, v in out.items()}


def _chunks(n):
    return [slice(i, min(n, i + CHUNK)) for i in range(0, n, CHUNK)]


def _arg(x, n, s):
    return np.broadcast_to(f64(x), (n,))[s]


def closest_hit(P, o, d, tmax=None, do=0.0, dd=0.0, dtmax=0.0):
    """the exact nearest primitive of every ray -> {"hit" bool, "t", "Et", "index" (position in tie order, -1),
    "geom", "prim", "ill" (some undecided pair could be, or beat, the answer), "tie" (the runner-up's exact t
    lies within the sum of the two bounds), "cand" (n, m + k) bool: the primitives the fp32 code may return}"""
    o, d = f64(o), f64(d)
    n, m = o.shape[0], len(P["geom"])
    tm = FLT_MAX if tmax is None else tmax
    res = {"hit": np.zeros(n, bool), "t": np.full(n, np.nan), "Et": np.full(n, np.nan),
           "index": np.full(n, -1, np.int64), "ill": np.zeros(n, bool), "tie": np.zeros(n, bool),
           "cand": np.zeros((n, m), bool)}
    for s in _chunks(n):
        k = s.stop - s.start
        pr = _pairs(P, o[s], d[s], _arg(tm, n, s), _arg(do, n, s), _arg(dd, n, s), _arg(dtmax, n, s))
        t = np.where(pr["state"] == HIT, pr["t"], np.inf)
        if m == 0:
            continue
        best = np.argmin(t, axis=1)  # the first of equals
        rows = np.arange(k)
        tb = t[rows, best]
        hit = np.isfinite(tb)
        Eb = np.where(hit, pr["Et"][rows, best], 0.0)
        reach = np.where(hit, tb + Eb, np.inf)
        undecided = pr["state"] == ILL
        res["ill"][s] = (undecided & (pr["tlow"] <= reach[:, None])).any(1)
        with np.errstate(invalid="ignore"):
            cand = (pr["state"] == HIT) & (t - np.where(pr["state"] == HIT, pr["Et"], 0.0) <= reach[:, None])
        cand &= hit[:, None]
        res["cand"][s] = cand
        res["tie"][s] = cand.sum(1) > 1
        res["hit"][s] = hit
        res["t"][s] = np.where(hit, tb, np.nan)
        res["Et"][s] = np.where(hit, Eb, np.nan)
        res["index"][s] = np.where(hit, best, -1)
    idx = res["index"]
    res["geom"] = np.where(idx >= 0, P["geom"][np.maximum(idx, 0)], -1).astype(np.int32)
    res["prim"] = np.where(idx >= 0, P["prim"][np.maximum(idx, 0)], -1).astype(np.int32)
    return res


def occluded(P, o, d, tmax=None, do=0.0, dd=0.0, dtmax=0.0, named=None):
    """-> {"occ" bool, "ill" bool, "ill_other" bool}: occluded when some pair is accepted under tmax beyond
    doubt; undecided when none is but some pair is undecided; ill_other: ... and one of the undecided pairs is
    not among `named` (n, m + k bool, in tie order)"""
    o, d = f64(o), f64(d)
    n = o.shape[0]
    tm = FLT_MAX if tmax is None else tmax
    occ, ill, other = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for s in _chunks(n):
        pr = _pairs(P, o[s], d[s], _arg(tm, n, s), _arg(do, n, s), _arg(dd, n, s), _arg(dtmax, n, s))
        occ[s] = (pr["state"] == HIT).any(1)
        und = pr["state"] == ILL
        ill[s] = ~occ[s] & und.any(1)
        other[s] = ill[s] if named is None else ~occ[s] & (und & ~named[s]).any(1)
    return {"occ": occ, "ill": ill, "ill_other": other}


# ---- colour -----------------------------------------------------------------------------------------------
def light_point(d, face=0):
    """quirk S2: the light's vertex[face], not a point of face `face`"""
    assert len(d["light_sources"]) == 1, "one light only (module docstring)"
    return f64(d["geometry"][d["light_sources"][0]]["vertex"])[face]


def _vec_err(e):
    return np.sqrt((e * e).sum(1))


def shading_geometry(d, P, o, dirs, hit, face=0):
    """for the rays that hit: the normal, the shadow ray and N.L with their bounds -> dict; rows of rays that
    miss hold NaN"""
    o, dirs = f64(o), f64(dirs)
    n = o.shape[0]
    t, Et = hit["t"], hit["Et"]
    with np.errstate(all="ignore"):
        dt = dirs * t[:, None]
        p = o + dt
        sphere = hit["hit"] & (hit["geom"] < 0)
        c = P["sph"][np.maximum(hit["prim"], 0)][:, :3] if len(P["sph"]) else np.zeros((n, 3))
        Pv = p - c
        E_P = Et[:, None] * np.abs(dirs) + U * (np.abs(dt) + np.abs(p) + np.abs(Pv))
        N = Pv / _len(Pv)[:, None]
        E_N = _vec_err(E_P) / _len(Pv) + 3.5 * U
        ti = np.where(hit["hit"] & ~sphere, hit["index"], 0)
        if len(P["tri"]):
            T = P["tri"][np.minimum(ti, len(P["tri"]) - 1)]
            fn = _cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
            fn = fn / _len(fn)[:, None]
            N = np.where(sphere[:, None], N, fn)
            E_N = np.where(sphere, E_N, 8 * U)  # edges, cross, normalize: a margin, not judged
        ht = dirs * (t - EPS)[:, None]
        hp = o + ht
        E_h = (Et + U * np.abs(t))[:, None] * np.abs(dirs) + U * (np.abs(ht) + np.abs(hp))
        L = light_point(d, face)[None, :] - hp
        E_L = E_h + U * np.abs(L)
        ln = _len(L)
        E_len = _vec_err(E_L) + 2.5 * U * ln
        Ld = L / ln[:, None]
        E_Ld = _vec_err(E_L) / ln + 3.5 * U
        NL = (N * Ld).sum(1)
        E_NL = (E_N + E_Ld + 3 * U) * SLACK
    return {"N": N, "E_N": E_N, "hp": hp, "E_h": _vec_err(E_h), "Ldir": Ld, "E_Ldir": E_Ld, "len": ln,
            "E_len": E_len + U * ln, "NL": NL, "E_NL": E_NL}


def materials(d, hit):
    """(n, 13) material rows of the hits (zeros for a miss)"""
    m = np.zeros((len(hit["geom"]), 13))
    for i, (g, p, h) in enumerate(zip(hit["geom"], hit["prim"], hit["hit"])):
        if h:
            m[i] = d["geometry"][g]["material"] if g >= 0 else d["sphere_materials"][p]
    return m


def colours(d, o, dirs, face=0, hit=None, P=None, unshifted_shadow_origin=False):
    """the colour of every ray in a scene with one light and ks == 0 -> {"rgb", "E_rgb", "ill", "lit", "dark",
    "either", "background", "hit", "geo", "shadow"}.  ill: the closest hit or the sign of N.L is undecided, or
    the hit is tied between primitives.  either: only the shadow ray is undecided, so the fp32 code may return
    "rgb" (the lit colour) within its bound, or exactly nothing -- and only where the undecided pairs are the
    surface the shadow ray starts from and the light's own triangle; any other undecided pair leaves the ray
    out (ill).  Quirk S2 aims every shadow ray at a VERTEX of
    the light's triangle, where u and v stand at eps and t at len - eps, each inside its margin; and the shadow
    ray starts eps off a surface whose position the fp32 chain knows to some u |o|: whether a lit point shadows
    itself, or the light hides itself, is decided by rounding in the definition.  No lit colour is therefore
    "decided"; "lit" stays empty on these scenes and "either" carries the lit pixels."""
    P = primitives(d) if P is None else P
    hit = closest_hit(P, o, dirs) if hit is None else hit
    mat = materials(d, hit)
    assert not mat[:, 6:9].any(), "ks != 0 is out of scope (module docstring)"
    g = shading_geometry(d, P, o, dirs, hit, face)
    n = len(hit["t"])
    h = hit["hit"]
    sh = {"occ": np.zeros(n, bool), "ill": np.zeros(n, bool), "ill_other": np.zeros(n, bool)}
    if h.any():
        # the two pairs that rounding decides in the definition: the surface the ray starts from, and the light
        named = np.zeros((int(h.sum()), len(P["geom"])), bool)
        named[np.arange(named.shape[0]), hit["index"][h]] = True
        named[:, P["geom"] == d["light_sources"][0]] = True
        s = occluded(P, g["hp"][h], g["Ldir"][h], g["len"][h] - EPS, g["E_h"][h], g["E_Ldir"][h], g["E_len"][h],
                     named)
        sh["occ"][h], sh["ill"][h], sh["ill_other"][h] = s["occ"], s["ill"], s["ill_other"]
    with np.errstate(invalid="ignore"):
        facing = g["NL"] > g["E_NL"]
        away = g["NL"] < -g["E_NL"]
    lit = h & facing & ~sh["occ"] & ~sh["ill"]
    dark = h & (away | sh["occ"])
    # only the own surface or the light's own triangle is undecided: the lit colour, or nothing
    either = h & facing & sh["ill"] & ~sh["ill_other"]
    ill = hit["ill"] | hit["tie"] | (h & ~lit & ~dark & ~either)
    nl = 1.0
    rgb = np.zeros((n, 3))
    amb = (mat[:, 0:3] * 0.5 + mat[:, 9:12]) / nl
    shown = lit | either
    with np.errstate(invalid="ignore"):
        rgb[shown] = (amb + mat[:, 3:6] * g["NL"][:, None] / nl)[shown]
        E = np.nan_to_num(mat[:, 3:6] * g["E_NL"][:, None] / nl) + 4 * U * np.abs(rgb)
    return {"rgb": rgb, "E_rgb": E * SLACK, "ill": ill, "lit": lit & ~ill, "dark": dark & ~ill,
            "either": either & ~ill, "background": ~h & ~ill, "hit": hit, "geo": g, "shadow": sh}


# ---- the rational cross-check -----------------------------------------------------------------------------
def exact_check(sample):
    """sample: (origins, dirs, spheres), one sphere per ray (fp32 values).  Recomputes every pair in
    fractions.Fraction -- the sign of D is exact -- and takes the roots to 60 digits through mpmath; asserts
    that the float64 path differs by less than 2^-20 of the pair's bounds (what SLACK sets aside for it), and
    that a discriminant it calls decided has the exact sign.  -> the largest share of a bound that was used"""
    import mpmath
    o, d, sph = (np.asarray(x, np.float32) for x in sample)
    worst = 0.0
    with mpmath.workdps(60):
        for i in range(len(o)):
            pr = sphere_pairs(o[i:i + 1], d[i:i + 1], sph[i:i + 1])
            fo, fd, fs = ([Fraction(float(x)) for x in v] for v in (o[i], d[i], sph[i]))
            oc = [fo[k] - fs[k] for k in range(3)]
            a = sum(x * x for x in fd)
            b = sum(x * y for x, y in zip(oc, fd))
            cc = sum(x * x for x in oc) - fs[3] * fs[3]
            D = b * b - a * cc
            D64, ED = float(pr["D"][0, 0]), float(pr["ED"][0, 0])
            err = abs(Fraction(D64) - D)
            assert err <= Fraction(ED) / (1 << 20), (i, float(err), ED)
            worst = max(worst, float(err / Fraction(ED)) if ED else 0.0)
            if abs(D64) > ED:
                assert (D > 0) == (D64 > 0), i
            if D >= 0:
                sq = mpmath.sqrt(mpmath.mpf(D.numerator) / mpmath.mpf(D.denominator))
                ma, mb = (mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator) for x in (a, b))
                for name, root in (("near", (-mb - sq) / ma), ("far", (-mb + sq) / ma)):
                    got, E = float(pr[name][0, 0]), float(pr["E" + name][0, 0])
                    if D64 < 0:  # float64 saw a negative zero-ish D: the rim, nothing to compare
                        continue
                    e = abs(mpmath.mpf(got) - root)
                    # sqrt loses digits at the rim; away from it float64 must be far inside the bound
                    if D64 > ED:
                        assert e <= mpmath.mpf(E) / (1 << 20), (i, name, float(e), E)
                        worst = max(worst, float(e / mpmath.mpf(E)))
    return worst
