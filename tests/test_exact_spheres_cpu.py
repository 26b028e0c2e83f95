"""The oracle's sphere path against exact arithmetic (tests/exact_lib.py) under derived rounding bounds: CPU.

Under test: orc_intersect_sphere through ray_oracle.sph_test / ref_queries (pinned to it pair by pair in
test_ray_queries.py) and scan_row's sphere branch through ray_oracle.ray_colours (orc_render).  The ray sets
are exact_cases.py's, the same the GPU module sends through the kernels.

Measured here with the oracle (tests/golden/exact_sphere_pins.json holds the figures; this module asserts that
today's do not exceed them): see DESIGN.md, "accuracy of the sphere definition".

What the bounds cannot tell apart, stated rather than hidden:
  - the shadow origin at t instead of t - eps: eps = 1.2e-7 is below the bound of the hit point (some u |o|,
    6e-7 at the synthetic eye's distances), so defect 5 of test_teeth is reported as not rejected (eps replaced
    by 0, defect 2, is rejected by the surface set, whose sphere is small enough for bounds far below eps);
  - whether a lit point shadows itself or the light's triangle hides its own vertex (quirk S2): every lit
    colour is "the lit colour within its bound, or nothing" (exact_lib.colours, `either`)."""
import json
import os

import numpy as np
import pytest

import exact_cases as xc
import exact_lib as xl
import ray_oracle as ro

F32 = np.float32
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_sphere_pins.json")
MEASURED = {}


def _oracle(s):
    if "oracle" not in s:
        s["oracle"] = ro.ref_queries(s["d"], s["o"], s["dirs"], s["tmax"])
    return s["oracle"]


# ---- the sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(xc.QUERY_SETS))
def test_queries_within_bounds(name):
    s = xc.QUERY_SETS[name]()
    hit, occ = _oracle(s)
    got = xc.check_queries(s, hit, occ)
    MEASURED[name] = got
    assert got["hits"] > 0, name
    if name not in ("inside", "tangent"):  # every ray of it starts inside a sphere
        assert got["misses"] > 0 and got["open"] > 0, name
    assert got["occluded"] > 0, name
    if name == "rim":
        for i in range(0, len(s["o"]), 97):  # pair by pair: the ray's own sphere is met inside its rim only
            ok, _ = ro.sph_test(s["o"][i:i + 1], s["dirs"][i:i + 1], s["d"]["spheres"][s["own"][i]])
            assert bool(ok[0]) == bool(s["want"][i] > 0), i
    if name == "inside":
        pr = xl.sphere_pairs(s["o"], s["dirs"], s["d"]["spheres"][s["own"]], paired=True)
        assert (pr["near"][:, 0] < 0).all() and (pr["state"][:, 0] == xl.HIT).all()  # the far root is the answer
    if name == "tmax":
        under = s["mult"] > 0
        assert (hit["prim"][under] >= 0).all() and (hit["prim"][~under] < 0).all()
    if name == "ties":  # duplicates: bit-equal fp32 t, the lower index wins on every ray; no band is needed
        xc.check_lower_index(s, hit)
    if name == "surface":
        xc.check_surface(s, hit)
    if name == "tangent":
        xc.check_tangent(s, hit)
    if name in ("rim", "surface"):
        xc.check_groups(s)


def test_far_bounds_still_hold():
    s = xc.far_set()
    hit, _ = _oracle(s)
    assert xc.check_far(s, hit) > 0
    for sp in s["d"]["spheres"][:32]:  # and the discriminant's bound, pair by pair
        pr = xl.sphere_pairs(s["o"], s["dirs"], sp[None])
        assert (np.abs(_fp32_disc(s["o"], s["dirs"], sp).astype(np.float64) - pr["D"][:, 0]) <= pr["ED"][:, 0]).all()


@pytest.mark.parametrize("name", ["camera/c2", "camera/c3", "camera/c4", "inside"])
def test_colours_within_bounds(name):
    s = xc.QUERY_SETS[name]()
    dirs, rgb = ro.ray_colours(s["d"], s["o"], s["a"])
    ro.assert_same(dirs, s["dirs"], "the oracle's camera gives the set's directions")
    with open(PINS) as f:
        pin = json.load(f)["black/" + name]
    MEASURED[name + "/colour_left_out"] = xc.check_colours(s, rgb, black_pin=pin)


# ---- the bounds are not slack -------------------------------------------------------------------------------
def _fp32_disc(o, d, sph):
    """sph_test's chain up to disc"""
    oc = o - sph[:3]
    b = ro.dot(oc, d)
    return (b * b - (ro.dot(oc, oc) - sph[3] * sph[3])).astype(F32)


def _fp32_nl(d, s, t, prim):
    """scan_row's sphere branch in numpy fp32: N = normalize((o + d t) - c), L = normalize(P - (o + d (t - eps)))"""
    o, dr = s["o"], s["dirs"]
    c = d["spheres"][prim, :3]
    N = ro.normalize((((o + (dr * t[:, None]).astype(F32)).astype(F32)) - c).astype(F32))
    hp = (o + (dr * (t - ro.EPS).astype(F32)[:, None]).astype(F32)).astype(F32)
    L = ro.normalize((xl.light_point(d).astype(F32)[None] - hp).astype(F32))
    return ro.dot(N, L)


def _slack(config):
    if "slack/" + config in MEASURED:
        return MEASURED["slack/" + config]
    worst = {"disc": 0.0, "t": 0.0, "NL": 0.0, "t_over_r": 0.0, "NL_err": 0.0, "rim_band": 0.0}
    for s in (xc.camera_set(config), xc.shadow_set(config)):
        d = s["d"]
        rim = aimed = 0
        for k, sp in enumerate(d["spheres"]):
            pr = xl.sphere_pairs(s["o"], s["dirs"], sp[None])
            r = np.abs(_fp32_disc(s["o"], s["dirs"], sp).astype(np.float64) - pr["D"][:, 0]) / pr["ED"][:, 0]
            worst["disc"] = max(worst["disc"], float(r.max()))
            rim += int((np.abs(pr["D"][:, 0]) <= pr["ED"][:, 0]).sum())
            aimed += int((pr["D"][:, 0] > -pr["ED"][:, 0]).sum())
            ok, t2 = ro.sph_test(s["o"], s["dirs"], sp)
            both = ok & (pr["state"][:, 0] == xl.HIT)
            if both.any():
                e = np.abs(t2[both].astype(np.float64) - pr["t"][both, 0])
                worst["t"] = max(worst["t"], float((e / pr["Et"][both, 0]).max()))
                worst["t_over_r"] = max(worst["t_over_r"], float(e.max() / sp[3]))
        if s["name"].startswith("camera"):
            worst["rim_band"] = rim / max(aimed, 1)
            hit, _ = _oracle(s)
            h = s["ref"]["hit"]
            sel = h["hit"] & (h["geom"] < 0) & ~h["ill"] & ~h["tie"] & (hit["prim"] == h["prim"])
            g = s["ref"]["rgb"]["geo"]
            sub = {"o": s["o"][sel], "dirs": s["dirs"][sel]}
            e = np.abs(_fp32_nl(d, sub, hit["t"][sel], hit["prim"][sel]).astype(np.float64) - g["NL"][sel])
            worst["NL"] = float((e / g["E_NL"][sel]).max())
            worst["NL_err"] = float(e.max())
    print(f"{config}: " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))
    MEASURED["slack/" + config] = worst
    return worst


@pytest.mark.parametrize("config", ["c2", "c3", "c4"])
def test_bounds_are_not_slack(config):
    worst = _slack(config)
    assert 0.1 <= worst["disc"] <= 1.0, worst
    assert 0.1 <= worst["t"] <= 1.0, worst
    assert 0.05 <= worst["NL"] <= 1.0, worst


def test_exact_check():
    s = xc.camera_set("c4")
    rng = np.random.default_rng(0xE5)
    h = s["ref"]["hit"]
    rays = rng.choice(np.flatnonzero(h["hit"] & (h["geom"] < 0)), 128)
    sph = np.concatenate([s["d"]["spheres"][h["prim"][rays]],  # the sphere the ray meets, and any sphere
                          s["d"]["spheres"][rng.integers(0, len(s["d"]["spheres"]), 128)]])
    rays = np.concatenate([rays, rays])
    used = xl.exact_check((s["o"][rays], s["dirs"][rays], sph))
    print(f"float64 used {used:.3g} of a bound at most (2^-20 = {2.0 ** -20:.3g} is set aside)")
    assert used <= 2.0 ** -20


# ---- teeth --------------------------------------------------------------------------------------------------
def _sph_test(o, d, sph, far_first=False, eps=ro.EPS):
    """a private copy of ray_oracle.sph_test that takes the defects"""
    with np.errstate(all="ignore"):
        oc = o - sph[:3]
        b = ro.dot(oc, d)
        cc = ro.dot(oc, oc) - sph[3] * sph[3]
        disc = b * b - cc
        ok = ~(disc < F32(0))
        sq = np.sqrt(disc)
        t2 = (-b + sq) if far_first else (-b - sq)
        t2 = np.where(t2 < eps, (-b - sq) if far_first else (-b + sq), t2).astype(F32)
        ok &= ~(t2 < eps)
    return ok, t2


def _queries(d, o, dirs, tmax=None, strict=False, **kw):
    """ray_oracle.ref_queries over the private sph_test; strict: `>` in place of `>=` at the bound"""
    n = o.shape[0]
    t0 = np.full(n, ro.FLT_MAX, F32) if tmax is None else tmax.copy()
    t, geom, prim, occ = t0.copy(), np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, bool)
    beyond = (lambda x, y: x > y) if strict else (lambda x, y: x >= y)
    for gi, g in enumerate(d["geometry"]):
        for f, fi in enumerate(g["face_index"]):
            ok, t2, _, _ = ro.tri_test(o, dirs, g["vertex"][fi[0]], g["vertex"][fi[1]], g["vertex"][fi[2]])
            occ |= ok & ~(t2 >= t0)
            acc = ok & ~(t2 >= t)
            t[acc], geom[acc], prim[acc] = t2[acc], gi, f
    for k, sp in enumerate(d["spheres"]):
        ok, t2 = _sph_test(o, dirs, sp, **kw)
        occ |= ok & ~beyond(t2, t0)
        acc = ok & ~beyond(t2, t)
        t[acc], geom[acc], prim[acc] = t2[acc], -1, k
    return {"t": t, "geom": geom, "prim": prim}, occ.astype(np.uint8)


def _shade(d, o, dirs, flip=False, shift=ro.EPS):
    """scan_row for one light and ks = 0 in numpy fp32 over ref_queries; flip: the sphere normal negated;
    shift: what the shadow origin stands back by"""
    hit, _ = ro.ref_queries(d, o, dirs)
    n = len(o)
    rgb = np.zeros((n, 3), F32)
    h = np.flatnonzero(hit["prim"] >= 0)
    N, _, _ = ro.normals_and_ks(d, {k: v[h] for k, v in hit.items()}, o[h], dirs[h])
    sph = hit["geom"][h] < 0
    N[sph & flip] *= F32(-1)
    t = hit["t"][h]
    hp = (o[h] + (dirs[h] * (t - F32(shift)).astype(F32)[:, None]).astype(F32)).astype(F32)
    L = (xl.light_point(d).astype(F32)[None] + F32(0) - hp).astype(F32)
    ln = np.sqrt(ro.dot(L, L))
    Ld = ro.normalize(L)
    _, occ = ro.ref_queries(d, hp, Ld, (ln - ro.EPS).astype(F32))
    nl = ro.dot(N, Ld)
    mat = np.array([d["geometry"][g]["material"] if g >= 0 else d["sphere_materials"][p]
                    for g, p in zip(hit["geom"][h], hit["prim"][h])], F32)
    c = ((mat[:, 0:3] * F32(0.5)).astype(F32) + mat[:, 9:12]).astype(F32)
    c = (c + (mat[:, 3:6] * nl[:, None]).astype(F32)).astype(F32)
    c[(occ > 0) | ~(nl > 0)] = 0
    rgb[h] = c
    return rgb


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_teeth():
    quiet = lambda *a: None
    cam, ins, tie = xc.camera_set("c2"), xc.inside_set(), xc.ties_set()
    # the private copies are the oracle's while they carry no defect
    for s in (cam, ins, tie):
        a, b = _queries(s["d"], s["o"], s["dirs"], s["tmax"]), _oracle(s)
        assert all(np.array_equal(a[0][k], b[0][k]) for k in ("geom", "prim")) and np.array_equal(a[1], b[1])
        ro.assert_same(a[0]["t"], b[0]["t"], "private copy")
    _, want = ro.ray_colours(cam["d"], cam["o"], cam["a"])
    ro.assert_same(_shade(cam["d"], cam["o"], cam["dirs"]), want, "private shade")

    def q(s, **kw):
        return lambda: xc.check_queries(s, *_queries(s["d"], s["o"], s["dirs"], s["tmax"], **kw), out=quiet)

    def c(**kw):
        return lambda: xc.check_colours(cam, _shade(cam["d"], cam["o"], cam["dirs"], **kw), out=quiet)
    found = {"far root first": _rejected(q(cam, far_first=True)),
             "eps = 0": _rejected(q(xc.surface_set(), eps=F32(0))),
             "> at tmax": _rejected(lambda: xc.check_lower_index(
                 tie, _queries(tie["d"], tie["o"], tie["dirs"], tie["tmax"], strict=True)[0])),
             "normal negated": _rejected(c(flip=True)),
             "shadow origin at t": _rejected(c(shift=0.0))}
    print(found)
    # eps = 1.2e-7 lies below the bound of the hit point at the synthetic scenes' distances (u |o| alone is
    # 6e-7), and whether a lit point shadows itself is decided by rounding there: leaving the shadow origin at
    # t moves no colour out of its bound.  Stated in DESIGN.md; no bound is narrowed to make it show.
    for k in ("far root first", "eps = 0", "> at tmax", "normal negated"):
        assert found[k], k
    MEASURED["teeth"] = found


# ---- the regression pin ---------------------------------------------------------------------------------------
def test_pins():
    """today's maxima do not exceed the recorded ones (a regression pin; the bound is the pass/fail rule)"""
    with open(PINS) as f:
        pins = json.load(f)
    for config in ("c2", "c3", "c4"):
        for k, v in _slack(config).items():
            assert v <= pins["slack/" + config][k] * (1 + 1e-12), (config, k, v)
