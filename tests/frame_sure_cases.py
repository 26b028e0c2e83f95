"""Scenes, cameras and rays that hunt statement (I) of DESIGN.md 3.9 "Frames that need no fallback": for a
camera the host predicate accepts (Scene.shadow_origins_inside, host/scene_tables.cpp), every shadow origin
ro = fl(o + d fl(t - eps)) of an accepted primary hit lies in the grown scene box.  Plain module: no pytest
here.  tests/test_frame_sure_hunt_cpu.py runs the hunt on the CPU, tests/test_frame_sure_hunt.py renders the
frames on the GPU.

Scenes (one one-face light, fewer than 64 triangles, 64 spheres or more, so that the launch can take SURE):
a floor turned by a fixed rotation and moved off the origin under a sphere cloud ("tilted"), the same 1e3,
1e5 and 1e6 away ("far 1e3" ...), a slab of 100 x 0.1 x 100, one sphere of half the box's extent with small
ones inside and outside it, spheres tangent to the faces of the ungrown box, and the tilted scene with a
sliver, which no camera may pass.

Cameras per scene: along eight directions from the box's middle the last fp32 eye the predicate accepts and
the first it refuses (bisection), an eye near the box's middle, eyes 128 and 512 box sizes out; over a floor,
at five places along its plane (two over it, three beyond its edge) the lowest accepted eye, and the eyes at
height 0 and +-1e-7.  One "box size" is S, the sum of the grown box's extents (the proof's S).

Rays per camera, seeded: a cube map of all directions; per sphere, directions within 1e-9 .. 1e-3 (relative)
of its tangent cone on both sides; per triangle, directions whose component along the normal is 1e-3 .. 10
times (camera height / longest edge), and exactly 0, at all azimuths; per triangle, directions aimed within
1e-7 .. 1 (times the longest edge) of its edges and corners.  All normalised in fp32 as the kernels do.

The arithmetic is ray_oracle's (tri_test, sph_test, ref_queries), which test_ray_queries.py pins pair by
pair to the oracle; the verdict is a callable, the product's by default."""
import functools

import numpy as np

import oracle_lib as ol
import ray_oracle as ro

F32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def rotation(axis=(0.36, 0.48, 0.8), angle=0.7):
    """Rodrigues: a fixed turn about no coordinate axis"""
    k = _unit(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


ROT = rotation()
DIRECTIONS = [_unit(v) for v in ((1, 0.02, 0.01), (0.01, 1, -0.02), (0.02, -0.01, -1), (1, 1, 1), (-1, 0.5, 0.3),
                                 (0.2, -1, 0.6), (-0.6, -0.3, -1), (0.7, 0.25, -0.7))]
SLAB_DIRECTIONS = [_unit(v) for v in ((1, 0.5, 0.01), (0.01, 1, -0.02), (0.02, 0.4, -1), (1, 1, 1), (-1, 0.5, 0.3),
                                      (0.2, -1, 0.6), (-0.6, -0.3, -1), (0.7, 0.25, -0.7))]
IN_PLANE = [(0.3, 0.2), (-0.7, 0.6), (1.5, 0.4), (3.0, -2.0), (6.0, 0.5)]  # (a, b) in units of the floor's half side


# ---- scenes -------------------------------------------------------------------------------------------
def _grey(n):
    return np.stack([ol.material13(ka=(0.3 + 0.004 * (k % 100), 0.45, 0.6), kd=(0.4 + 0.004 * (k % 100), 0.5, 0.7))
                     for k in range(n)])


def _build(name, tris, sph, light, rot, centre, light_size=0.3, floor_half=None, directions=None):
    """local coordinates -> the scene: x -> rot x + centre, rounded to fp32 once"""
    centre = np.asarray(centre, np.float64)

    def xf(q):
        return np.asarray(q, np.float64) @ rot.T + centre
    geoms = []
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    if len(tris):
        geoms.append({"vertex": xf(tris.reshape(-1, 3)).astype(F32), "face_index": np.arange(3 * len(tris)).reshape(-1, 3),
                      "material": ol.WHITE})
    p = np.asarray(light, np.float64)
    lv = np.array([p, p + (light_size, 0.0, 0.2 * light_size), p + (0.0, 0.3 * light_size, light_size)])
    geoms.append({"vertex": xf(lv).astype(F32), "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_A})
    sph = np.asarray(sph, np.float64).reshape(-1, 4)
    s = np.concatenate([xf(sph[:, :3]), sph[:, 3:]], axis=1).astype(F32)
    d = ol.scene_dict(geoms, s, _grey(len(s)))
    sc = ol.scene_to_product(d)
    hdr = sc.table("header").view(F32)
    case = {"name": name, "d": d, "sc": sc, "lo": hdr[4:7].copy(), "hi": hdr[7:10].copy(),
            "floor": None, "directions": directions or DIRECTIONS}
    lo, hi = case["lo"].astype(np.float64), case["hi"].astype(np.float64)
    case["mid"], case["S"] = 0.5 * (lo + hi), float((hi - lo).sum())
    if floor_half is not None:  # the plane of the first floor triangle as fp32 stores it
        v = geoms[0]["vertex"][:3].astype(np.float64)
        n = _unit(np.cross(v[1] - v[0], v[2] - v[0]))
        case["floor"] = {"p0": xf((0.0, 0.0, 0.0)), "n": n, "u": rot @ (1.0, 0.0, 0.0), "v": rot @ (0.0, 0.0, 1.0),
                         "half": floor_half, "v0": v[0]}
    return case


def _floor(h):
    a, b, c, e = (-h, 0.0, -h), (h, 0.0, h), (h, 0.0, -h), (-h, 0.0, h)
    return [[a, b, c], [a, e, b]]  # both normals +y, towards the light


def _cloud():
    rng = np.random.default_rng(7)
    n = 96
    return np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(0.4, 4.0, n), rng.uniform(-4.5, 4.5, n),
                     rng.uniform(0.1, 0.4, n)], axis=1)


TILTED_CENTRE = np.array([3.7, -2.3, 5.1])
FAR_ALONG = np.array([1.0, -0.6, 0.8])


def _tilted(name="tilted", shift=0.0, extra=None):
    tris = _floor(5.0) + (extra or [])
    return _build(name, tris, _cloud(), (0.3, 7.0, -0.2), ROT, TILTED_CENTRE + shift * FAR_ALONG, floor_half=5.0)


def _slab():
    rng = np.random.default_rng(11)
    n = 128
    s = np.stack([rng.uniform(-49, 49, n), rng.uniform(0.03, 0.07, n), rng.uniform(-49, 49, n),
                  rng.uniform(0.01, 0.025, n)], axis=1)
    return _build("slab", _floor(50.0), s, (0.3, 0.09, -0.2), np.eye(3), (12.0, 2.0, -7.0), light_size=0.03,
                  floor_half=50.0, directions=SLAB_DIRECTIONS)


def _big_sphere():
    rng = np.random.default_rng(13)
    n = 80
    small = np.concatenate([rng.uniform(-4.8, 4.8, (n, 3)), rng.uniform(0.05, 0.15, (n, 1))], axis=1)
    return _build("big sphere", [], np.concatenate([[(0.0, 0.0, 0.0, 5.0)], small]), (4.0, 4.3, -4.0), np.eye(3),
                  (-6.0, 4.0, 2.5))


def _touching():
    """16 spheres per face of the box [-4, 4]^3 + (2, 1, -3), radius a multiple of 1/4, centre 4 - r from the
    middle along the face's axis: centre +- r is the face's coordinate exactly, in fp32 too"""
    rng = np.random.default_rng(17)
    s = []
    for a in range(3):
        for sign in (-1.0, 1.0):
            for k in range(16):
                r = 0.25 * (1 + k % 4)
                c = np.round(rng.uniform(-3.0, 3.0, 3) * 16.0) / 16.0
                c[a] = sign * (4.0 - r)
                s.append(list(c) + [r])
    return _build("touching", [], s, (0.5, 1.0, 0.25), np.eye(3), (2.0, 1.0, -3.0))


def _sliver():
    # three collinear points: what area the triangle has comes from the rounding of its corners
    return _tilted("sliver", extra=[[(-3.0, 1.0, 0.0), (3.0, 1.0, 0.0), (0.0, 1.0, 0.0)]])


SCENES = {"tilted": _tilted, "far 1e3": lambda: _tilted("far 1e3", 1e3), "far 1e5": lambda: _tilted("far 1e5", 1e5),
          "far 1e6": lambda: _tilted("far 1e6", 1e6), "slab": _slab, "big sphere": _big_sphere, "touching": _touching,
          "sliver": _sliver}
# "sliver": the predicate must refuse every camera.  "far 1e6": it refuses every camera a box size or more out (e_fp
# alone exceeds the margin there); what it accepts next to the scene is held to statement (I) all the same
NEVER = ("sliver", "far 1e6")
SOUND = [n for n in SCENES if n not in NEVER]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


# ---- cameras ------------------------------------------------------------------------------------------
def eye32(p):
    return tuple(float(x) for x in np.asarray(p, np.float64).astype(F32))


def product_verdict(case):
    return lambda eye: bool(case["sc"].shadow_origins_inside(eye))


def along(case, k, s):
    """the fp32 eye s box sizes from the box's middle along direction k"""
    return eye32(case["mid"] + s * case["S"] * case["directions"][k])


def over_floor(case, ab, h):
    """the fp32 eye at in-plane place ab (units of the floor's half side) and height h over the floor's plane"""
    f = case["floor"]
    return eye32(f["p0"] + f["half"] * (ab[0] * f["u"] + ab[1] * f["v"]) + h * f["n"])


def bisect(yes, at, s_yes, s_no):
    """yes(at(s_yes)) and not yes(at(s_no)) -> (last accepted eye, first refused eye) between them: fp32 eyes
    that at() no longer tells apart from one another's neighbours"""
    assert yes(at(s_yes)) and not yes(at(s_no))
    while True:
        m = 0.5 * (s_yes + s_no)
        e = at(m)
        if e == at(s_yes) or e == at(s_no) or m == s_yes or m == s_no:
            return at(s_yes), at(s_no)
        if yes(e):
            s_yes = m
        else:
            s_no = m


def height_of(case, eye):
    f = case["floor"]
    return float((np.asarray(eye, np.float64) - f["v0"]) @ f["n"])


@functools.lru_cache(maxsize=None)
def cameras(name):
    """-> list of {"eye", "kind", "where"}; kinds: "inside", "at 4", "last yes", "first no", "far 128", "far 512",
    "lowest", "plane 0", "plane +1e-7", "plane -1e-7".  The bisections ask the product's predicate; where it
    refuses both ends there is no "last yes" / "lowest" camera."""
    case = scene(name)
    yes = product_verdict(case)
    cams = [{"eye": eye32(case["mid"] + 0.01 * case["S"] * _unit((0.3, 0.5, -0.4))), "kind": "inside", "where": None}]
    for k in range(len(case["directions"])):
        cams.append({"eye": along(case, k, 4.0), "kind": "at 4", "where": k})
        for s in (128.0, 512.0):
            cams.append({"eye": along(case, k, s), "kind": f"far {s:.0f}", "where": k})
        if yes(along(case, k, 4.0)) and not yes(along(case, k, 128.0)):
            a, b = bisect(yes, lambda s: along(case, k, s), 4.0, 128.0)
            cams += [{"eye": a, "kind": "last yes", "where": k}, {"eye": b, "kind": "first no", "where": k}]
    if case["floor"] is not None:
        top = 0.25 * case["S"]
        for ab in IN_PLANE:
            for kind, h in (("plane 0", 0.0), ("plane +1e-7", 1e-7), ("plane -1e-7", -1e-7)):
                cams.append({"eye": over_floor(case, ab, h), "kind": kind, "where": ab})
            if yes(over_floor(case, ab, top)) and not yes(over_floor(case, ab, 0.0)):
                a, _ = bisect(yes, lambda h: over_floor(case, ab, h), top, 0.0)
                cams.append({"eye": a, "kind": "lowest", "where": ab})
    return cams


def pick(name, kind, where=None):
    out = [c for c in cameras(name) if c["kind"] == kind and (where is None or c["where"] == where)]
    assert out, f"{name}: no camera of kind {kind!r} at {where}"
    return out


# ---- rays ---------------------------------------------------------------------------------------------
def triangles_of(d):
    return np.concatenate([g["vertex"][g["face_index"].astype(int)] for g in d["geometry"]]).astype(F32)


def _perp(axis):
    """unit vectors (u, v) square to the unit vectors axis (n, 3) and to each other"""
    e = np.where((np.abs(axis[:, 2]) < 0.9)[:, None], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    u = np.cross(axis, e)
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u, np.cross(axis, u)


def _finish(v):
    """float64 vectors -> fp32 directions normalised as the kernels normalise (vec.h:135 in fp32)"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v / np.abs(v).max(axis=1)[:, None]  # a scale that keeps the squares in range
    with np.errstate(all="ignore"):
        d = ro.normalize(v.astype(F32))
    return d[np.isfinite(d).all(axis=1)]


def cube_map_rays(n=26):
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    a, b = (x.ravel() for x in np.meshgrid(c, c))
    out = []
    for m in range(3):
        for s in (1.0, -1.0):
            v = np.zeros((n * n, 3))
            v[:, m], v[:, (m + 1) % 3], v[:, (m + 2) % 3] = s, a, b
            out.append(v)
    return _finish(np.concatenate(out))


def limb_rays(case, eye, rng, total=4000):
    """per sphere the camera is outside of: directions at (1 + delta) times the tangent angle, |delta| log-uniform
    in 1e-9 .. 1e-3, either sign, every azimuth"""
    sph = case["d"]["spheres"].astype(np.float64)
    w = sph[:, :3] - np.asarray(eye, np.float64)
    dist = np.linalg.norm(w, axis=1)
    out = dist > sph[:, 3]
    w, dist, r = w[out], dist[out], sph[out, 3]
    if not len(w):
        return np.zeros((0, 3), F32)
    k = max(8, total // len(w))
    axis = w / dist[:, None]
    u, v = _perp(axis)
    delta = 10.0 ** rng.uniform(-9, -3, (len(w), k)) * rng.choice([-1.0, 1.0], (len(w), k))
    theta = np.arcsin(r / dist)[:, None] * (1.0 + delta)
    phi = rng.uniform(0, 2 * np.pi, (len(w), k))
    d = np.cos(theta)[..., None] * axis[:, None, :] + np.sin(theta)[..., None] * (
        np.cos(phi)[..., None] * u[:, None, :] + np.sin(phi)[..., None] * v[:, None, :])
    return _finish(d)


def _tri_frames(case, eye):
    """per triangle with an area: (v (3, 3), unit normal, camera height, longest edge)"""
    out = []
    for t in triangles_of(case["d"]).astype(np.float64):
        n = np.cross(t[1] - t[0], t[2] - t[0])
        ell = max(np.linalg.norm(t[(i + 1) % 3] - t[i]) for i in range(3))
        if np.linalg.norm(n) > 1e-12 * ell * ell:
            n = n / np.linalg.norm(n)
            out.append((t, n, float((np.asarray(eye, np.float64) - t[0]) @ n), ell))
    return out


def grazing_rays(case, eye, rng, total=4000):
    """per triangle: d = dn n + sqrt(1 - dn^2) (in-plane unit vector), dn = -k h / l with k log-uniform in
    1e-3 .. 10 (h the camera's height over the plane, l the longest edge), every fifth dn exactly 0; half the
    azimuths uniform, half towards a random point of the triangle"""
    frames = _tri_frames(case, eye)
    k = max(200, total // max(len(frames), 1))
    out = []
    for t, n, h, ell in frames:
        u, v = _perp(n[None, :])
        dn = np.clip(-(10.0 ** rng.uniform(-3, 1, k)) * h / ell, -0.999, 0.999)
        dn[::5] = 0.0
        phi = rng.uniform(0, 2 * np.pi, k)
        bary = rng.dirichlet((1.0, 1.0, 1.0), k) @ t - np.asarray(eye, np.float64)
        aimed = np.arctan2(bary @ v[0], bary @ u[0])
        phi[1::2] = aimed[1::2]
        flat = np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v
        out.append(dn[:, None] * n + np.sqrt(1.0 - dn * dn)[:, None] * flat)
    return _finish(np.concatenate(out)) if out else np.zeros((0, 3), F32)


def edge_rays(case, eye, rng, total=4000):
    """per triangle: aimed at v_i + s (v_j - v_i) + q m, m the in-plane normal of edge ij (for every third ray
    s is 0 or 1: a corner, and m any in-plane direction), q = +-l 10^U(-7, 0)"""
    frames = _tri_frames(case, eye)
    k = max(200, total // max(len(frames), 1))
    out = []
    for t, n, _, ell in frames:
        i = rng.integers(0, 3, k)
        a, b = t[i], t[(i + 1) % 3]
        s = rng.uniform(0, 1, k)
        s[::3] = rng.integers(0, 2, len(s[::3]))
        e = b - a
        m = np.cross(e, n)
        m /= np.linalg.norm(m, axis=1)[:, None]
        psi = rng.uniform(0, 2 * np.pi, k)
        eh = e / np.linalg.norm(e, axis=1)[:, None]
        m[::3] = (np.cos(psi)[:, None] * m + np.sin(psi)[:, None] * eh)[::3]
        q = ell * 10.0 ** rng.uniform(-7, 0, k) * rng.choice([-1.0, 1.0], k)
        out.append(a + s[:, None] * e + q[:, None] * m - np.asarray(eye, np.float64))
    return _finish(np.concatenate(out)) if out else np.zeros((0, 3), F32)


KINDS = ("cube map", "limb", "grazing", "edge")


def rays(case, eye, seed=0, kinds=KINDS, total=4000):
    """-> {kind: (n, 3) fp32 unit directions}, about `total` of each kind"""
    rng = np.random.default_rng([seed, 2024])
    make = {"cube map": lambda: cube_map_rays(max(2, int(round((total / 6.0) ** 0.5)))),
            "limb": lambda: limb_rays(case, eye, rng, total), "grazing": lambda: grazing_rays(case, eye, rng, total),
            "edge": lambda: edge_rays(case, eye, rng, total)}
    return {k: make[k]() for k in KINDS if k in kinds}


# ---- the shadow origins -------------------------------------------------------------------------------
def origin_of(o, dirs, t):
    """scan_row's hitp = origin + dir * (t - eps), one fp32 rounding per step (main.cpp:757-758)"""
    with np.errstate(all="ignore"):
        return (o + (dirs * (t - ro.EPS).astype(F32)[:, None]).astype(F32)).astype(F32)


def shadow_origins(d, eye, dirs):
    """-> (closest, every): `closest` = {"ray", "ro"}: the fp32 shadow origin of each ray's closest accepted hit
    (ro.ref_queries); `every` = {"ray", "ro", "t", "tri" (-1: a sphere), "sph" (-1: a triangle), "uv"}: one entry
    per (ray, primitive) whose test accepts the ray at all (ro.tri_test / ro.sph_test, the tests ref_queries is
    made of) -- a hit is the closest one of some ray from the same eye whenever nothing nearer is in the way,
    so statement (I) is held to all of them"""
    dirs = np.ascontiguousarray(dirs, F32)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(eye, F32), dirs.shape))
    hit, _ = ro.ref_queries(d, o, dirs)
    ok = hit["prim"] >= 0
    closest = {"ray": np.flatnonzero(ok), "ro": origin_of(o[ok], dirs[ok], hit["t"][ok])}
    cols = {k: [] for k in ("ray", "ro", "t", "tri", "sph", "uv")}

    def keep(acc, t2, tri, sph, uv):
        r = np.flatnonzero(acc)
        cols["ray"].append(r)
        cols["ro"].append(origin_of(o[r], dirs[r], t2[r]))
        cols["t"].append(t2[r])
        cols["tri"].append(np.full(len(r), tri))
        cols["sph"].append(np.full(len(r), sph))
        cols["uv"].append(uv[r])
    for i, tv in enumerate(triangles_of(d)):
        acc, t2, u2, v2 = ro.tri_test(o, dirs, tv[0], tv[1], tv[2])
        keep(acc, t2, i, -1, np.stack([u2, v2], axis=1))
    zero = np.zeros((len(dirs), 2), F32)
    for i, s in enumerate(d["spheres"]):
        acc, t2 = ro.sph_test(o, dirs, s)
        keep(acc, t2, -1, i, zero)
    every = {k: np.concatenate(v) for k, v in cols.items()}
    # the closest hit is one of them: same t, same origin bits
    assert np.isin(closest["ray"], every["ray"]).all()
    return closest, every


def outside(case, p):
    """shadow_wave_lists' test: fp32 compares against scene_lo / scene_hi; anything not inside is outside"""
    p = np.asarray(p, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return ~((p >= case["lo"]) & (p <= case["hi"])).all(axis=1)


# ---- the proof's terms, for the report only -----------------------------------------------------------
def proof_terms(case, eye):
    """DESIGN.md 3.9 restated in float64: M, m, e_fp, e_sph and per triangle 4.01 Q / D_min (inf where
    D_min <= 0 or the triangle is a pad)"""
    lo, hi = case["lo"].astype(np.float64), case["hi"].astype(np.float64)
    o = np.asarray(eye, np.float64)
    S = float((hi - lo).sum())
    A = float(np.maximum(np.abs(lo), np.abs(hi)).max())
    M = float(np.sqrt((np.maximum(np.abs(o - lo), np.abs(o - hi)) ** 2).sum()))
    m = S / 26.0 - 2.0 ** -22 * A
    cu = 2.0 ** -20
    bound = []
    for t in triangles_of(case["d"]):
        e1, e2 = (t[1] - t[0]).astype(np.float64), (t[2] - t[0]).astype(np.float64)  # the fp32 edges
        w = o - t[0].astype(np.float64)
        n = np.cross(e1, e2)
        L1, L2, A2 = np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(n)
        W = 1.0001 * np.linalg.norm(w)
        Q = cu * W * L1 * L2
        with np.errstate(all="ignore"):
            Dmin = min(0.5 * A2 - cu * L1 * L2, (0.86 * abs(w @ n) - 3.0 * Q) / (1.0001 * (L1 + L2 + W)))
        bound.append(4.01 * Q / Dmin if Dmin > 0.0 else np.inf)
    return {"S": S, "M": M, "m": m, "e_fp": 2.0 ** -20 * (1.0 + M + m + float(np.abs(o).max())), "e_sph": 2.0 ** -8 * M,
            "tri_bound": np.array(bound)}


def worst_ratios(case, eye, dirs, every):
    """the largest distance of X = o + d t (float64, for the accepted fp32 t) from its primitive, over e_sph and
    over the triangle's own 4.01 Q / D_min: spheres | |X - c| - r |, triangles |X - (v0 + u e1 + v e2)|"""
    terms = proof_terms(case, eye)
    o = np.asarray(eye, F32).astype(np.float64)
    X = o + dirs[every["ray"]].astype(np.float64) * every["t"].astype(np.float64)[:, None]
    r_sph = r_tri = 0.0
    is_s = every["sph"] >= 0
    if is_s.any():
        s = case["d"]["spheres"][every["sph"][is_s]].astype(np.float64)
        off = np.abs(np.linalg.norm(X[is_s] - s[:, :3], axis=1) - s[:, 3])
        r_sph = float(off.max() / terms["e_sph"])
    is_t = ~is_s
    if is_t.any():
        t = triangles_of(case["d"])[every["tri"][is_t]]
        e1, e2 = (t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64)
        uv = every["uv"][is_t].astype(np.float64)
        Y = t[:, 0].astype(np.float64) + uv[:, :1] * e1 + uv[:, 1:] * e2
        r_tri = float((np.linalg.norm(X[is_t] - Y, axis=1) / terms["tri_bound"][every["tri"][is_t]]).max())
    return r_sph, r_tri


# ---- the hunt -----------------------------------------------------------------------------------------
def hunt(name, verdict=None, cams=None, kinds=KINDS, seed=0, total=4000):
    """for every camera of `cams` (default: all of cameras(name)) that verdict(eye) accepts (default: the
    product's predicate): about `total` rays of each of `kinds`, every accepted hit's shadow origin, the count outside the box.
    -> {"yes", "no", "rays", "origins", "escaped": [(camera, kind of ray, count outside, worst excess)],
        "worst_sph", "worst_tri"}"""
    case = scene(name)
    verdict = verdict or product_verdict(case)
    rep = {"name": name, "yes": 0, "no": 0, "rays": 0, "origins": 0, "escaped": [], "worst_sph": 0.0, "worst_tri": 0.0}
    for ci, cam in enumerate(cameras(name) if cams is None else cams):
        if not verdict(cam["eye"]):
            rep["no"] += 1
            continue
        rep["yes"] += 1
        for kind, dirs in rays(case, cam["eye"], seed + ci, kinds, total).items():
            if not len(dirs):
                continue
            closest, every = shadow_origins(case["d"], cam["eye"], dirs)
            rep["rays"] += len(dirs)
            rep["origins"] += len(every["ray"])
            out = outside(case, every["ro"])
            assert not (outside(case, closest["ro"]).any() and not out.any())
            if out.any():
                p = every["ro"][out].astype(np.float64)
                excess = np.nanmax(np.maximum(case["lo"] - p, p - case["hi"]))
                rep["escaped"].append((cam, kind, int(out.sum()), float(excess)))
            a, b = worst_ratios(case, cam["eye"], dirs, every)
            rep["worst_sph"], rep["worst_tri"] = max(rep["worst_sph"], a), max(rep["worst_tri"], b)
    return rep


def n_escaped(rep):
    return sum(e[2] for e in rep["escaped"])


def assert_sound(rep):
    """statement (I): no accepted camera has a shadow origin outside the box"""
    assert not rep["escaped"], f"{rep['name']}: accepted cameras with shadow origins outside the box: " + "; ".join(
        f"{c['kind']} {c['where']} eye {c['eye']}: {n} of the {kind} rays, by up to {x:.3g}"
        for c, kind, n, x in rep["escaped"][:6])


# ---- frames for the GPU tests -------------------------------------------------------------------------
def limb_view(case, eye):
    """-> (look, vfov): a frame centred on the limb of the sphere nearest the eye (the first sphere where the
    first is the scene's big one) on the light's side, as tall as the sphere's angular radius"""
    sph = case["d"]["spheres"].astype(np.float64)
    o = np.asarray(eye, np.float64)
    dist = np.linalg.norm(sph[:, :3] - o, axis=1)
    i = 0 if case["name"] == "big sphere" else int(np.argmin(dist - sph[:, 3]))
    axis = (sph[i, :3] - o) / dist[i]
    to_light = case["d"]["geometry"][case["d"]["light_sources"][0]]["vertex"][0].astype(np.float64) - sph[i, :3]
    u = _unit(to_light - (to_light @ axis) * axis)  # the limb on the light's side
    look = sph[i, :3] + sph[i, 3] * u
    return eye32(look), float(np.degrees(np.arcsin(min(1.0, sph[i, 3] / dist[i]))))


def whole_view(case, eye):
    """-> (look, vfov): the box's middle, the frame as tall as the grown box's diagonal looks from the eye"""
    o = np.asarray(eye, np.float64)
    diag = np.linalg.norm(case["hi"].astype(np.float64) - case["lo"].astype(np.float64))
    return eye32(case["mid"]), float(np.degrees(2.0 * np.arctan(0.5 * diag / np.linalg.norm(case["mid"] - o))))


def floor_view(case, eye):
    """-> (look, vfov): along the floor towards the middle of its edge farthest from the eye; the frame is four
    times as tall as the edge's depression below the eye's horizon, and no taller than the floor looks"""
    f = case["floor"]
    o = np.asarray(eye, np.float64)
    mids = [f["p0"] + f["half"] * (a * f["u"] + b * f["v"]) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1))]
    look = max(mids, key=lambda p: np.linalg.norm(p - o))
    dist = np.linalg.norm(look - o)
    ang = min(4.0 * abs(height_of(case, eye)) / dist, f["half"] / dist)
    return eye32(look), float(np.degrees(ang))


def far_sphere_view(case, i, boxes, oy, oz):
    """-> (eye, look, vfov): sphere i seen along -x from `boxes` box sizes beyond the box's middle, the eye
    (oy, oz) radii off the sphere's axis, the frame as tall as the sphere's angular radius.  The eye's y and z stay
    small, so the camera's fp32 corner still tells the frame's pixels apart."""
    c = case["d"]["spheres"][i].astype(np.float64)
    eye = eye32((case["mid"][0] + boxes * case["S"], c[1] + oy * c[3], c[2] + oz * c[3]))
    return eye, eye32(c[:3]), float(np.degrees(c[3] / (eye[0] - c[0])))


# frames whose first-light shadow origins leave the box ("touching": spheres 16 .. 31 touch the face +x); found
# with the oracle's own record of its shadow rays, which the GPU test counts again: 336 and 648 pixels outside
FALLBACK_FRAMES = {"512 box sizes": (31, 512.0, 0.25, -0.4), "256 box sizes": (22, 256.0, -0.5, 0.4)}
