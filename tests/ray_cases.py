"""Scenes and rays of the ray tests, chosen on the CPU by the restatement of tests/ray_oracle.py alone,
before anything runs on the GPU.

The bounce cases (trace_case_rays, transmission_case_rays) keep only rays for which the hand-built camera
reproduces every bounce direction at every setting (ray_oracle.py's docstring), and every test asserts
that all the rays it submits are compared.

powf: the device's and the host libm's differ in the last bit, which shade against orc_render shows at
level 0 already (16 of 576 values on cornell_mixed, relative difference up to 1.6e-7).  The trace cases
therefore come in two kinds, as tests/test_gpu_parity.py treats specular pixels: with Ns = 0 on the edited
materials (pow(x, 0) is 1 on both sides) every bit is compared; the `_ns` cases keep the materials' own and
random Ns.  Every material of the transmission cases has Ns = 0."""
import numpy as np

import oracle_lib as ol
import random_scenes as rs
from ray_oracle import F32, FRESNEL, REFRACT, normalize, oracle_trace

CORNELL_EYE, CORNELL_LOOK = (0, 1, 3.5), (0, 1, 0)


# ---- rays ---------------------------------------------------------------------------------------------
def camera_targets(eye, look, W, H):
    """origins and lower-left-corner style targets of a W x H frame's rays (any point on the ray)"""
    import esctp1raytracer_amd as esc
    cam = esc.Camera.for_image(eye, look, W, H).c
    o = np.tile(np.array(list(cam.origin), F32), (W * H, 1))
    llc, hz, vt = (np.array(list(v), F32) for v in (cam.lower_left_corner, cam.horizontal, cam.vertical))
    t = []
    for h in range(H):
        for w_ in range(W):
            s, tt = F32(w_) / F32(W - 1), F32(h) / F32(H - 1)
            t.append(((llc + (hz * s).astype(F32)).astype(F32) + (vt * tt).astype(F32)).astype(F32))
    return o, np.array(t, F32)


def box(d):
    pts = [g["vertex"] for g in d["geometry"] if len(g["vertex"])]
    if len(d["spheres"]):
        s = d["spheres"]
        pts += [s[:, :3] - s[:, 3:], s[:, :3] + s[:, 3:]]
    p = np.concatenate(pts)
    return p.min(0), p.max(0)


def surface_points(d, n, rng):
    """points on triangles (barycentric) and on spheres"""
    tris = [g["vertex"][g["face_index"]] for g in d["geometry"] if len(g["face_index"])]
    T = np.concatenate(tris) if tris else np.zeros((0, 3, 3), F32)
    pts = []
    if len(T):
        k = rng.integers(0, len(T), n)
        a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        pts.append(T[k, 0] + a[:, None] * (T[k, 1] - T[k, 0]) + b[:, None] * (T[k, 2] - T[k, 0]))
    if len(d["spheres"]):
        s = d["spheres"][rng.integers(0, len(d["spheres"]), n)]
        pts.append(s[:, :3] + normalize(rng.standard_normal((n, 3))) * s[:, 3:])
    p = np.concatenate(pts)
    return p[rng.integers(0, len(p), n)].astype(F32)


def ray_sets(d, rng, n):
    """-> {name: (origins, targets)}"""
    lo, hi = box(d)
    ext = F32(max(1e-3, float(np.max(hi - lo))))
    inside = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F32)
    surf = surface_points(d, n, rng)
    sets = {
        # orthographic bundle: one direction, origins on a plane in front of the scene
        "ortho": ((lo + rng.uniform(0, 1, (n, 3)) * (hi - lo) + np.array([0, 0, 2]) * ext).astype(F32),
                  None),
        "from_surfaces": (surf, (surf + rng.standard_normal((n, 3)) * ext).astype(F32)),
        "inside": (inside, surface_points(d, n, rng)),
        "far": ((lo + hi) / 2 + normalize(rng.standard_normal((n, 3))) * ext * F32(3e3), surface_points(d, n, rng)),
        # grazing: towards a surface point from a point nudged off it along the surface
        "grazing": ((surf + rng.standard_normal((n, 3)) * ext * F32(1e-3)).astype(F32), surface_points(d, n, rng)),
    }
    out = {}
    for k, (o, a) in sets.items():
        if a is None:
            a = (o - np.array([0.02, 0.01, 1.0], F32) * ext).astype(F32)
        out[k] = (np.ascontiguousarray(o, F32), np.ascontiguousarray(a, F32))
    return out


# ---- mirror bounces -----------------------------------------------------------------------------------
def with_ks(d, seed, share=0.6, ns_zero=True):
    """a share of the materials gets ks > 0, one a zero channel, one NaN, one negative; Ns = 0 or random
    (the module docstring says why)"""
    rng = np.random.default_rng(seed)
    mats = [g["material"] for g in d["geometry"]] + list(d["sphere_materials"])
    pick = [m for m in mats if rng.uniform() < share]
    for j, m in enumerate(pick):
        m[6:9] = rng.uniform(0.3, 0.95, 3)
        m[12] = 0.0 if ns_zero else rng.uniform(1.0, 60.0)
        if j % 7 == 3:
            m[6 + j % 3] = 0.0
        if j % 23 == 11:
            m[6:9] = np.nan
        if j % 23 == 17:
            m[7] = -0.5
    return d


def trace_case(name):
    """-> (scene dict, origins, targets) before the choice of trace_case_rays"""
    ns_zero = not name.endswith("_ns")
    name = name[:-3] if name.endswith("_ns") else name
    rng = np.random.default_rng(11)
    if name in ("mirror_camera", "mirror_floor_camera"):
        d = ol.load_dump("CornellBox-Mirror")
        if name == "mirror_floor_camera":  # the floor reflects too, so that paths go past level 1
            d["geometry"][0]["material"][6:9] = (0.5, 0.4, 0.0)
            d["geometry"][0]["material"][12] = 0.0  # see with_ks
        V = d["geometry"][5]["vertex"]
        c = (V.min(0) + V.max(0)) / 2
        o, a = camera_targets(tuple(float(x) for x in c + np.array([0.5, 0.3, 1.6])), tuple(float(x) for x in c),
                              16, 12)
        return d, o, a
    if name == "mirror_block":
        d = ol.load_dump("CornellBox-Mirror")
        G = d["geometry"][5]  # ks = 0.95, Ns = 1000: the tall block
        T = G["vertex"][G["face_index"]]
        k = rng.integers(0, len(T), 160)
        a, b = rng.uniform(0.05, 0.45, 160), rng.uniform(0.05, 0.45, 160)
        pts = (T[k, 0] + a[:, None] * (T[k, 1] - T[k, 0]) + b[:, None] * (T[k, 2] - T[k, 0])).astype(F32)
        o = (np.array([0, 1, 0.9], F32) + rng.uniform(-0.6, 0.6, (160, 3))).astype(F32)
        return d, o, pts
    if name == "cornell_mixed":
        d = with_ks(ol.load_dump("CornellBox-Original"), 5, share=0.8, ns_zero=ns_zero)
        o, a = camera_targets(CORNELL_EYE, CORNELL_LOOK, 16, 12)
        return d, o, a
    seed = int(name[4:])
    d, eye, look, _, _, _ = rs.random_scene(seed)
    d = with_ks(d, seed, ns_zero=ns_zero)
    o, a = ray_sets(d, rng, 64)["inside"]
    o2, a2 = camera_targets(eye, look, 12, 8)
    return d, np.concatenate([o, o2]), np.concatenate([a, a2])


# the unedited Mirror scene has one reflecting (convex) block: its paths end at level 1
TRACE_SETTINGS = [(1, 0.0, True), (2, 1e-4, True), (5, 0.5, False), (2, 0.0, False), (5, 1e-4, True)]
TRACE_CASES = [("mirror_camera", 1, 0.0, True), ("mirror_camera", 1, 1e-4, False), ("mirror_block", 1, 0.0, True),
               ("mirror_block", 1, 0.5, False)] + \
              [(n, *s) for n in ("mirror_floor_camera", "cornell_mixed", "rand3", "rand5", "rand9")
               for s in TRACE_SETTINGS] + \
              [(n, *s) for n in ("cornell_mixed_ns", "rand3_ns", "rand9_ns") for s in TRACE_SETTINGS[1::3]]
_TRACE_CACHE = {}


def trace_case_rays(name):
    """-> (scene dict, origins, targets): chosen on the CPU so that the oracle itself bounces, and so that
    the hand-built camera reproduces every bounce direction down to level 5"""
    if name not in _TRACE_CACHE:
        d, o, a = trace_case(name)
        keep = np.ones(len(o), bool)
        for bias, shadows in {(b, s_) for _, b, s_ in TRACE_SETTINGS}:
            keep &= oracle_trace(d, o, a, 5, float(F32(bias)), shadows=shadows)["usable"]
        _TRACE_CACHE[name] = (d, o[keep], a[keep])
    return _TRACE_CACHE[name]


# ---- refraction ---------------------------------------------------------------------------------------
def product(d):
    sc = ol.scene_to_product(d)
    for g, t in d.get("transmission", {}).items():
        sc.set_transmission(g, t[:3], t[3])
    for p, t in d.get("sphere_transmission", {}).items():
        sc.set_sphere_transmission(p, [t[:3]], [t[3]])
    return sc


def cornell():
    d = ol.load_dump("CornellBox-Original")
    d["geometry"][0]["material"][6:9] = (0.5, 0.4, 0.3)  # the floor mirrors, so that paths go on after the glass
    d["geometry"][0]["material"][12] = 0.0
    d["transmission"], d["sphere_transmission"] = {}, {}
    return d


def glass(ks=(0.5, 0.5, 0.5)):
    return ol.material13(ka=(0, 0, 0), kd=(0.1, 0.1, 0.1), ks=ks, Ns=0.0)  # its ks must drive no bounce


def add_box(d, lo, hi, tr):
    """a closed box of 12 triangles, normals outwards"""
    lo, hi = np.array(lo, F32), np.array(hi, F32)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], F32)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    d["geometry"].append({"vertex": v, "normals": np.zeros((0, 3), F32), "face_index": np.array(f, np.uint32),
                          "material": glass()})
    d["transmission"][len(d["geometry"]) - 1] = np.array(tr, F32)


def add_sheet(d, y, tr, seed, n=3, amp=0.03):
    """an open, gently uneven sheet across the box at height ~y (n x n quads), normals upwards"""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-0.99, 0.99, n + 1)
    zs = np.linspace(-0.99, 0.99, n + 1)
    v = np.array([[x, y + rng.uniform(-amp, amp), z] for z in zs for x in xs], F32)
    f = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            f += [(a, a + n + 1, a + 1), (a + 1, a + n + 1, a + n + 2)]
    d["geometry"].append({"vertex": v, "normals": np.zeros((0, 3), F32), "face_index": np.array(f, np.uint32),
                          "material": glass(ks=(0, 0, 0))})
    d["transmission"][len(d["geometry"]) - 1] = np.array(tr, F32)


def transmission_case(name):
    """-> (scene dict, origins, targets) before the choice of transmission_case_rays"""
    d = cornell()
    if name == "sphere":  # an analytic glass sphere; tf has a zero channel
        d["spheres"] = np.array([[0.35, 1.05, 0.4, 0.35]], F32)  # above the short block
        d["sphere_materials"] = glass()[None].copy()
        d["sphere_transmission"][0] = np.array([0.9, 0.7, 0.0, 1.5], F32)
        o, a = camera_targets((0.1, 1.3, 2.2), (0.35, 1.05, 0.4), 16, 12)
    elif name == "slab":  # a closed glass box: what enters by one face meets its neighbour beyond the critical angle
        add_box(d, (-0.6, 1.3, -0.4), (0.5, 1.7, 0.5), (0.8, 0.9, 0.7, 1.5))  # above both blocks
        o, a = camera_targets((0.9, 1.9, 2.4), (-0.05, 1.5, 0.05), 16, 12)
    elif name == "sheet_above":  # water, ni < 1 (reflects internally from above) and ni = 1 (straight through)
        add_sheet(d, 1.2, (0.9, 0.8, 0.7, 0.75), 1)
        add_sheet(d, 0.8, (0.6, 0.9, 0.0, 1.33), 2)
        add_sheet(d, 0.4, (0.9, 0.9, 0.9, 1.0), 3)
        o, a = camera_targets((0.2, 1.85, 0.9), (-0.1, 0.0, -0.3), 16, 12)
    elif name == "sheet_below":  # seen from under the water: beyond 48.8 degrees the surface is a mirror
        add_sheet(d, 1.0, (0.6, 0.9, 0.8, 1.33), 2)
        o, a = camera_targets((0.85, 0.3, 0.9), (-0.3, 1.0, -0.4), 16, 12)
    else:
        raise KeyError(name)
    for m in [g["material"] for g in d["geometry"]] + list(d["sphere_materials"]):
        m[12] = 0.0  # Ns (module docstring)
    return d, o, a


DEPTH = 5
TRANSMISSION_SETTINGS = [(3, 1e-4, True), (DEPTH, 1e-3, False), (DEPTH, 0.0, True)]
TIR_CASES = ("slab", "sheet_above", "sheet_below")
TRANSMISSION_CASES = [(n, *s) for n in ("sphere", "slab", "sheet_above", "sheet_below") for s in TRANSMISSION_SETTINGS]
_TRANSMISSION_CACHE = {}


def transmission_case_rays(name):
    """-> (scene, origins, targets) with the rays for which the hand-built camera reproduces every bounce
    direction at every setting and in both modes: chosen by the restatement alone"""
    if name not in _TRANSMISSION_CACHE:
        d, o, a = transmission_case(name)
        keep = np.ones(len(o), bool)
        for bias, shadows in {(b, s_) for _, b, s_ in TRANSMISSION_SETTINGS}:
            for mode in (REFRACT, FRESNEL):
                keep &= oracle_trace(d, o, a, DEPTH, float(F32(bias)), mode, shadows=shadows)["usable"]
        _TRANSMISSION_CACHE[name] = (d, o[keep], a[keep])
    return _TRANSMISSION_CACHE[name]
