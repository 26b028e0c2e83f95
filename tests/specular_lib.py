"""What tests/test_specular_cpu.py and tests/test_specular.py share: probe scenes that make a frame
report pow(dot(N, H), Ns) itself, the oracle's view of such a frame (which pixels are lit, and the
base and the exponent of each), and the distance of a measured power from the exact one.

The probe material is ka = kd = ke = 0, ks = (1, 1, 1).  With one light (nl == 1) scan_row's colour
of a lit pixel is (0 * 0.5 + 0) + (0 * d + 1 * sp) = sp exactly, and black otherwise, so a frame of
the scene is the renderer's power per lit pixel, bit for bit.  A light needs a ke to be a light: its
probe material has ke = (1, 0, 0), so that its own lit pixels are (1 + sp, sp, sp).  The power is read
from the green channel everywhere; blue must equal it, and red must be it or fl(1 + it)."""
import copy
import functools

import numpy as np

import oracle_lib as ol
import random_scenes as rs
import ray_cases as rc
import ray_oracle as ro

F32 = np.float32
NS_VALUES = (0.0, 1.0, 2.0, 16.5, 64.0, 120.0, 1000.0, 1024.0)
PIN_NS = (16.5, 64.0, 120.0)  # one step of x moves x^Ns by >= Ns / 2 >= 8 steps, and x^Ns stays normal
# the order in which faces / spheres take their exponent: 10 of 16 carry a pinning one
PATTERN = (16.5, 0.0, 64.0, 1000.0, 120.0, 1.0, 16.5, 64.0, 2.0, 120.0, 1024.0, 16.5, 64.0, 120.0, 16.5, 64.0)


def probe_material(ns):
    return ol.material13(ks=(1, 1, 1), Ns=ns)


def _light_material(ns):
    return ol.material13(ks=(1, 1, 1), ke=(1, 0, 0), Ns=ns)


def _faces_of(g, sel, material):
    """the faces `sel` of geometry g as a geometry of their own, de-indexed like the loader's"""
    f = g["face_index"][sel].reshape(-1)
    out = {"vertex": g["vertex"][f].copy(), "face_index": np.arange(len(f), dtype=np.uint32).reshape(-1, 3),
           "material": material}
    if len(g["normals"]):
        out["normals"] = g["normals"][f].copy()
    return out


def split_materials(d, mats, offset=0, light=lambda m: _light_material(0.0)):
    """face k (counted through the non-light geometries) and then sphere k take mats[(offset + k) %
    len(mats)]; a geometry is cut into one geometry per material it received.  Lights stay whole, keep
    their order in the light list and take `light` (a function of their material) as their material."""
    geoms, k = [], offset
    for gi, g in enumerate(d["geometry"]):
        if gi in d["light_sources"]:
            geoms.append({**copy.deepcopy(g), "material": np.array(light(g["material"]), F32)})
            continue
        nf = len(g["face_index"])
        which = (k + np.arange(nf)) % len(mats)
        k += nf
        for j in np.unique(which):
            geoms.append(_faces_of(g, np.flatnonzero(which == j), np.array(mats[j], F32)))
    n = len(d["spheres"])
    sm = np.stack([np.array(mats[(k + i) % len(mats)], F32) for i in range(n)]) if n else None
    return ol.scene_dict(geoms, d["spheres"].copy() if n else None, sm)


def probe_split(d, offset=0, pattern=PATTERN):
    """3a: every surface a probe, with the exponents of `pattern` dealt out face by face"""
    return split_materials(d, [probe_material(v) for v in pattern], offset)


def probe_keep_ns(d):
    """3b: the scene's own geometry and exponents, every other material constant the probe's"""
    out = copy.deepcopy(d)
    for gi, g in enumerate(out["geometry"]):
        m = g["material"]
        g["material"] = _light_material(m[12]) if gi in d["light_sources"] else probe_material(m[12])
    for k in range(len(out["sphere_materials"])):
        out["sphere_materials"][k] = probe_material(out["sphere_materials"][k][12])
    return ol.scene_dict(out["geometry"], out["spheres"], out["sphere_materials"])


def oracle_probe_frames(d, eye, look, W, H, **kw):
    """the oracle's frames of a probe scene: {"one", "base", "expo", "lit", "on_light"}.  lit (H, W)
    bool: the pixels whose colour is the power; every other pixel is black in every mode."""
    osc = ol.OracleScene(d)
    return oracle_probe(d, lambda: ol.oracle_render(osc, eye, look, W, H, threads=8, **kw))


def oracle_probe(d, colours):
    """colours() -> the oracle's (..., 3) colours of some rays on probe scene d, under the pow mode that
    is set when it is called"""
    assert len(d["light_sources"]) == 1, "the probe needs nl == 1"
    out = {}
    for name, mode in (("one", ol.POW_ONE), ("base", ol.POW_BASE), ("expo", ol.POW_EXPONENT)):
        with ol.pow_mode(mode):
            out[name] = colours()
    one = out["one"]
    out["lit"] = lit = one[..., 1] == F32(1)
    out["on_light"] = one[..., 0] == F32(2)  # a light's own surface: red carries ke = 1 as well
    assert (one[~lit] == 0).all() and (one[lit][:, 1:] == 1).all() and (out["on_light"] <= lit).all()
    assert ((one[..., 0] == 1) | out["on_light"])[lit].all()
    for name in ("base", "expo"):
        assert (out[name][~lit] == 0).all()
        split_frame(out, out[name])
    return out


def split_frame(frames, img):
    """a probe frame from any renderer -> its powers on the oracle's lit pixels (1-D), after checking
    that every unlit pixel is black (+0), that blue has green's bits and that red has them too, or
    those of fl(1 + green) on a light's own surface"""
    img = np.ascontiguousarray(img, F32).reshape(frames["one"].shape)
    lit = frames["lit"]
    assert not img[~lit].view(np.uint32).any(), "a pixel the oracle leaves black is not +0"
    g = img[..., 1]
    red = np.where(frames["on_light"], (F32(1) + g).astype(F32), g)
    assert (img[..., 2].view(np.uint32) == g.view(np.uint32))[lit].all(), "blue differs from green on a lit pixel"
    assert (img[..., 0].view(np.uint32) == red.view(np.uint32))[lit].all(), "red is not the power (+ ke) on a lit pixel"
    return g[lit]


# ---- exact powers ------------------------------------------------------------------------------------
_STEP_CACHE = {}


def _exact(x, ns):
    import mpmath
    return mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(float(ns)))


def _spacing(e):
    """the fp32 spacing at the exact positive value e, subnormals included"""
    import mpmath
    _, k = mpmath.frexp(e)  # e = m * 2^k, m in [0.5, 1)
    return mpmath.ldexp(mpmath.mpf(1), max(int(k) - 1, -126) - 23)


def round_to_f32(e):
    """nearest fp32 (ties to even) of a positive mpmath value below the overflow threshold"""
    import mpmath
    q = _spacing(e)
    return F32(float(mpmath.nint(e / q) * q))


def steps_from_exact(x, ns, got):
    """per (x, Ns, measured power): |measured - x^Ns| in units of the fp32 spacing at the exact x^Ns
    (mpmath, 120 bits).  Every triple is judged; equal triples are computed once."""
    import mpmath
    x, ns, got = (np.ascontiguousarray(a, F32).ravel() for a in (x, ns, got))
    assert np.isfinite(got).all() and (x > 0).all(), "a power that is not finite, or a base <= 0"
    out = np.zeros(len(x))
    with mpmath.workprec(120):
        for i, key in enumerate(zip(x.view(np.uint32).tolist(), ns.view(np.uint32).tolist(),
                                    got.view(np.uint32).tolist())):
            v = _STEP_CACHE.get(key)
            if v is None:
                e = _exact(x[i], ns[i])
                v = _STEP_CACHE[key] = float(abs(mpmath.mpf(float(got[i])) - e) / _spacing(e))
            out[i] = v
    return out


def report_steps(what, ns, steps):
    """-> {Ns: largest distance}, printed"""
    worst = {float(v): float(steps[ns == F32(v)].max()) for v in np.unique(ns)}
    print(f"{what}: largest distance from the exact power, in fp32 steps, per Ns: " +
          ", ".join(f"{k:g}: {v:.3f}" for k, v in worst.items()))
    return worst


# ---- the scenes of 3a --------------------------------------------------------------------------------
CORNELL_EYE, CORNELL_LOOK = (0, 1, 3), (0, 1, 0)


def probe_case(name):
    """-> (probe scene dict, eye, look, W, H, vfov, oracle / renderer keywords)"""
    import esctp1raytracer_amd as esc
    hashed = {"face_mode": ol.ORC_FACE_HASH, "seed": 7}  # the Cornell light has two faces
    if name == "sphere":  # 2,188 triangles, smooth normals (quirk S1)
        return probe_split(ol.load_dump("CornellBox-Sphere"), 0), CORNELL_EYE, CORNELL_LOOK, 96, 72, 60.0, hashed
    if name == "original":  # flat normals
        return probe_split(ol.load_dump("CornellBox-Original"), 0), CORNELL_EYE, CORNELL_LOOK, 128, 96, 60.0, hashed
    if name == "c3":
        sc = esc.Scene.synthetic("c3", 1000)
        eye, look = esc.synthetic_view()
        return (probe_split(ol.scene_from_product(sc), 0), tuple(float(v) for v in eye),
                tuple(float(v) for v in look), 128, 72, 60.0, {})
    if name == "random":
        d, eye, look, W, H, vfov = rs.random_scene(RANDOM_SEED)
        return probe_split(d, 0), eye, look, W, H, vfov, {}
    raise KeyError(name)


RANDOM_SEED = 31
PROBE_CASES = ("sphere", "original", "c3", "random")
_FRAMES = {}


def probe_case_frames(name):
    """probe_case(name) + the oracle's frames of it, once per process"""
    if name not in _FRAMES:
        d, eye, look, W, H, vfov, kw = probe_case(name)
        _FRAMES[name] = (d, eye, look, W, H, vfov, kw, oracle_probe_frames(d, eye, look, W, H, vfov=vfov, **kw))
    return _FRAMES[name]


def check_probe_inputs(name):
    """what 3a needs from its inputs, from the oracle alone: nl == 1, every Ns on a lit pixel, at least
    half of the lit pixels with a pinning Ns, x in the range rt_shade.h proves.  -> (x, Ns) per lit pixel"""
    d, eye, look, W, H, vfov, kw, fr = probe_case_frames(name)
    assert len(d["light_sources"]) == 1
    lit = fr["lit"]
    x, ns = fr["base"][..., 1][lit], fr["expo"][..., 1][lit]
    for v in NS_VALUES:
        assert (ns == F32(v)).any(), f"Ns = {v} on no lit pixel"
    share = float(np.isin(ns, np.array(PIN_NS, F32)).mean())
    print(f"{name}: {int(lit.sum())} lit pixels of {W}x{H}, {share:.3f} with a pinning Ns")
    assert share >= 0.5
    assert x.min() >= F32(0.49) and x.max() <= F32(1.001)
    return x, ns


# ---- section 4: materials at the edges of the skip ------------------------------------------------------
def edge_materials():
    """ks in {+0, -0, mixed zeros} x Ns at and beyond the edges of [0, 1024], with kd = +0 / -0 /
    ordinary so that kd * d + ks * sp is sometimes a zero whose sign the product decides"""
    nz = F32(-0.0)
    kss = [(0.0, 0.0, 0.0), (nz, nz, nz), (nz, 0.0, nz)]
    nss = [0.0, nz, 1.0, 1024.0, np.nextafter(F32(1024), F32(np.inf)), -1.0, 1e30, -1e30, np.inf, -np.inf,
           np.nan, 1e-45]
    kds = [(0.0, 0.0, 0.0), (nz, nz, nz), (0.5, 0.4, 0.3), (0.7, nz, 0.0)]
    kas = [(0.0, 0.0, 0.0), (0.2, 0.3, 0.4), (nz, nz, nz)]
    mats = []
    for i, ks in enumerate(kss):
        for j, ns in enumerate(nss):
            k = i * len(nss) + j
            mats.append(ol.material13(ka=kas[k % 3], kd=kds[(k + i) % 4], ks=ks, Ns=ns))
    return mats


def flagged_materials():
    """rows of edge_materials() that material_spec_free flags (ks = +-0, Ns = 1024 / 1 / 0), with an
    ordinary kd: on a normal about 1.2 long the power overflows and +-0 * inf is a NaN that `sp = 1`
    would not give"""
    mats = edge_materials()
    out = [mats[i].copy() for i in (3, 12 + 3, 2, 24 + 3, 0)]
    for m in out:
        m[3:6] = (0.5, 0.4, 0.3)
        assert (m[6:9] == 0).all() and 0 <= m[12] <= 1024
    return out


MIRROR = ol.material13(ka=(0.1, 0.1, 0.1), kd=(0.2, 0.2, 0.2), ks=(0.6, 0.5, 0.4), Ns=0.0)  # pow(x, 0) == 1


def odd_normal_patches(y, x0, z0, size, mats):
    """horizontal squares at height y facing up, one per per-vertex-normal recipe, whose interpolated
    normal main.cpp:733-738 normalises into something that is NOT a unit vector (or is one only by
    luck): squares of subnormal size lose most of their bits in dot(n, n), so n / sqrt(dot) comes out
    about 0.8 or 1.2 long; 2e19 overflows the dot (N = 0); opposite normals cancel along the face; and
    two collapsed triangles (NaN face normal, never hit) travel along.  -> list of geometries"""
    out = []
    recipes = [("scaled", 3e-23), ("scaled", 4.5e-23), ("scaled", 1e-19), ("scaled", 1e19), ("scaled", 2e19),
               ("cancel", 1.0), ("cancel", 4.5e-23), ("collapsed", 0.0)]
    for k, (kind, s) in enumerate(recipes):
        xa, xb = x0 + k * size * 1.1, x0 + k * size * 1.1 + size
        quad = [(xa, y, z0 + size), (xb, y, z0 + size), (xb, y, z0), (xa, y, z0)]
        v = np.array([quad[i] for i in (0, 1, 2, 0, 2, 3)], F32)
        n = np.tile(np.array([0.0, s, 0.0], F32), (6, 1))
        if kind == "cancel":  # n0 up, n2 down: n2 * v + n0 * (1 - v) passes through zero at v = 1/2
            n[2] = n[5] = (0.3 * s, -s, 0.0)
        if kind == "collapsed":
            v[1] = v[0]       # two equal corners
            v[3:] = v[3]      # a point
            n[:] = (0.0, 1.0, 0.0)
        out.append({"vertex": v, "face_index": np.arange(6, dtype=np.uint32).reshape(2, 3), "normals": n,
                    "material": np.array(mats[k % len(mats)], F32)})
    return out


def edge_scene(name):
    """-> (scene dict, eye, look, W, H, vfov): one light, every surface a row of edge_materials()"""
    mats = edge_materials()
    if name == "cornell":
        d = ol.load_dump("CornellBox-Original")
        eye, look, W, H, vfov = (0, 1, 3.2), (0, 0.9, 0), 128, 96, 60.0
        out = split_materials(d, mats, light=lambda m: m)
        # and one surface that reflects (Ns = 0: its own power is exactly 1), lying on the floor, so that
        # `trace` carries the NaN colours of the walls and the ceiling through a weight
        mirror = {"vertex": np.array([(-0.95, 0.015, 0.68), (0.95, 0.015, 0.68), (0.95, 0.015, 0.42),
                                      (-0.95, 0.015, 0.68), (0.95, 0.015, 0.42), (-0.95, 0.015, 0.42)], F32),
                  "face_index": np.arange(6, dtype=np.uint32).reshape(2, 3), "material": MIRROR.copy()}
        geoms = out["geometry"] + odd_normal_patches(0.02, -0.9, 0.7, 0.2, flagged_materials()) + [mirror]
        out = ol.scene_dict(geoms)
    else:
        import esctp1raytracer_amd as esc
        sc = esc.Scene.synthetic("c3", 400)
        eye, look = (tuple(float(v) for v in a) for a in esc.synthetic_view())
        W, H, vfov = 128, 72, 60.0
        out = split_materials(ol.scene_from_product(sc), mats, light=lambda m: m)
    assert len(out["light_sources"]) == 1
    return out, eye, look, W, H, vfov


_EDGE_RAYS = {}


def edge_trace_rays():
    """-> (the cornell edge scene, origins, targets): rays of a 16 x 12 frame and rays aimed at the mirror strip
    for which the hand-built camera of ray_oracle.py reproduces every bounce direction (chosen by the oracle)"""
    if not _EDGE_RAYS:
        d, eye, look, _, _, _ = edge_scene("cornell")
        o, a = rc.camera_targets(eye, look, 16, 12)
        rng = np.random.default_rng(4)  # and 160 rays from around the eye to points on the mirror strip
        strip = np.stack([rng.uniform(-0.9, 0.9, 160), np.full(160, 0.015), rng.uniform(0.44, 0.66, 160)], 1)
        o = np.concatenate([o, np.array(eye, F32) + rng.uniform(-0.3, 0.3, (160, 3))]).astype(F32)
        a = np.concatenate([a, strip]).astype(F32)
        keep = ro.oracle_trace(d, o, a, 2, float(F32(1e-4)))["usable"]
        _EDGE_RAYS["v"] = (d, o[keep], a[keep])
    return _EDGE_RAYS["v"]


def odd_patch_scene():
    """the Cornell light over nothing but the odd patches, all with flagged materials (ks = +-0, Ns in
    [0, 1024]): the scene on which skipping the power without looking at |N| changes the frame"""
    d = ol.load_dump("CornellBox-Original")
    light = [copy.deepcopy(d["geometry"][gi]) for gi in d["light_sources"]]
    out = ol.scene_dict(odd_normal_patches(0.02, -0.9, 0.7, 0.2, flagged_materials()) + light)
    assert len(out["light_sources"]) == 1
    return out, (0, 1.5, 1.5), (0, 0, 0.8), 160, 40, 20.0


# ---- 3b: a table of measured powers --------------------------------------------------------------------
def table_from_probe(d, eye, look, W, H, render_probe, **kw):
    """render_probe(probe scene) -> its frame from the renderer under test.  -> (keys, values) of the
    (x, Ns) -> power table of every lit pixel of d's own rays, x and Ns from the oracle"""
    probe = probe_keep_ns(d)
    fr = oracle_probe_frames(probe, eye, look, W, H, **kw)
    powers = split_frame(fr, render_probe(probe))
    lit = fr["lit"]
    return ol.pow_table(fr["base"][..., 1][lit], fr["expo"][..., 1][lit], powers)


def oracle_with_table(d, eye, look, W, H, table, **kw):
    """-> (the oracle's frame of d with the table's powers, table misses)"""
    with ol.pow_mode(ol.POW_TABLE, table=table):
        ref = ol.oracle_render(d, eye, look, W, H, threads=8, **kw)
        return ref, ol.pow_misses()


# ---- 3b: traced rays, a table gathered level by level ---------------------------------------------------
# ray_oracle.ray_colours with `horizontal` = 0: every power the oracle takes inside is one of the ray that
# is compared, so that the table's miss counter speaks of those rays alone
ray_colours = functools.partial(ro.ray_colours, horizontal=(0, 0, 0))


def recorded_levels():
    """-> (calls, colours): with oracle_trace(..., colours=colours) each level's colours come from
    ray_colours, and every such call is recorded in `calls` as (origins, targets, fixed_face, shadows, dirs)"""
    calls = []

    def colours(d, origins, llc, fixed_face=0, shadows=True):
        dirs, rgb = ray_colours(d, origins, llc, fixed_face, shadows)
        calls.append((origins.copy(), llc.copy(), fixed_face, shadows, dirs.copy()))
        return dirs, rgb
    return calls, colours


def table_from_levels(d, levels, shade_probe):
    """levels: the calls recorded_levels() gathered while the restatement traced d (the rays of a level do not
    depend on any power).  shade_probe(probe scene, origins, targets, dirs, fixed_face, shadows) -> (n, 3) colours
    from the renderer under test.  -> (keys, values) over every lit ray of every level"""
    probe = probe_keep_ns(d)
    x, ns, powers = [], [], []
    for origins, llc, fixed_face, shadows, dirs in levels:
        fr = oracle_probe(probe, lambda: ray_colours(probe, origins, llc, fixed_face, shadows)[1])
        powers.append(split_frame(fr, shade_probe(probe, origins, llc, dirs, fixed_face, shadows)))
        x.append(fr["base"][..., 1][fr["lit"]])
        ns.append(fr["expo"][..., 1][fr["lit"]])
    return ol.pow_table(np.concatenate(x), np.concatenate(ns), np.concatenate(powers))


def trace_ns_case(name):
    """the `_ns` cases of ray_cases.py, all three with one light (CornellBox-Original; random_scene
    3 and 9: 1 + (seed % 7 == 0) + (seed % 11 == 0) lights)"""
    d, o, a = rc.trace_case_rays(name)
    assert name.endswith("_ns") and len(d["light_sources"]) == 1
    return d, o, a


REFRACTION_SETTING = (3, float(F32(1e-4)), True)  # TRANSMISSION_SETTINGS' first: depth, bias, shadows
_REFRACTION = {}


def refraction_ns_case(name="slab"):
    """a transmission case's scene and camera, but specular all over: the case's walls have ks = 0
    (no power reaches a colour there), so every surface that is not a light gets ks in [0.2, 0.6] unless
    it has one, and a random Ns in [1, 60]; the light keeps its loaded Ns.  The rays are then chosen as
    ray_cases.py chooses its own: those whose every bounce direction the hand-built camera reproduces, in
    both modes.  -> (scene, origins, targets)"""
    if name not in _REFRACTION:
        d, o, a = rc.transmission_case(name)
        loaded = ol.load_dump("CornellBox-Original")
        rng = np.random.default_rng(6)
        for gi, g in enumerate(d["geometry"]):
            m = g["material"]
            if gi in d["light_sources"]:
                m[12] = loaded["geometry"][gi]["material"][12]
                continue
            if not m[6:9].any():
                m[6:9] = rng.uniform(0.2, 0.6, 3)
            m[12] = rng.uniform(1.0, 60.0)
        assert len(d["light_sources"]) == 1 and all(g["material"][12] != 0 for g in d["geometry"])
        depth, bias, shadows = REFRACTION_SETTING
        keep = np.ones(len(o), bool)
        for mode in (ro.REFRACT, ro.FRESNEL):
            keep &= ro.oracle_trace(d, o, a, depth, bias, mode, shadows=shadows)["usable"]
        _REFRACTION[name] = (d, o[keep], a[keep])
    return _REFRACTION[name]


# ---- 3c: several lights ---------------------------------------------------------------------------------
def with_specular(d, seed):
    """ks in [0.2, 0.9] and Ns in [1, 120] on every material that is not a light's (kd stays: both
    addends of kd * d + ks * sp are non-zero)"""
    rng = np.random.default_rng(seed)
    d = copy.deepcopy(d)
    mats = [g["material"] for gi, g in enumerate(d["geometry"]) if gi not in d["light_sources"]]
    mats += list(d["sphere_materials"])
    for m in mats:
        m[6:9] = rng.uniform(0.2, 0.9, 3)
        m[12] = rng.uniform(1.0, 120.0)
    return d


def bracket_scenes():
    """`two` (2 lights) and the 3-light scene of test_both_shading_forms_on_small_frames"""
    rng = np.random.default_rng(17)
    base = ol.load_dump("two")
    sph = np.concatenate([rng.uniform(-1.5, 1.5, (300, 1)), rng.uniform(0.1, 1.8, (300, 1)),
                          rng.uniform(-1.5, 1.0, (300, 1)), rng.uniform(0.03, 0.2, (300, 1))], 1)
    mats = np.stack([ol.material13(ka=c, kd=c) for c in rng.uniform(0.2, 0.9, (300, 3))])
    third = {"vertex": np.array([[-1.8, 1.6, 1.2], [-1.8, 1.9, 1.2], [-1.5, 1.6, 1.0]], F32),
             "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_B}
    two = with_specular(ol.load_dump("two"), 1)
    three = with_specular(ol.scene_dict([dict(g) for g in base["geometry"] + [third]], sph.astype(F32), mats), 2)
    assert len(two["light_sources"]) == 2 and len(three["light_sources"]) == 3
    return {"two": (two, (0, 1, 3), (0, 1, 0), 160, 90), "three": (three, (0, 1, 3), (0, 1, 0), 97, 61)}


def steps_between(lo, hi):
    """fp32 values from lo to hi (same sign or zero), counted on the integer line of their bits"""
    def line(a):
        b = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
        return np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return line(hi) - line(lo)
