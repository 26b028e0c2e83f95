"""Refraction on the GPU (esc_trace_rays_ex / esc_render_traced_ex, rt_trace.hip + rt_transmit.h), bit for
bit against a CPU restatement built the way tests/test_trace_rays.py builds its own: the index-order
closest hit pinned in test_ray_queries.py, orc_cross / orc_normalize for the normal, each level's colour
from orc_render through a hand-built camera, and the bounce rule of include/esctp1_rt.h (at
esc_trace_options) in numpy fp32, one rounding per operation, with the hash in numpy uint64.

The scenes and rays are chosen on the CPU before anything runs on the GPU (case_rays): only rays for
which the hand-built camera reproduces every bounce direction are kept, every case asserts that all the
rays it submits are compared, and that the restatement itself refracts, reflects internally and (in
FRESNEL mode) takes both branches, on paths at least three levels deep.  Every material of these
scenes has Ns = 0, so that powf's last bit (test_trace_rays.py's docstring) plays no part.

esc_transmit_stats counts the rays a branch sent on to the next level; the restatement counts the same
way, so the three counters plus the mirror bounces add up to depth_rays of the following level."""
import numpy as np
import pytest

import oracle_lib as ol
from test_trace_rays import (CORNELL_EYE, CORNELL_LOOK, F32, _dot, _normalize, assert_same, camera_targets,
                             closest_hits, normals_and_ks, oracle_colours, same_bits)

OFF, REFRACT, FRESNEL = 0, 1, 2
MODE_NAME = {OFF: "off", REFRACT: "refract", FRESNEL: "fresnel"}
SEED, PIXEL_BASE = 77, 1234
U64 = np.uint64


# ---- the rule of include/esctp1_rt.h in numpy ---------------------------------------------------------
def mix_hi32(seed, pixel, light=0xFFFFFFFF):
    """the light-face hash's 64-bit mixer (splitmix64's finaliser), high 32 bits, before the modulo"""
    with np.errstate(over="ignore"):
        z = U64(seed % (1 << 64)) + ((pixel.astype(U64) << U64(32)) | U64(light)) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return (z >> U64(32)).astype(np.uint32)


def test_mixer_restatement_is_splitmix64():
    """pure python integers against the numpy form (no GPU): the finaliser of splitmix64"""
    M = (1 << 64) - 1
    for seed, pixel in ((0, 0), (77, 1234), (2 ** 64 - 1, 2 ** 32 - 1), (5 + 64 * 3, 99)):
        z = (seed + ((pixel << 32) | 0xFFFFFFFF) + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        assert int(mix_hi32(seed, np.array([pixel], np.uint32))[0]) == z >> 32


def bounce(o, dr, t0, N, ks, tr, w, mode, seed_k, q, bias, swap_bias=False):
    """one bounce of every ray -> (go, o', x, w', what) with d' = normalize(x); what: 0 mirror (or the path
    ends), 1 refracted, 2 fresnel_reflected, 3 total_internal.  swap_bias puts the origins of a
    transmissive hit on the wrong sides (the bias case shows that this changes the result)."""
    one, two = F32(1), F32(2)
    bias = F32(bias)
    tf, ni = tr[:, :3], tr[:, 3]
    glass = (mode != OFF) & ((tf[:, 0] > 0) | (tf[:, 1] > 0) | (tf[:, 2] > 0)) & (ni > 0)
    s = _dot(dr, N)
    pos = s > 0
    Nf = np.where(pos[:, None], -N, N).astype(F32)
    c1 = np.where(pos, s, -s).astype(F32)
    eta = np.where(pos, ni, one / ni).astype(F32)
    k = (one - ((eta * eta).astype(F32) * (one - (c1 * c1).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    tir = glass & ~(k >= 0)
    sq = np.sqrt(k).astype(F32)
    fres = np.zeros(len(o), bool)
    if mode == FRESNEL:
        r0 = ((ni - one).astype(F32) / (ni + one).astype(F32)).astype(F32)
        r0 = (r0 * r0).astype(F32)
        cx = np.where(pos, sq, c1).astype(F32)
        m = (one - cx).astype(F32)
        m2 = (m * m).astype(F32)
        Fr = (r0 + ((one - r0).astype(F32) * ((m2 * m2).astype(F32) * m).astype(F32)).astype(F32)).astype(F32)
        u = ((mix_hi32(seed_k, q) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
        fres = glass & ~tir & (u < Fr)
    reflect = tir | fres
    refr = glass & ~reflect
    P = (o + (dr * t0[:, None]).astype(F32)).astype(F32)
    nb = (Nf * bias).astype(F32)
    near, far = (P + nb).astype(F32), (P - nb).astype(F32)
    if swap_bias:
        o2 = np.where(glass[:, None], np.where(refr[:, None], near, far), near)
    else:
        o2 = np.where(refr[:, None], far, near)
    xr = (dr - (N * (two * s).astype(F32)[:, None]).astype(F32)).astype(F32)
    xt = ((dr * eta[:, None]).astype(F32) + (Nf * ((eta * c1).astype(F32) - sq).astype(F32)[:, None]).astype(F32))
    x = np.where(refr[:, None], xt.astype(F32), xr)
    w2 = np.where(glass[:, None], np.where(reflect[:, None], w, (w * tf).astype(F32)), (w * ks).astype(F32))
    go = (glass & reflect) | (w2[:, 0] > 0) | (w2[:, 1] > 0) | (w2[:, 2] > 0)
    what = np.where(refr & go, 1, np.where(fres, 2, np.where(tir, 3, 0)))
    return go, o2.astype(F32), x.astype(F32), w2.astype(F32), what


def transmission_rows(d, hit):
    """the side table's entry (tf, ni) of every ray's hit; (0, 0, 0, 1) where there is none"""
    tr = np.tile(np.array([0, 0, 0, 1], F32), (len(hit["geom"]), 1))
    for i, (g, p) in enumerate(zip(hit["geom"], hit["prim"])):
        if g >= 0:
            tr[i] = d.get("transmission", {}).get(int(g), tr[i])
        elif p >= 0:
            tr[i] = d.get("sphere_transmission", {}).get(int(p), tr[i])
    return tr


def oracle_trace(d, o, targets, max_depth, bias, mode, shadows=True, swap_bias=False, colours=True):
    """-> {"dirs", "rgb", "usable", "depth_rays", "refracted", "fresnel_reflected", "total_internal"}"""
    n = o.shape[0]
    dirs0, c = oracle_colours(d, o, targets, 0, shadows)
    Cc = c.copy()
    usable = np.ones(n, bool)
    counts = [n] + [0] * 16
    ev = [0, 0, 0, 0]
    idx = np.arange(n)
    co, cd, w = o.copy(), dirs0.copy(), np.ones((n, 3), F32)
    with np.errstate(all="ignore"):
        for k in range(max_depth):
            if len(idx) == 0:
                break
            hit = closest_hits(d, co, cd)
            N, ks, has = normals_and_ks(d, hit, co, cd)
            q = ((PIXEL_BASE + idx) % (1 << 32)).astype(np.uint32)
            go, o2, x, w, what = bounce(co, cd, hit["t"], N, ks, transmission_rows(d, hit), w, mode, SEED + 64 * k,
                                        q, bias, swap_bias)
            go &= has
            for j in (1, 2, 3):
                ev[j] += int(((what == j) & go).sum())
            d2 = _normalize(x)
            idx, co, cd, w, x = idx[go], o2[go], d2[go], w[go], x[go]
            counts[k + 1] = len(idx)
            if len(idx) == 0:
                break
            if colours:
                got_d, c = oracle_colours(d, co, (x * F32(2.0 ** 40)).astype(F32), 0, shadows)
                usable[idx[~same_bits(got_d, cd).all(axis=1)]] = False
                Cc[idx] = (Cc[idx] + (w * c).astype(F32)).astype(F32)
    return {"dirs": dirs0, "rgb": Cc, "usable": usable, "depth_rays": counts, "refracted": ev[1],
            "fresnel_reflected": ev[2], "total_internal": ev[3]}


# ---- scenes -------------------------------------------------------------------------------------------
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


def _case(name):
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
SETTINGS = [(3, 1e-4, True), (DEPTH, 1e-3, False), (DEPTH, 0.0, True)]
_CASE_CACHE = {}


def case_rays(name):
    """-> (scene, origins, targets) with the rays for which the hand-built camera reproduces every bounce
    direction at every setting and in both modes: chosen by the restatement alone"""
    if name not in _CASE_CACHE:
        d, o, a = _case(name)
        keep = np.ones(len(o), bool)
        for bias, shadows in {(b, s_) for _, b, s_ in SETTINGS}:
            for mode in (REFRACT, FRESNEL):
                keep &= oracle_trace(d, o, a, DEPTH, float(F32(bias)), mode, shadows)["usable"]
        _CASE_CACHE[name] = (d, o[keep], a[keep])
    return _CASE_CACHE[name]


TIR_CASES = ("slab", "sheet_above", "sheet_below")
CASES = [(n, *s) for n in ("sphere", "slab", "sheet_above", "sheet_below") for s in SETTINGS]


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def stats_of(want):
    return {k: want[k] for k in ("refracted", "fresnel_reflected", "total_internal")}


# ---- 1. the restatement --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,max_depth,bias,shadows", CASES)
def test_refraction_against_the_restatement(esc, r, name, max_depth, bias, shadows):
    d, o, a = case_rays(name)
    bias = float(F32(bias))
    assert len(o) >= 64, len(o)
    r.upload(product(d))
    for mode in (REFRACT, FRESNEL):
        want = oracle_trace(d, o, a, max_depth, bias, mode, shadows)
        print(name, MODE_NAME[mode], len(o), want["depth_rays"][:max_depth + 1], stats_of(want))
        # the restatement alone must do what the comparison is about
        assert want["usable"].all(), np.flatnonzero(~want["usable"]).tolist()  # every ray is compared
        assert want["refracted"] > 0 and want["depth_rays"][2] > 0, (want["depth_rays"], stats_of(want))
        if name in TIR_CASES:
            assert want["total_internal"] > 0, stats_of(want)
        if mode == FRESNEL:
            assert want["fresnel_reflected"] > 0, stats_of(want)
        else:
            assert want["fresnel_reflected"] == 0
        for exact in (False, True):
            got = r.trace(o, want["dirs"], max_depth=max_depth, bias=bias, shadows=shadows, seed=SEED,
                          pixel_base=PIXEL_BASE, exact=exact, transmission=MODE_NAME[mode])
            st = r.trace_stats()
            assert st["depth_rays"] == want["depth_rays"], (st["depth_rays"], want["depth_rays"])
            assert r.transmit_stats() == stats_of(want), (r.transmit_stats(), stats_of(want))
            assert_same(got["rgb"], want["rgb"], f"{name} {MODE_NAME[mode]} exact {exact}")
            assert np.array_equal(got["rgb8"], ol.oracle_quantise(want["rgb"]))
    # and "off" is the mirror-only loop on the same scene
    off = r.trace(o, want["dirs"], max_depth=max_depth, bias=bias, shadows=shadows, seed=SEED, pixel_base=PIXEL_BASE,
                  transmission="off")
    want_off = oracle_trace(d, o, a, max_depth, bias, OFF, shadows)
    assert r.transmit_stats() == {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}
    assert r.trace_stats()["depth_rays"] == want_off["depth_rays"]
    assert_same(off["rgb"], want_off["rgb"], f"{name} off")
    plain = r.trace(o, want["dirs"], max_depth=max_depth, bias=bias, shadows=shadows, seed=SEED, pixel_base=PIXEL_BASE)
    assert_same(plain["rgb"], off["rgb"], f"{name}: off vs the plain call")


@pytest.mark.gpu
def test_bias_puts_the_refracted_origin_on_the_far_side(esc, r):
    d, o, a = case_rays("slab")
    bias = float(F32(0.02))  # a fifth of a millimetre would hide in the slab; this is 2 % of the box
    want = oracle_trace(d, o, a, 3, bias, REFRACT)
    swapped = oracle_trace(d, o, a, 3, bias, REFRACT, swap_bias=True)
    if not want["usable"].all():  # another bias than case_rays tried: keep what the restatement accepts
        keep = want["usable"]
        o, a = o[keep], a[keep]
        want = oracle_trace(d, o, a, 3, bias, REFRACT)
        swapped = oracle_trace(d, o, a, 3, bias, REFRACT, swap_bias=True)
    assert len(o) >= 64 and want["usable"].all()
    assert want["refracted"] > 0 and want["total_internal"] > 0
    # with the origins on the wrong sides the restatement gives something else ...
    assert (~same_bits(want["rgb"], swapped["rgb"])).any() and want["depth_rays"] != swapped["depth_rays"]
    r.upload(product(d))
    got = r.trace(o, want["dirs"], max_depth=3, bias=bias, seed=SEED, pixel_base=PIXEL_BASE, transmission="refract")
    # ... and the GPU agrees with the right one
    assert r.trace_stats()["depth_rays"] == want["depth_rays"]
    assert r.transmit_stats() == stats_of(want)
    assert_same(got["rgb"], want["rgb"], "bias 0.02")


# ---- 2. nothing transmissive: every mode is the mirror loop --------------------------------------------
@pytest.mark.gpu
def test_modes_on_an_opaque_scene_are_the_plain_calls(esc, r):
    d = cornell()
    # entries that look like glass but are not: tf without ni, ni without tf, NaN
    d["transmission"] = {1: np.array([0.5, 0.5, 0.5, 0.0], F32), 2: np.array([0, 0, 0, 1.5], F32),
                         3: np.array([np.nan, np.nan, np.nan, 1.5], F32), 4: np.array([0.5, 0.5, 0.5, np.nan], F32),
                         5: np.array([-1, -1, 0, 1.5], F32)}
    r.upload(product(d))
    W, H = 97, 61
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()
    o, dd = o.cpu().numpy(), dd.cpu().numpy()
    want = r.trace(o, dd, max_depth=3, bias=1e-4, seed=9, pixel_base=5, face_mode=esc.ESC_FACE_HASH)
    depth = r.trace_stats()["depth_rays"]
    assert depth[1] > 0
    frame = r.render_traced(cam, W, H, spp=4, max_depth=3, bias=1e-4, seed=9)
    for mode in ("off", "refract", "fresnel"):
        got = r.trace(o, dd, max_depth=3, bias=1e-4, seed=9, pixel_base=5, face_mode=esc.ESC_FACE_HASH,
                      transmission=mode)
        assert r.trace_stats()["depth_rays"] == depth
        assert r.transmit_stats() == {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}
        assert_same(got["rgb"], want["rgb"], mode)
        assert np.array_equal(got["rgb8"], want["rgb8"])
        assert_same(r.render_traced(cam, W, H, spp=4, max_depth=3, bias=1e-4, seed=9, transmission=mode), frame,
                    f"frame {mode}")
        assert r.transmit_stats() == {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}


# ---- 3. frames are a composition of public calls -------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_scene(esc, tmp_path_factory):
    import os
    import tarfile
    d = tmp_path_factory.mktemp("models")
    with tarfile.open(os.path.join(ol.ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        if hasattr(tarfile, "data_filter"):
            t.extractall(d, filter="data")
        else:
            t.extractall(d)
    return esc.Scene.load_obj(os.path.join(str(d), "cornell", "CornellBox-Sphere.obj"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["refract", "fresnel"])
@pytest.mark.parametrize("spp", [1, 4])
def test_frames_are_composed_of_camera_rays_and_trace(esc, r, sphere_scene, mode, spp):
    import torch
    dev = torch.device("cuda", r.device)
    sc = sphere_scene
    assert any(sc.transmission(g)[0].any() for g in range(sc.info()["n_geometry"]))
    r.upload(sc)
    W, H, depth, bias, seed = 64, 48, 4, float(F32(1e-4)), 21
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), W, H)
    img, u8 = r.render_traced(cam, W, H, spp=spp, max_depth=depth, bias=bias, seed=seed, want_u8=True,
                              face_mode=esc.ESC_FACE_HASH, transmission=mode)
    st, ts = r.trace_stats(), r.transmit_stats()
    assert ts["refracted"] > 0 and st["depth_rays"][3] > 0, (st, ts)
    if mode == "fresnel":
        assert ts["fresnel_reflected"] > 0
    nn = int(round(spp ** 0.5))
    acc = np.zeros((W * H, 3), F32)
    total = {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}
    rays = 0
    for j in range(spp):  # render_supersampled's sample offsets, in fp32
        dx = F32(F32(F32(j % nn) + F32(0.5)) / F32(nn)) - F32(0.5)
        dy = F32(F32(F32(j // nn) + F32(0.5)) / F32(nn)) - F32(0.5)
        off = torch.from_numpy(np.tile(np.array([dx, dy], F32), (W * H, 1))).to(dev)
        torch.cuda.synchronize()
        o, dd = r.camera_rays(cam, W, H, offsets=off)
        r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
        got = r.trace(o.cpu().numpy(), dd.cpu().numpy(), max_depth=depth, bias=bias, seed=seed + j,
                      face_mode=esc.ESC_FACE_HASH, transmission=mode)
        acc = (acc + got["rgb"]).astype(F32)
        for k, v in r.transmit_stats().items():
            total[k] += v
        rays += r.trace_stats()["rays"]
    want = (acc / F32(spp)).astype(F32)
    assert_same(img.reshape(-1, 3), want, f"{mode} spp {spp}")
    assert np.array_equal(u8.reshape(-1, 3), ol.oracle_quantise(want))
    assert ts == total and st["rays"] == rays
    # the glass changes the picture
    plain = r.render_traced(cam, W, H, spp=spp, max_depth=depth, bias=bias, seed=seed, face_mode=esc.ESC_FACE_HASH)
    assert (~same_bits(plain, img)).any()


# ---- 4. odd table values -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_odd_table_values_match_exact_and_the_restatements_counts(esc, r):
    d = cornell()
    nan, inf = np.nan, np.inf
    odd = [(nan, 0.5, 0.5, 1.5), (-0.5, 0.5, 0.0, 1.5), (inf, 0.5, 0.5, 1.5), (0.5, 0.5, 0.5, 0.0),
           (0.5, 0.5, 0.5, -1.5), (0.5, 0.5, 0.5, nan), (0.5, 0.5, 0.5, inf), (0.5, 0.5, 0.5, 1e-30),
           (0.5, 0.5, 0.5, 1e30), (nan, nan, nan, 1.5), (0.0, -0.0, 1e-45, 1.5), (0.9, 0.9, 0.9, 1.0)]
    rng = np.random.default_rng(6)
    c = rng.uniform([-0.8, 0.2, -0.8], [0.8, 1.7, 0.8], (len(odd), 3))
    d["spheres"] = np.concatenate([c, np.full((len(odd), 1), 0.22)], axis=1).astype(F32)
    d["sphere_materials"] = np.tile(glass(), (len(odd), 1))
    for k, t in enumerate(odd):
        d["sphere_transmission"][k] = np.array(t, F32)
    for g, t in zip(range(1, 6), odd[:5]):  # and on the walls
        d["transmission"][g] = np.array(t, F32)
    for m in [g["material"] for g in d["geometry"]]:
        m[12] = 0.0
    r.upload(product(d))
    o, a = camera_targets(CORNELL_EYE, CORNELL_LOOK, 16, 12)
    o2 = (np.array([0, 1, 0.2], F32) + rng.uniform(-0.3, 0.3, (192, 3))).astype(F32)
    a2 = (o2 + _normalize(rng.standard_normal((192, 3)))).astype(F32)
    o, a = np.concatenate([o, o2]), np.concatenate([a, a2])
    for mode in (REFRACT, FRESNEL):
        for bias in (0.0, 1e-4, 1e22):
            want = oracle_trace(d, o, a, 4, float(F32(bias)), mode, colours=False)
            x = r.trace(o, want["dirs"], max_depth=4, bias=bias, seed=SEED, pixel_base=PIXEL_BASE,
                        transmission=MODE_NAME[mode])
            sa, ta = r.trace_stats(), r.transmit_stats()
            y = r.trace(o, want["dirs"], max_depth=4, bias=bias, seed=SEED, pixel_base=PIXEL_BASE, exact=True,
                        transmission=MODE_NAME[mode])
            sb, tb = r.trace_stats(), r.transmit_stats()
            print(MODE_NAME[mode], bias, sa["depth_rays"][:5], ta, want["depth_rays"][:5], stats_of(want))
            assert_same(x["rgb"], y["rgb"], f"{MODE_NAME[mode]} bias {bias}: filtered vs exact")
            assert np.array_equal(x["rgb8"], y["rgb8"])
            assert sa["depth_rays"] == sb["depth_rays"] and ta == tb
            assert sa["depth_rays"] == want["depth_rays"], (sa["depth_rays"], want["depth_rays"])
            assert ta == stats_of(want), (ta, stats_of(want))
            assert want["refracted"] > 0 and want["depth_rays"][2] > 0


# ---- 5. no interference ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two"])
def test_reference_md5_after_ex_calls(esc, name, tmp_path):
    import hashlib
    r = esc.Renderer(0)
    d, o, a = case_rays("sphere")
    r.upload(product(d))
    want = oracle_trace(d, o, a, 3, 1e-4, FRESNEL)
    r.trace(o, want["dirs"], max_depth=3, bias=1e-4, seed=SEED, pixel_base=PIXEL_BASE, transmission="fresnel")
    r.upload(ol.scene_to_product(ol.load_dump(name)))
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), 1024, 768)
    r.render_traced(cam, 1024, 768, max_depth=2, bias=1e-4, transmission="refract")
    _, u8 = r.render(cam, 1024, 768, want_u8=True)
    md5 = {"one": "b10e1cb14f839129bd111670002cfb0b", "two": "c8137a8d70d8de0ad6a001d41be4e0e1"}[name]
    p = tmp_path / "x.ppm"
    esc.write_ppm(p, u8)
    assert hashlib.md5(p.read_bytes()).hexdigest() == md5
    r.close()


@pytest.mark.gpu
def test_ex_calls_leave_everything_else_alone(esc):
    import torch
    r = esc.Renderer(0)
    sc = esc.Scene.synthetic("c4", 2000)
    sp, _ = sc.spheres()
    n = len(sp)
    sc.set_sphere_transmission(0, np.tile(np.array([0.8, 0.9, 0.7], F32), (n // 3, 1)), np.full(n // 3, 1.5, F32))
    r.upload(sc)
    W, H = 320, 180
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()
    on, dn = o.cpu().numpy(), dd.cpu().numpy()
    frame = r.render(cam, W, H)
    query = r.intersect(on, dn)
    shade = r.shade(on, dn)
    mirror = r.trace(on, dn, max_depth=3, bias=1e-4)
    r.reset_counters()
    r.render(cam, W, H)
    c1 = r.counters()
    big = r.trace(on, dn, max_depth=3, bias=1e-4, transmission="refract")
    assert r.transmit_stats()["refracted"] > 0
    assert (~same_bits(big["rgb"], mirror["rgb"])).any()
    small = r.trace(on[:1000], dn[:1000], max_depth=3, bias=1e-4, transmission="refract")
    assert_same(small["rgb"], big["rgb"][:1000], "n = 1000 after n = 57600")
    r.render_traced(cam, W, H, spp=4, max_depth=2, bias=1e-4, transmission="fresnel")
    assert_same(r.trace(on, dn, max_depth=3, bias=1e-4)["rgb"], mirror["rgb"], "plain trace after _ex calls")
    assert r.transmit_stats() == {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}
    assert_same(r.render(cam, W, H), frame, "frame after _ex calls")
    q2 = r.intersect(on, dn)
    for k in ("t", "geom", "prim"):
        assert np.array_equal(q2[k], query[k]), k
    assert_same(r.shade(on, dn)["rgb"], shade["rgb"], "shade after _ex calls")
    r.reset_counters()
    r.render(cam, W, H)
    assert r.counters() == c1
    # a recorded frame still launches (test_trace_rays.py records on the Cornell box: so does this)
    d, o, a = case_rays("sphere")
    r.upload(product(d))
    W, H = 160, 90
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    frame = r.render(cam, W, H)
    dev = torch.device("cuda", 0)
    out = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
    rec = r.record_strips(cam, W, H, 0, 1, out)
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()
    on, dn = o.cpu().numpy(), dd.cpu().numpy()
    for mode in ("refract", "fresnel"):
        r.trace(on, dn, max_depth=3, bias=1e-4, transmission=mode)
        assert r.transmit_stats()["refracted"] > 0
    r.render_traced(esc.Camera.for_image(CORNELL_EYE, (0.3, 1, 0), 97, 61), 97, 61, spp=4, max_depth=2, bias=1e-4,
                    transmission="fresnel")
    assert_same(r.render(cam, W, H), frame, "Cornell frame after _ex calls")
    out.zero_()
    r.synchronize()
    rec.launch()
    r.synchronize()
    assert_same(out.cpu().numpy().reshape(H, W, 3), frame, "recorded frame after _ex calls")
    rec.close()
    # argument checks reach the caller as errors
    for kw in ({"max_depth": 17, "bias": 0.0}, {"max_depth": 1, "bias": -1.0}):
        with pytest.raises(esc.EscError) as e:
            r.trace(on[:4], dn[:4], transmission="refract", **kw)
        assert e.value.code == -1 and "esc_trace_rays_ex" in str(e.value)
    r.close()
