"""Cases and conditions of the temporal-accumulation tests, chosen on the CPU by the restatement of
tests/temporal_lib.py alone, before anything runs on the GPU.  A case's guides, images and expected answer are
computed once and shared.

(a) traced: the five 16 x 12 frames of tests/ambient_cases.py.  The current frame is ambient_cases.frame_camera's;
    the previous frame is seen by one of three cameras with the same look-at: the same eye, a small eye shift
    and a large one (SHIFTS, in units of the scene's extent, found per scene by a search with the restatement).
    The current image is the restatement's vis (1 channel) or sky light (3 channels) at seed ambient_cases.SEED,
    the history is the previous camera's at seed SEED + 1; the guides are filter_lib.gbuffer's.  history_n is
    drawn by a seeded generator from 1 .. 40 (so some lengths are beyond max_history = 32), with zeros on the
    previous frame's misses and planted on about 6 % of its hits.
(b) synthetic: guides, history and a camera that are plain data, no tracing -- the previous camera looks down
    -z at six planar regions in a 3 x 2 layout, and pixel (w, h) of the current frame is aimed at a chosen point
    (fx, fy) of the previous image: a global shift plus a jitter of eighths of a pixel for most pixels; exact
    integers (ax = ay = 0), exactly -1 and exactly W or H for some; and points behind the camera, on it
    (det = 0), in its plane (det = 0), NaN and infinite positions and normals, misses, and history_n of 0, 1, M,
    INT32_MAX and negative values, NaN / inf in history and current -- at sizes from 2 x 2 to 130 x 70.

The conditions that make the comparison worth having are asserted by check_* below and printed."""
import numpy as np

import ambient_cases as ac
import ambient_lib as al
import filter_lib as fl
import skylight_cases as sc
import skylight_lib as sl
import temporal_lib as tl
from ray_oracle import F32

W, H = ac.FRAME_W, ac.FRAME_H
MAX_HISTORY, NORMAL_COS, PLANE_EXTENTS = 32, 0.9, 0.02
SEEDS = (ac.SEED, ac.SEED + 1)  # of the current image, of the history
CAMERAS = ("same", "small", "large")
# eye shifts of the previous camera in units of the scene's extent
SHIFTS = {
    "CornellBox-Original": {"small": (0.03, 0.02, 0.01), "large": (0.3, 0.1, 0.0)},
    "CornellBox-Sphere": {"small": (0.03, 0.02, 0.01), "large": (0.3, 0.0, 0.0)},
    "rand3": {"small": (0.005, 0.0025, 0.0), "large": (0.03, -0.1, 0.1)},
    "rand5": {"small": (0.005, 0.0025, 0.0), "large": (0.12, 0.0, 0.0)},
    "c2_200": {"small": (0.02, 0.01, 0.0), "large": (0.2, 0.0, 0.0)},
}
TRACED = [(s, c) for s in ac.SCENES for c in CAMERAS]
TRACED_IDS = [f"{s}-{c}" for s, c in TRACED]
SYNTHETIC = [(2, 2), (5, 3), (33, 19), (64, 8), (65, 9), (130, 70)]
SYNTHETIC_IDS = [f"{w}x{h}" for w, h in SYNTHETIC]
SYN_PLANE = 0.05
_FRAMES, _SYN, _WANT = {}, {}, {}


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- (a) ---------------------------------------------------------------------------------------------------
def camera(name, which="same", shifts=None):
    """the current frame's camera ("same"), or a previous camera whose eye is shifted"""
    import esctp1raytracer_amd as esc
    cam = ac.frame_camera(name)
    if which == "same":
        return cam
    s = np.array((shifts or SHIFTS)[name][which], F32)
    eye = (cam.lookfrom + (s * F32(ac.scene(name)[3])).astype(F32)).astype(F32)
    return esc.Camera.for_image(tuple(float(x) for x in eye), tuple(float(x) for x in cam.lookat), W, H,
                                vfov=cam.vfov)


def frame(name, which, seed, cam=None):
    """-> {"guides", "vis" (H, W), "light" (H, W, 3)} of the camera's 16 x 12 frame at the seed, by the
    restatements of the G-buffer, of ambient occlusion (setting 0) and of sky lighting"""
    key = (name, which, seed)
    if cam is not None or key not in _FRAMES:
        d = ac.scene(name)[0]
        if cam is None and which == "same" and seed == ac.SEED:  # the frame the other suites share
            o, dirs = ac.rays(name, "frame")
            amb = ac.want(name, "frame", 0)
            light = sc.want(name, "frame", 0)["light"]
        else:
            o, dirs = ac.camera_rays(cam or camera(name, which), W, H)
            o, dirs = np.ascontiguousarray(o, F32), np.ascontiguousarray(dirs, F32)
            radius, bias = ac.setting(name, 0)
            amb = al.ambient(d, o, dirs, ac.table(), radius, bias, seed, 0)
            light = sl.skylight(d, amb, sc.cube(), sc.K, False)["light"]
        f = {"guides": frozen(fl.gbuffer(d, o, dirs)),
             "vis": np.ascontiguousarray(amb["vis"], F32).reshape(H, W),
             "light": np.ascontiguousarray(light, F32).reshape(H, W, 3)}
        f["vis"].setflags(write=False)
        f["light"].setflags(write=False)
        if cam is not None:
            return f
        _FRAMES[key] = f
    return _FRAMES[key]


def traced_plane(name):
    return float(F32(F32(PLANE_EXTENTS) * F32(ac.scene(name)[3])))


def history_n(prev_guides, seed):
    """1 .. 40 on the previous frame's hits, 0 on its misses and on about 6 % of its hits"""
    g = prev_guides
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 41, (H, W)).astype(np.int32)
    n[rng.random((H, W)) < 0.06] = 0
    n[~((g["geom"] >= 0) | (g["prim"] >= 0)).reshape(H, W)] = 0
    n.setflags(write=False)
    return n


def traced_inputs(name, which, channels):
    """-> dict of temporal_lib.accumulate's / Renderer.temporal_accumulate's inputs of the case"""
    cur, prev = frame(name, "same", SEEDS[0]), frame(name, which, SEEDS[1])
    what = "vis" if channels == 1 else "light"
    return {"current": cur[what], "cur": cur["guides"], "prev_cam": camera(name, which), "history": prev[what],
            "history_n": history_n(prev["guides"], 5 + TRACED.index((name, which))), "prev": prev["guides"]}


def traced_want(name, which, channels=1, taps=4, same_object=True, reverse=False):
    """-> (out, out_n, stats) of temporal_lib.accumulate for the case"""
    key = ("a", name, which, channels, taps, same_object, reverse)
    if key not in _WANT:
        i = traced_inputs(name, which, channels)
        out, n, st = tl.accumulate(i["current"], i["cur"], i["prev_cam"], i["history"], i["history_n"], i["prev"],
                                   taps, MAX_HISTORY, NORMAL_COS, traced_plane(name), same_object, reverse)
        out.setflags(write=False)
        n.setflags(write=False)
        _WANT[key] = (out, n, st)
    return _WANT[key]


def landing(name, which, cam=None, prev_guides=None):
    """where the current frame's hit pixels land in the previous camera's image under taps = 1:
    -> (hit, inside, to itself, largest |fx - round(fx)| over the hit pixels that land inside)"""
    g = frame(name, "same", SEEDS[0])["guides"]
    hit = g["has"].reshape(H, W)
    with np.errstate(all="ignore"):
        fx, fy, z = tl.reproject(cam or camera(name, which), g["position"], W, H)
        x0, y0 = np.floor(fx + F32(0.5)), np.floor(fy + F32(0.5))
        inside = hit & (z > 0) & (x0 >= 0) & (x0 <= W - 1) & (y0 >= 0) & (y0 <= H - 1)
        hh, ww = np.mgrid[0:H, 0:W]
        itself = inside & (x0 == ww) & (y0 == hh)
        off = float(np.max(np.abs(fx - x0)[inside])) if inside.any() else 0.0
    return int(hit.sum()), int(inside.sum()), int(itself.sum()), off


def check_traced(name, which):
    """the per-case conditions: the same camera maps every hit pixel to itself; the small shift keeps most
    pixels; the large one reuses between 25 % and 95 % of the hit pixels and sends some outside the image"""
    hit, inside, itself, off = landing(name, which)
    st1 = traced_want(name, which, 1, 1)[2]
    st4 = traced_want(name, which, 1, 4)[2]
    share = st4["reused_pixels"] / max(1, hit)
    print(f"{name} {which}: {hit} hit pixels, {inside} land inside, {itself} on themselves (largest |fx - round| "
          f"{off:.2e}); taps 1 reuses {st1['reused_pixels']}, taps 4 reuses {st4['reused_pixels']} "
          f"({share:.3f}), rejects {[st4[s] for s in tl.STOPS]} of {st4['taps_tested']} taps")
    assert hit >= 0.9 * W * H
    if which == "same":
        assert inside == itself == hit and off < 1e-3, (name, inside, itself, off)
    elif which == "small":
        assert itself < hit and share >= 0.5, (name, itself, share)
    else:
        assert 0.25 <= share <= 0.95, (name, share)
        assert inside < hit, (name, inside, hit)
    assert 0 < st4["taps_accepted"] < st4["taps_tested"], (name, which, st4)


def traced_rejects(same_object):
    """over the (a) cases with taps = 4: how many taps each stop rejected"""
    tot = dict.fromkeys(tl.STOPS, 0)
    for name, which in TRACED:
        st = traced_want(name, which, 1, 4, same_object)[2]
        for s in tl.STOPS:
            tot[s] += st[s]
    return tot


# ---- (b) ---------------------------------------------------------------------------------------------------
# region of the previous image: its depth below the camera, its normal (unnormalised) and its (geom, prim)
REGIONS = ((1.0, (0.0, 0.0, 1.0), (0, 7)), (1.5, (-0.02, 0.0, 1.0), (0, 3)), (2.0, (-1.0, -0.3, 1.0), (1, 0)),
           (1.0, (0.0, 0.0, 1.0), (2, 5)), (1.25, (0.5, -0.5, 1.0), (-1, 0)), (1.25, (0.5, -0.5, 1.0), (-1, 1)))
SYN_ORIGIN = (0.5, -0.25, 2.0)
SYN_SHIFT = (1.25, -0.625)
INT32_MAX = 2 ** 31 - 1


def synthetic_camera(Ws, Hs):
    """origin O, and the ray through pixel (fx, fy) of the previous image is O + l * (fx, fy, -1)"""
    o = np.array(SYN_ORIGIN, F32)
    return {"origin": o, "lower_left_corner": (o + np.array((0, 0, -1), F32)).astype(F32),
            "horizontal": np.array((Ws - 1, 0, 0), F32), "vertical": np.array((0, Hs - 1, 0), F32)}


def _regions(Ws, Hs, ww, hh):
    return np.minimum(ww * 3 // Ws, 2) + 3 * np.minimum(hh * 2 // Hs, 1)


def synthetic(Ws, Hs, seed=23):
    """-> {"cur", "prev" (guides), "prev_cam", "history_n" (H, W), "current1", "history1" (H, W), "current3",
    "history3" (H, W, 3), "kind" (H, W): how the pixel was aimed}"""
    key = (Ws, Hs, seed)
    if key in _SYN:
        return _SYN[key]
    rng = np.random.default_rng(seed + 1000 * Ws + Hs)
    hh, ww = np.mgrid[0:Hs, 0:Ws]
    o = np.array(SYN_ORIGIN, F32)
    depth = np.array([r[0] for r in REGIONS], F32)
    normal = np.array([np.array(r[1]) / np.linalg.norm(r[1]) for r in REGIONS]).astype(F32)
    ids = np.array([r[2] for r in REGIONS], np.int32)

    def surface(fx, fy, reg):
        d = depth[reg]
        return (o + np.stack([d * fx, d * fy, -d], axis=-1).astype(F32)).astype(F32)

    # the previous frame: pixel q sees its region's plane at q
    reg_p = _regions(Ws, Hs, ww, hh)
    prev = {"normal": normal[reg_p].copy(), "position": surface(ww.astype(F32), hh.astype(F32), reg_p),
            "geom": ids[reg_p, 0].copy(), "prim": ids[reg_p, 1].copy()}
    # the current frame: pixel p is aimed at (fx, fy) of the previous image
    kind = rng.choice(8, (Hs, Ws), p=(0.60, 0.10, 0.06, 0.06, 0.05, 0.04, 0.04, 0.05))
    jit = rng.integers(0, 8, (2, Hs, Ws)).astype(F32) / F32(8)
    fx = (ww + F32(SYN_SHIFT[0]) + jit[0]).astype(F32)
    fy = (hh + F32(SYN_SHIFT[1]) + jit[1]).astype(F32)
    whole = kind == 1  # ax = ay = 0: three of the four taps have k = 0
    fx[whole], fy[whole] = ww[whole] + 1, hh[whole]
    edge = kind == 2  # exactly -1, W or H
    pick = rng.integers(0, 4, (Hs, Ws))
    fx[edge & (pick == 0)] = -1
    fx[edge & (pick == 1)] = Ws
    fy[edge & (pick == 2)] = -1
    fy[edge & (pick == 3)] = Hs
    half = kind == 3  # whole in x only, and the last column / row exactly
    fx[half] = np.where(pick[half] < 2, Ws - 1, ww[half])
    reg_c = _regions(Ws, Hs, np.clip(np.floor(fx + F32(0.5)), 0, Ws - 1).astype(np.int64),
                     np.clip(np.floor(fy + F32(0.5)), 0, Hs - 1).astype(np.int64))
    P = surface(fx, fy, reg_c)
    N = normal[reg_c].copy()
    G, R = ids[reg_c, 0].copy(), ids[reg_c, 1].copy()
    behind = kind == 4  # behind the camera, on it (v = 0: det = 0), in its plane (v.z = 0: det = 0)
    P[behind & (pick == 0)] = (o + (o - P[behind & (pick == 0)]).astype(F32)).astype(F32)
    P[behind & (pick == 1)] = o
    P[behind & (pick >= 2), 2] = o[2]
    odd = kind == 5  # NaN and infinite positions and normals
    P[odd & (pick == 0), 0] = np.nan
    P[odd & (pick == 1), 1] = np.inf
    N[odd & (pick == 2)] = np.nan
    N[odd & (pick == 3), 2] = -np.inf
    miss = kind == 6
    P[miss], N[miss], G[miss], R[miss] = 0, 0, -1, -1
    cur = {"normal": N, "position": P, "geom": G, "prim": R}
    # the previous frame's own misses and odd values
    pm = rng.random((Hs, Ws)) < 0.06
    prev["position"][pm], prev["normal"][pm], prev["geom"][pm], prev["prim"][pm] = 0, 0, -1, -1
    pn = (rng.random((Hs, Ws)) < 0.03) & ~pm
    prev["normal"][pn] = np.nan
    pp = (rng.random((Hs, Ws)) < 0.02) & ~pm
    prev["position"][pp, 2] = np.where(rng.random(int(pp.sum())) < 0.5, np.nan, np.inf)
    hn = rng.integers(1, 2 * MAX_HISTORY, (Hs, Ws)).astype(np.int32)
    special = np.array([0, 0, 1, MAX_HISTORY, INT32_MAX, -1, -INT32_MAX - 1, MAX_HISTORY - 1], np.int64)
    sp = rng.random((Hs, Ws)) < 0.25
    hn[sp] = special[rng.integers(0, len(special), int(sp.sum()))].astype(np.int32)
    out = {"cur": frozen(cur), "prev": frozen(prev), "prev_cam": synthetic_camera(Ws, Hs), "history_n": hn,
           "kind": kind}
    for ch in (1, 3):
        shape = (Hs, Ws) if ch == 1 else (Hs, Ws, 3)
        for what in ("current", "history"):
            a = rng.random(shape).astype(F32)
            bad = rng.random((Hs, Ws)) < 0.02
            a[bad] = np.array([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, int(bad.sum()))][
                (...,) + (None,) * (ch == 3)]
            out[f"{what}{ch}"] = a
    _SYN[key] = frozen(out)
    return _SYN[key]


def synthetic_want(Ws, Hs, channels=1, taps=4, same_object=True, reverse=False):
    key = ("b", Ws, Hs, channels, taps, same_object, reverse)
    if key not in _WANT:
        g = synthetic(Ws, Hs)
        out, n, st = tl.accumulate(g[f"current{channels}"], g["cur"], g["prev_cam"], g[f"history{channels}"],
                                   g["history_n"], g["prev"], taps, MAX_HISTORY, NORMAL_COS, SYN_PLANE, same_object,
                                   reverse)
        out.setflags(write=False)
        n.setflags(write=False)
        _WANT[key] = (out, n, st)
    return _WANT[key]


def synthetic_landings(Ws, Hs):
    """what the restatement's reprojection makes of the aimed pixels: counts of hit pixels whose fx or fy is
    exactly whole, exactly -1, exactly W or H, not finite, and whose z <= 0"""
    g = synthetic(Ws, Hs)
    hit = (g["cur"]["geom"] >= 0) | (g["cur"]["prim"] >= 0)
    with np.errstate(all="ignore"):
        fx, fy, z = tl.reproject(g["prev_cam"], g["cur"]["position"], Ws, Hs)
        ok = hit & np.isfinite(fx) & np.isfinite(fy) & (z > 0)
        return {"whole": int((ok & (fx == np.floor(fx)) & (fy == np.floor(fy))).sum()),
                "minus_one": int((ok & ((fx == -1) | (fy == -1))).sum()),
                "size": int((ok & ((fx == Ws) | (fy == Hs))).sum()),
                "not_finite": int((hit & ~(np.isfinite(fx) & np.isfinite(fy) & np.isfinite(z))).sum()),
                "behind": int((hit & (z <= 0)).sum())}


def check_synthetic():
    """over the (b) cases: every stop rejects, taps with k = 0 are skipped untested, every kind of landing
    occurs, every history length of the list is met by a tested tap"""
    tot = dict.fromkeys(tl.STOPS, 0)
    land = dict.fromkeys(("whole", "minus_one", "size", "not_finite", "behind"), 0)
    for Ws, Hs in SYNTHETIC:
        st = synthetic_want(Ws, Hs)[2]
        l = synthetic_landings(Ws, Hs)
        print(f"{Ws}x{Hs}: hit {st['hit_pixels']}, reused {st['reused_pixels']}, tested {st['taps_tested']}, "
              f"accepted {st['taps_accepted']}, rejects {[st[s] for s in tl.STOPS]}, landings {l}")
        for s in tl.STOPS:
            tot[s] += st[s]
        for k in land:
            land[k] += l[k]
        assert 0 < st["reused_pixels"] < st["hit_pixels"] or Ws * Hs <= 15, (Ws, Hs, st)
        if Ws * Hs >= 33 * 19:
            assert l["whole"] >= 1, (Ws, Hs, l)
            # a pixel that lands on whole coordinates inside the image tests one tap, not four
            assert st["taps_tested"] < 4 * st["hit_pixels"]
    assert all(tot[s] >= 1 for s in tl.STOPS), tot
    assert all(land[k] >= 1 for k in land), land
    return tot, land


# ---- a sequence of frames ------------------------------------------------------------------------------------
SEQ_SCENES = ("rand5", "c2_200")
SEQ_FRAMES, SEQ_MAX_HISTORY = 5, 3
# eye shift per frame in units of the scene's extent: the camera moves in, turns back and stops
SEQ_STEPS = ((0.0, 0.0, 0.0), (0.004, 0.002, 0.0), (0.008, 0.004, 0.0), (0.004, 0.002, 0.0), (0.004, 0.002, 0.0))


def sequence(name, channels, taps=4):
    """-> [(camera, image, guides, (out, out_n, stats))] for SEQ_FRAMES frames: frame f is seen from the
    f-th eye at seed f, and the restatement's out / out_n / guides of frame f - 1 are its history (the first
    frame starts from zero history), with max_history = SEQ_MAX_HISTORY so that the cap engages"""
    key = ("s", name, channels, taps)
    if key not in _WANT:
        frames, acc, n, pcam, pg = [], None, None, None, None
        for f in range(SEQ_FRAMES):
            cam = camera(name, f, {name: {f: SEQ_STEPS[f]}})
            fk = (name, "seq", f)
            if fk not in _FRAMES:
                _FRAMES[fk] = frame(name, "seq", f, cam)
            fr = _FRAMES[fk]
            img = fr["vis" if channels == 1 else "light"]
            if f == 0:
                acc, n, pcam, pg = np.zeros(img.shape, F32), np.zeros((H, W), np.int32), cam, fr["guides"]
            acc, n, st = tl.accumulate(img, fr["guides"], pcam, acc, n, pg, taps, SEQ_MAX_HISTORY, NORMAL_COS,
                                       traced_plane(name))
            acc.setflags(write=False)
            n.setflags(write=False)
            frames.append((cam, img, fr["guides"], (acc, n, st)))
            pcam, pg = cam, fr["guides"]
        _WANT[key] = frames
    return _WANT[key]


def check_sequence(name):
    """the first frame reuses nothing, every later one does, the lengths reach the cap and some stay below it"""
    for ch in (1, 3):
        seq = sequence(name, ch)
        ns = [s[3][1] for s in seq]
        reused = [s[3][2]["reused_pixels"] for s in seq]
        print(f"{name} channels {ch}: reused {reused}, largest n {[int(n.max()) for n in ns]}, "
              f"pixels at the cap {[int((n == SEQ_MAX_HISTORY).sum()) for n in ns]}")
        assert reused[0] == 0 and all(r > 0 for r in reused[1:]), reused
        assert ns[0].max() == 1 and ns[-1].max() == SEQ_MAX_HISTORY
        assert ((ns[-1] >= 1) & (ns[-1] < SEQ_MAX_HISTORY)).any()
        assert seq[1][0].vectors()["origin"].tobytes() != seq[0][0].vectors()["origin"].tobytes()
