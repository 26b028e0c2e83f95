"""Cases and conditions of the filter tests, chosen on the CPU by the restatement of tests/filter_lib.py alone,
before anything runs on the GPU.  A case's guides, image and expected answer are computed once and shared.

(a) traced: the five 16 x 12 frames of tests/ambient_cases.py at settings 0 and 1.  The 1-channel image is the
    restatement's vis, the 3-channel one the restatement's sky light (tests/skylight_cases.py), the guides are
    filter_lib.gbuffer's.  L = 3, normal_cos 0.9, plane_dist 0.02 x the scene's extent, same_object on and off.
(b) synthetic: guides made by a seeded generator without any tracing -- six planar regions in a 3 x 2 layout
    (two of them nearly parallel and 0.5 apart on one geometry, two on one plane but different geometries, two
    spheres on one plane), about 8 % misses and 2 % NaN normals, a random image -- at sizes from 1 x 1 to
    130 x 70, with steps larger than the image on purpose: every non-centre tap then falls outside.

The conditions that make the comparison worth having are asserted by check_* below and printed."""
import numpy as np

import ambient_cases as ac
import filter_lib as fl
import skylight_cases as sc
from ray_oracle import F32

ITER_A, NORMAL_COS, PLANE_EXTENTS = 3, 0.9, 0.02
TRACED = [(s, k) for s in ac.SCENES for k in (0, 1)]
TRACED_IDS = [f"{s}-{k}" for s, k in TRACED]
# (W, H, L)
SYNTHETIC = [(1, 1, 1), (1, 7, 3), (5, 3, 2), (33, 19, 3), (64, 8, 4), (65, 9, 5), (130, 70, 6)]
SYNTHETIC_IDS = [f"{w}x{h}-L{l}" for w, h, l in SYNTHETIC]
SYN_PLANE = 0.05
_GUIDES, _SYN, _WANT = {}, {}, {}


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- (a) ---------------------------------------------------------------------------------------------------
def traced_guides(name):
    """filter_lib.gbuffer of the scene's 16 x 12 frame rays"""
    if name not in _GUIDES:
        _GUIDES[name] = frozen(fl.gbuffer(ac.scene(name)[0], *ac.rays(name, "frame")))
    return _GUIDES[name]


def traced_plane(name):
    return float(F32(F32(PLANE_EXTENTS) * F32(ac.scene(name)[3])))


def traced_image(name, k, channels):
    shape = (ac.FRAME_H, ac.FRAME_W)
    if channels == 1:
        return ac.want(name, "frame", k)["vis"].reshape(shape)
    return sc.want(name, "frame", k)["light"].reshape(shape + (3,))


def traced_want(name, k, channels=1, same_object=True, descending=False):
    """-> (out, stats) of filter_lib.atrous for the case"""
    key = ("a", name, k, channels, same_object, descending)
    if key not in _WANT:
        out, st = fl.atrous(traced_image(name, k, channels), traced_guides(name), ITER_A, NORMAL_COS,
                            traced_plane(name), same_object, descending)
        out.setflags(write=False)
        _WANT[key] = (out, st)
    return _WANT[key]


def check_traced(name, k):
    """the per-case conditions: the order shows, the accepted share is neither nothing nor all, the variance falls"""
    img = traced_image(name, k, 1)
    out, st = traced_want(name, k)
    desc, _ = traced_want(name, k, descending=True)
    has = traced_guides(name)["has"].reshape(img.shape)
    changed = int(((out.view(np.uint32) != desc.view(np.uint32)) & has).sum())
    share = st["taps_accepted"] / max(1, st["taps_tested"])
    v0, v1 = float(np.var(img[has].astype(np.float64))), float(np.var(out[has].astype(np.float64)))
    print(f"{name} setting {k}: {int(has.sum())} hit pixels, descending order changes {changed}, accepted "
          f"{share:.3f} of {st['taps_tested']} taps, rejects {[st[s] for s in fl.STOPS]}, variance {v0:.4f} -> {v1:.4f}")
    assert changed >= 0.10 * has.sum(), (name, k, changed)
    assert 0.2 <= share <= 0.995, (name, k, share)
    assert v1 < v0, (name, k, v0, v1)


def traced_rejects(same_object):
    """over the (a) cases: how many taps each stop rejected"""
    tot = dict.fromkeys(fl.STOPS, 0)
    for name, k in TRACED:
        st = traced_want(name, k, 1, same_object)[1]
        for s in fl.STOPS:
            tot[s] += st[s]
    return tot


# ---- (b) ---------------------------------------------------------------------------------------------------
# region: (a, b, c) of the plane z = a*x + b*y + c over x = 0.1*w, y = 0.1*h, and its (geom, prim)
REGIONS = (((0.0, 0.0, 0.0), (0, 7)), ((0.02, 0.0, 0.5), (0, 3)), ((1.0, 0.3, 0.0), (1, 0)),
           ((0.0, 0.0, 0.0), (2, 5)), ((-0.5, 0.5, 0.0), (-1, 0)), ((-0.5, 0.5, 0.0), (-1, 1)))


def synthetic(W, H, seed=11):
    """-> {"normal", "position" (H, W, 3), "geom", "prim" (H, W), "image1" (H, W), "image3" (H, W, 3)}"""
    key = (W, H, seed)
    if key not in _SYN:
        rng = np.random.default_rng(seed + 1000 * W + H)
        hh, ww = np.mgrid[0:H, 0:W]
        reg = np.minimum(ww * 3 // max(W, 1), 2) + 3 * np.minimum(hh * 2 // max(H, 1), 1)
        x, y = (ww * F32(0.1)).astype(F32), (hh * F32(0.1)).astype(F32)
        N = np.zeros((H, W, 3), F32)
        P = np.zeros((H, W, 3), F32)
        G = np.full((H, W), -1, np.int32)
        R = np.full((H, W), -1, np.int32)
        for r, ((a, b, c), (g, p)) in enumerate(REGIONS):
            m = reg == r
            n = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
            N[m] = n.astype(F32)
            P[m] = np.stack([x[m], y[m], (F32(a) * x[m] + F32(b) * y[m] + F32(c)).astype(F32)], axis=-1)
            G[m], R[m] = g, p
        miss = rng.random((H, W)) < 0.08
        N[miss], P[miss], G[miss], R[miss] = 0, 0, -1, -1
        nan = (rng.random((H, W)) < 0.02) & ~miss
        N[nan] = np.nan
        _SYN[key] = frozen({"normal": N, "position": P, "geom": G, "prim": R,
                            "image1": rng.random((H, W)).astype(F32), "image3": rng.random((H, W, 3)).astype(F32)})
    return _SYN[key]


def synthetic_want(W, H, L, channels=1, same_object=True):
    key = ("b", W, H, L, channels, same_object)
    if key not in _WANT:
        g = synthetic(W, H)
        out, st = fl.atrous(g[f"image{channels}"], g, L, NORMAL_COS, SYN_PLANE, same_object)
        out.setflags(write=False)
        _WANT[key] = (out, st)
    return _WANT[key]


def check_synthetic():
    """over the (b) cases every stop rejects, and the plane stop does at every size from 33 x 19 up"""
    tot = dict.fromkeys(fl.STOPS, 0)
    for W, H, L in SYNTHETIC:
        st = synthetic_want(W, H, L)[1]
        print(f"{W}x{H} L {L}: tested {st['taps_tested']}, accepted {st['taps_accepted']}, rejects "
              f"{[st[s] for s in fl.STOPS]}")
        for s in fl.STOPS:
            tot[s] += st[s]
        if (W, H, L) in SYNTHETIC[3:]:  # 33 x 19 and above
            assert st["plane"] >= 1, (W, H, st)
        if W * H == 1:  # every non-centre tap falls outside
            assert st["taps_tested"] == 0, st
    assert all(tot[s] >= 1 for s in fl.STOPS), tot
    return tot
