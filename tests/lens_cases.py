"""Cameras, frames and lens settings of the thin-lens tests, chosen on the CPU by the restatement of
tests/lens_lib.py alone, before anything runs on the GPU.  The restatement's answer of a case is computed once
and shared by the tests that need it.

A case is (camera, frame, aperture, focus, table, sample, offsets, rows):
  cameras    ambient_cases.frame_camera of CornellBox-Original and of c2_200, and the synthetic view
  frames     17 x 13 (221 rays: under one workgroup) and 33 x 9 (297 rays: crosses a workgroup)
  apertures  0, about 1 % and about 10 % of the scene's extent (the synthetic view: c2_200's extent)
  focus      the fp32 distance from the eye to the look-at point, and a quarter of it
  tables     (S, K) = (1, 4) and (3, 16): one modulus that is no power of two
  samples    k = 0 and k = K - 1
  offsets    none, and an (n, 2) array of sub-pixel offsets (rng seed 7, uniform in [-0.5, 0.5))
  rows       the whole frame, and rows 4..9

check_condition is what makes an aperture > 0 case worth comparing: at least 90 % of its rays differ in bits
from the pinhole ray of the same pixel and offset."""
import numpy as np

import ambient_cases as ac
import lens_lib as ll
from ray_oracle import F32, dot, same_bits

CAMERAS = ("CornellBox-Original", "c2_200", "synthetic")
FRAMES = ((17, 13), (33, 9))
APERTURES = (0.0, 0.01, 0.10)  # in units of the scene's extent
FOCUS = (1.0, 0.25)            # in units of the distance to the look-at point
TABLES = ((1, 4), (3, 16))
ROWS = (None, (4, 9))
TABLE_SEED, LENS_SEED, OFFSET_SEED = 3, 5, 7

_CAMS, _WANT, _OFFS = {}, {}, {}


def table(S, K, seed=TABLE_SEED):
    import esctp1raytracer_amd as esc
    return esc.lens_table(S, K, seed)


def camera(name, W, H):
    """-> (Camera, extent of its scene, fp32 distance from the eye to the look-at point)"""
    if (name, W, H) not in _CAMS:
        import esctp1raytracer_amd as esc
        if name == "synthetic":
            eye, look = esc.synthetic_view()
            cam, ext = esc.Camera.for_image(tuple(map(float, eye)), tuple(map(float, look)), W, H), ac.scene("c2_200")[3]
        else:
            cam, ext = ac.frame_camera(name, W, H), ac.scene(name)[3]
        v = (cam.lookat - cam.lookfrom).astype(F32)
        _CAMS[(name, W, H)] = (cam, float(ext), float(np.sqrt(dot(v, v)).astype(F32)))
    return _CAMS[(name, W, H)]


def pixels(W, H, rows):
    r0, r1 = (0, H) if rows is None else rows
    return np.arange(r0 * W, r1 * W, dtype=np.int64)


def offsets(n):
    if n not in _OFFS:
        o = np.random.default_rng(OFFSET_SEED).uniform(-0.5, 0.5, (n, 2)).astype(F32)
        o.setflags(write=False)
        _OFFS[n] = o
    return _OFFS[n]


def cases(name, W, H):
    """every case of one camera and frame, as dicts"""
    _, ext, dist = camera(name, W, H)
    out = []
    for S, K in TABLES:
        for ap in APERTURES:
            for fo in FOCUS:
                for k in (0, K - 1):
                    for with_offsets in (False, True):
                        for rows in ROWS:
                            out.append({"camera": name, "W": W, "H": H, "S": S, "K": K, "k": k, "rows": rows,
                                        "aperture": float(F32(F32(ap) * F32(ext))), "focus_dist": float(F32(F32(fo) * F32(dist))),
                                        "offsets": with_offsets})
    return out


def key(c):
    return tuple(c[x] for x in ("camera", "W", "H", "S", "K", "k", "rows", "aperture", "focus_dist", "offsets"))


def case_offsets(c):
    return offsets(len(pixels(c["W"], c["H"], c["rows"]))) if c["offsets"] else None


def want(c):
    """the restatement's rays (origins, dirs) of a case, computed once, never written to"""
    if key(c) not in _WANT:
        cam = camera(c["camera"], c["W"], c["H"])[0]
        o, d = ll.lens_rays(cam.vectors(), c["W"], c["H"], pixels(c["W"], c["H"], c["rows"]), c["aperture"], c["focus_dist"],
                            table(c["S"], c["K"]), c["k"], LENS_SEED, case_offsets(c))
        o.setflags(write=False)
        d.setflags(write=False)
        _WANT[key(c)] = (o, d)
    return _WANT[key(c)]


def pinhole(c):
    """the pinhole rays of the same pixels and offsets"""
    return want(dict(c, aperture=0.0))


def moved_share(c):
    """the share of a case's rays that differ in bits, in origin or direction, from the pinhole ray"""
    (o, d), (o0, d0) = want(c), pinhole(c)
    return float((~(same_bits(o, o0).all(axis=1) & same_bits(d, d0).all(axis=1))).mean())


def check_condition(c):
    if c["aperture"] > 0:
        share = moved_share(c)
        assert share >= 0.90, (key(c), share)
