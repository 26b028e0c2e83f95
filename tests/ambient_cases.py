"""Scenes, rays and settings of the ambient-occlusion tests, chosen on the CPU by the restatement of
tests/ambient_lib.py alone, before anything runs on the GPU.  The restatement's answer of a case is computed
once and shared by the tests that need it.

A case is (scene, ray set, setting): five scenes, two ray sets (96 rays from the eye to points on the scene's
surfaces, rng seed 1; a 16 x 12 camera frame), three settings (radius, bias) with the radius in units of the
scene's extent.  check_condition is what makes a case worth comparing: most rays hit, and the counts are
neither all in between nor all at an end."""
import numpy as np

import ambient_lib as al
import oracle_lib as ol
import random_scenes as rs
from ray_cases import CORNELL_EYE, CORNELL_LOOK, box, surface_points
from ray_oracle import F32, FLT_MAX, normalize

SCENES = ("CornellBox-Original", "CornellBox-Sphere", "rand3", "rand5", "c2_200")
RAY_SETS = ("surface", "frame")
# (radius in extents, or None: unbounded; bias).  bias 0: a sample may meet its own surface at t ~ 0, which
# the reference's own rounding decides -- exactly what must match
SETTINGS = ((None, 1e-4), (0.25, 1e-3), (0.05, 0.0))
CASES = [(s, r, k) for s in SCENES for r in RAY_SETS for k in range(len(SETTINGS))]
TABLE_SETS, TABLE_SAMPLES, TABLE_SEED = 4, 8, 3
SEED, PIXEL_BASE = 77, 1234
# the frame: aimed at one of the surface points of the ray set above (its index), with a view narrow enough
# that most rays hit, from the scene's own eye or from halfway between the eye and that point.  Chosen per
# scene by a search with the restatement alone, so that the condition holds at all three settings.
FRAME_W, FRAME_H = 16, 12
FRAME_VIEW = {"CornellBox-Original": (4, 20.0, True), "CornellBox-Sphere": (11, 30.0, True), "rand3": (0, 30.0, False),
              "rand5": (0, 40.0, False), "c2_200": (5, 40.0, False)}

_SCENES, _RAYS, _WANT = {}, {}, {}


def table(sets=TABLE_SETS, samples=TABLE_SAMPLES, seed=TABLE_SEED):
    import esctp1raytracer_amd as esc
    return esc.ambient_table(sets, samples, seed)


def scene(name):
    """-> (scene dict, eye, look, extent)"""
    if name not in _SCENES:
        if name.startswith("CornellBox"):
            d, eye, look = ol.load_dump(name), CORNELL_EYE, CORNELL_LOOK
        elif name.startswith("rand"):
            d, eye, look = rs.random_scene(int(name[4:]))[:3]
        else:  # analytic spheres: the synthetic config c2 with 200 of them
            import esctp1raytracer_amd as esc
            d = ol.scene_from_product(esc.Scene.synthetic("c2", 200))
            eye, look = (tuple(float(x) for x in v) for v in esc.synthetic_view())
        lo, hi = box(d)
        _SCENES[name] = (d, eye, look, float(F32(np.max(hi - lo))))
    return _SCENES[name]


def setting(name, k):
    """-> (radius, bias) as the floats the call takes"""
    rad, bias = SETTINGS[k]
    ext = scene(name)[3]
    return (float(FLT_MAX) if rad is None else float(F32(F32(rad) * F32(ext)))), float(F32(bias))


def frame_camera(name, W=FRAME_W, H=FRAME_H):
    import esctp1raytracer_amd as esc
    d, eye, _, _ = scene(name)
    j, vfov, halfway = FRAME_VIEW[name]
    at = surface_points(d, 96, np.random.default_rng(1))[j]
    eye = (np.array(eye) + at) / 2 if halfway else np.array(eye)
    return esc.Camera.for_image(tuple(float(x) for x in eye), tuple(float(x) for x in at), W, H, vfov=vfov)


def camera_rays(cam, W, H):
    """esc_camera_rays without offsets (camera.h:31-34) in numpy fp32 -> (origins, dirs), ray h * W + w"""
    v = cam.vectors()
    o = np.tile(v["origin"], (W * H, 1)).astype(F32)
    s = (np.arange(W, dtype=F32) / F32(W - 1)).astype(F32)[None, :, None]
    t = (np.arange(H, dtype=F32) / F32(H - 1)).astype(F32)[:, None, None]
    p = ((v["lower_left_corner"] + (v["horizontal"] * s).astype(F32)).astype(F32) + (v["vertical"] * t).astype(F32))
    return o, normalize((p.astype(F32).reshape(-1, 3) - o).astype(F32))


def rays(name, ray_set):
    """-> (origins, dirs), float32"""
    if (name, ray_set) not in _RAYS:
        d, eye, look, _ = scene(name)
        if ray_set == "surface":
            pts = surface_points(d, 96, np.random.default_rng(1))
            o = np.tile(np.array(eye, F32), (len(pts), 1))
            with np.errstate(all="ignore"):
                dirs = normalize((pts - o).astype(F32))
        else:
            o, dirs = camera_rays(frame_camera(name), FRAME_W, FRAME_H)
        _RAYS[(name, ray_set)] = (np.ascontiguousarray(o, F32), np.ascontiguousarray(dirs, F32))
    return _RAYS[(name, ray_set)]


def want(name, ray_set, k):
    """the restatement's answer of a case (ambient_lib.ambient's dict), computed once, never written to"""
    key = (name, ray_set, k)
    if key not in _WANT:
        o, dirs = rays(name, ray_set)
        radius, bias = setting(name, k)
        w = al.ambient(scene(name)[0], o, dirs, table(), radius, bias, SEED, PIXEL_BASE if ray_set == "surface" else 0)
        for v in w.values():
            v.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def condition(w, K=TABLE_SAMPLES):
    """-> (share of rays that hit, share of hit rays with 0 < count < K, share with count 0 or K)"""
    has, count = w["has"], w["count"]
    nh = max(1, int(has.sum()))
    part = int(((count > 0) & (count < K) & has).sum())
    ends = int((((count == 0) | (count == K)) & has).sum())
    return has.mean(), part / nh, ends / nh


def check_condition(name, ray_set, k):
    hit, part, ends = condition(want(name, ray_set, k))
    print(f"{name} {ray_set} setting {k}: {hit:.3f} of the rays hit, {part:.3f} of those in between, {ends:.3f} at an end")
    assert hit >= 0.90, (name, ray_set, k, hit)
    assert part >= 0.10, (name, ray_set, k, part)
    assert ends >= 0.05, (name, ray_set, k, ends)
