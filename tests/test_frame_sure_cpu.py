"""CPU: the host's sufficient condition for "every shadow-ray origin lies in the grown scene box"
(host/scene_tables.cpp shadow_origins_inside, DESIGN.md 3.9 "Frames that need no fallback"), the condition
under which the one-kernel frame runs without its vote and fallback sweep.

Cameras around the boxes of the c2-c5 workloads (small cuts of them), in six directions from the box's
middle, at distances from 0 to past the bound in octaves.  Wherever the predicate says yes, the shadow
origins of a 32 x 16 frame -- the reference arithmetic's own fl(origin + dir (t - eps)), recorded by the
oracle per pixel and light -- all lie in [scene_lo, scene_hi], fp32 compares as the kernel makes them.
The predicate must say yes next to the scene and no far away, or the statement above would be empty; and
no for a non-finite coordinate, a camera in a triangle's plane and a scene with two lights."""
import numpy as np
import pytest

import oracle_lib as ol

F32 = np.float32
W, H = 32, 16
CUTS = {"c2": 60, "c3": 120, "c4": 200, "c5": 8}  # spheres; c5: quads per side of its mesh


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as esc
    return esc


def box_of(sc):
    hdr = sc.table("header").view(F32)
    return hdr[4:7].astype(np.float64), hdr[7:10].astype(np.float64)


def origins_in_box(sc, d, eye, look):
    """(shadow origins of the frame inside the box, shadow origins)"""
    hdr = sc.table("header").view(F32)
    lo, hi = hdr[4:7], hdr[7:10]
    rec = ol.oracle_shadow_rays(d, eye, look, W, H)[:, 0]
    p = rec[rec[:, 7] > 0, :3]
    return int(((p >= lo) & (p <= hi)).all(axis=1).sum()), len(p)


@pytest.mark.parametrize("config", list(CUTS))
def test_predicate_implies_origins_inside(esc, config):
    sc = esc.Scene.synthetic(config, CUTS[config])
    d = ol.scene_from_product(sc)
    lo, hi = box_of(sc)
    mid, half, size = 0.5 * (lo + hi), 0.5 * (hi - lo), float((hi - lo).sum())
    yes = no = rays = 0
    said = {}
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for k in [None] + list(range(-4, 8)):  # in the middle; then size / 16 .. 128 size off the box's face
                eye = mid.copy()
                if k is not None:
                    eye[axis] += sign * (half[axis] + size * 2.0 ** k)
                    eye[(axis + 1) % 3] += 0.013 * size  # not exactly on an axis of the scene
                eye32 = tuple(float(x) for x in eye.astype(F32))
                ok = sc.shadow_origins_inside(eye32)
                said[(axis, sign, k)] = ok
                if not ok:
                    no += 1
                    continue
                yes += 1
                look = mid if k is not None else mid + size * np.array([0.1, -0.2, sign if axis == 2 else -sign])
                inside, n = origins_in_box(sc, d, eye32, tuple(look))
                rays += n
                assert inside == n, f"{config}: camera {eye32}: {n - inside} of {n} shadow origins outside the box"
    print(f"{config}: predicate yes for {yes} cameras, no for {no}; {rays} shadow origins checked")
    assert rays > 0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            assert not said[(axis, sign, 7)], f"{config}: a camera 128 scene sizes away qualifies"
    if config != "c5":  # (c5's floor mesh: the camera's height over each triangle's plane decides)
        assert said[(1, 1.0, -4)], f"{config}: a camera just above the scene does not qualify"


def test_predicate_says_no(esc):
    sc = esc.Scene.synthetic("c3", 120)
    lo, hi = box_of(sc)
    mid = 0.5 * (lo + hi)
    assert sc.shadow_origins_inside(mid.astype(F32))
    for bad in (np.inf, -np.inf, np.nan):
        for axis in range(3):
            eye = mid.astype(F32)
            eye[axis] = bad
            assert not sc.shadow_origins_inside(eye)
    # a camera in the plane of a large triangle: a grazing ray's t is rounding noise
    floor = {"vertex": np.array([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], F32),
             "face_index": np.array([[0, 1, 2], [0, 2, 3]]), "material": ol.WHITE}
    light = {"vertex": np.array([(-1, 4, 0), (1, 4, 0), (0, 4, -1)], F32), "face_index": np.array([[0, 1, 2]]),
             "material": ol.LIGHT_A}
    sph = np.array([(0, 1, 0, 0.5)], F32)
    mats = np.stack([ol.material13(ka=(0.5, 0.5, 0.5), kd=(0.5, 0.5, 0.5))])
    one = ol.scene_to_product(ol.scene_dict([dict(floor), dict(light)], sph, mats))
    assert one.shadow_origins_inside((0.5, 2.0, 0.3))
    assert not one.shadow_origins_inside((0.5, 0.0, 0.3))
    assert not one.shadow_origins_inside((0.5, 1e-7, 0.3))
    # two lights: quirk S3 starts the second light's ray wherever the first light's t left it
    light2 = {"vertex": np.array([(-1, 4, 2), (1, 4, 2), (0, 4, 1)], F32), "face_index": np.array([[0, 1, 2]]),
              "material": ol.LIGHT_A}
    two = ol.scene_to_product(ol.scene_dict([dict(floor), dict(light), light2], sph, mats))
    assert not two.shadow_origins_inside((0.5, 2.0, 0.3))
