"""The HIP query, shading and frame kernels against exact arithmetic (tests/exact_lib.py) under the derived
rounding bounds the oracle is held to in test_exact_spheres_cpu.py: the same ray sets, the same assertions,
the same caps, no extra margin (the kernels are built -ffp-contract=off and the bounds cover every rounding
of the documented operation order).  Nothing of the oracle is imported.

The ray queries and shade do not walk the ESC_STAGE_BVH tree; "with the tree staged" means a frame rendered
through it first (with the triangle tree where `bvh_tree` asks for it), then the same queries on that context."""
import numpy as np
import pytest

import exact_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def _run_queries(r, s, exact):
    hit = r.intersect(s["o"], s["dirs"], s["tmax"], exact=exact)
    occ = r.occluded(s["o"], s["dirs"], s["tmax"], exact=exact)
    return xc.check_queries(s, hit, occ)


def _also(name, s, hit, got):
    if name == "ties":
        xc.check_lower_index(s, hit)
    if name == "surface":
        xc.check_surface(s, hit)
    if name == "tangent":
        xc.check_tangent(s, hit)
    if name == "tmax":
        under = s["mult"] > 0
        assert (hit["prim"][under] >= 0).all() and (hit["prim"][~under] < 0).all()
    assert got["hits"] > 0 and got["occluded"] > 0
    if name not in ("inside", "tangent"):
        assert got["misses"] > 0 and got["open"] > 0


@pytest.mark.parametrize("exact", [False, True], ids=["filtered", "exact"])
@pytest.mark.parametrize("name", list(xc.QUERY_SETS))
def test_queries_within_bounds(esc, r, name, exact):
    s = xc.QUERY_SETS[name]()
    r.upload(s["sc"])
    got = _run_queries(r, s, exact)
    _also(name, s, r.intersect(s["o"], s["dirs"], s["tmax"], exact=exact), got)
    if s["tmax"] is not None:  # and without the bound
        free = dict(s, tmax=None, ref=dict(s["ref"], hit=xc.xl.closest_hit(s["ref"]["P"], s["o"], s["dirs"]),
                                           occ=xc.xl.occluded(s["ref"]["P"], s["o"], s["dirs"])),
                    cap=1.0 if name.startswith("shadow/") else 0.05, name=name + " (no tmax)")
        _run_queries(r, free, exact)


@pytest.mark.parametrize("exact", [False, True], ids=["filtered", "exact"])
def test_far_bounds_still_hold(esc, r, exact):
    s = xc.far_set()
    r.upload(s["sc"])
    assert xc.check_far(s, r.intersect(s["o"], s["dirs"], exact=exact)) > 0


def _black_pin(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_sphere_pins.json")) as f:
        return json.load(f)["black/" + name]


@pytest.mark.parametrize("exact", [False, True], ids=["filtered", "exact"])
@pytest.mark.parametrize("name", ["camera/c2", "camera/c3", "camera/c4", "inside"])
def test_shade_within_bounds(esc, r, name, exact):
    s = xc.QUERY_SETS[name]()
    r.upload(s["sc"])
    got = r.shade(s["o"], s["dirs"], face_mode=esc.ESC_FACE_FIXED, exact=exact)
    xc.check_colours(s, got["rgb"], black_pin=_black_pin(name))
    xc.check_queries(s, got, r.occluded(s["o"], s["dirs"], exact=exact))  # shade's t, geom, prim are intersect's


@pytest.mark.parametrize("config", ["c2", "c3", "c4"])
def test_frames_within_bounds(esc, r, config, bvh_tree):
    s = xc.camera_set(config)
    r.upload(s["sc"])
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, xc.W, xc.H)
    for stage in (esc.ESC_STAGE_AUTO, esc.ESC_STAGE_BVH):
        img = r.render(cam, xc.W, xc.H, stage=stage)
        xc.check_colours(s, img.reshape(-1, 3), black_pin=_black_pin("camera/" + config))
    # the tree is staged now: the camera and rim sets once more on this context
    _run_queries(r, s, False)
    if config == "c4":
        rim = xc.rim_set()
        _also("rim", rim, r.intersect(rim["o"], rim["dirs"]), _run_queries(r, rim, False))
