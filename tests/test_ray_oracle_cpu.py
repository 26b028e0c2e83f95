"""tests/ray_oracle.py and tests/ray_cases.py give what the test modules' own restatements gave before the
two libraries existed: sha256 digests of their results, recorded then in tests/golden/ray_oracle_pins.json,
are recomputed here (no GPU).  The mirror cases go through oracle_trace with transmission off."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import random_scenes as rs
import ray_cases as rc
import ray_oracle as ro

F32 = np.float32
with open(os.path.join(ol.GOLDEN_DIR, "ray_oracle_pins.json")) as f:
    PINS = json.load(f)


def digest(*parts):
    """fp32 by their bits (every NaN as one), bool as it is, every other number as int64"""
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        if a.dtype == F32:
            a = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).astype(np.uint32)
        elif a.dtype != np.bool_:
            a = a.astype(np.int64)
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name,setting", [("mirror_block", (1, 0.0, True)), ("cornell_mixed", (2, 1e-4, True)),
                                          ("rand9", (5, 1e-4, True))])
def test_mirror_cases(name, setting):
    depth, bias, shadows = setting
    assert (name, *setting) in rc.TRACE_CASES
    d, o, a = rc.trace_case_rays(name)
    w = ro.oracle_trace(d, o, a, depth, float(F32(bias)), ro.OFF, shadows=shadows)
    assert digest(w["dirs"], w["rgb"], w["usable"], w["depth_rays"], w["hit_rays0"]) == PINS["mirror"][name]
    assert ro.stats_of(w) == {"refracted": 0, "fresnel_reflected": 0, "total_internal": 0}


@pytest.mark.parametrize("name,mode", [("slab", ro.REFRACT), ("slab", ro.FRESNEL), ("slab", ro.OFF),
                                       ("sheet_below", ro.REFRACT), ("sheet_below", ro.FRESNEL)])
def test_transmission_cases(name, mode):
    depth, bias, shadows = rc.TRANSMISSION_SETTINGS[0]
    d, o, a = rc.transmission_case_rays(name)
    w = ro.oracle_trace(d, o, a, depth, float(F32(bias)), mode, shadows=shadows)
    got = digest(w["dirs"], w["rgb"], w["usable"], w["depth_rays"], w["refracted"], w["fresnel_reflected"],
                 w["total_internal"])
    assert got == PINS["transmission"][f"{name}/{ro.MODE_NAME[mode]}"]


def test_ray_colours_and_ref_queries():
    d = rs.random_scene(9)[0]
    shade, query = [], []
    for o, a in rc.ray_sets(d, np.random.default_rng(9), 64).values():
        dirs, rgb = ro.ray_colours(d, o, a)
        hit, occ = ro.ref_queries(d, o, dirs)
        shade += [dirs, rgb]
        query += [hit["t"], hit["geom"], hit["prim"], hit["uv"], occ]
    assert digest(*shade) == PINS["oracle_shade"]
    assert digest(*query) == PINS["ref_queries"]


def test_reflect_is_the_mirror_branch_of_bounce():
    rng = np.random.default_rng(3)
    n = 512
    o, dr, N = (rng.standard_normal((n, 3)).astype(F32) for _ in range(3))
    dr, N = ro.normalize(dr), ro.normalize(N)
    N[::9] = -N[::9] * F32(1.2)  # main.cpp's normals are not all unit vectors
    t0 = rng.uniform(0.1, 5.0, n).astype(F32)
    one = np.ones((n, 3), F32)
    opaque = np.tile(np.array([0, 0, 0, 1], F32), (n, 1))
    for bias in (0.0, 1e-4, 0.5):
        o2, x, d2 = ro.reflect(o, dr, t0, N, bias)
        go, bo, bx, _, what = ro.bounce(o, dr, t0, N, one, opaque, one, ro.OFF, 0, None, bias)
        assert go.all() and not what.any() and (dr * N).sum(1).min() < 0 < (dr * N).sum(1).max()
        assert ro.same_bits(o2, bo).all() and ro.same_bits(x, bx).all() and ro.same_bits(d2, ro.normalize(bx)).all()
