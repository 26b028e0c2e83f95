"""The G-buffer of rays and frames (esc_gbuffer_rays / esc_render_gbuffer): the C ABI, its binding and the
invariants of the restatement filter_lib.gbuffer -- all checked without a GPU.  Floats compare bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ambient_cases as ac
import esctp1raytracer_amd as esc
import filter_cases as fc
from esctp1raytracer_amd import _capi
from ray_oracle import F32, FLT_MAX, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gbuffer_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        text = f.read()
    lib = _capi.load()
    for name, nargs in (("esc_gbuffer_rays", 11), ("esc_render_gbuffer", 11), ("esc_last_gbuffer_stats", 2)):
        assert re.search(r"\bint " + name + r"\(", text), name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
        assert len(_capi.SIGNATURES[name][1]) == nargs
    body = re.search(r"typedef struct esc_gbuffer_stats \{(.*?)\} esc_gbuffer_stats;", text, re.S).group(1)
    names = re.findall(r"uint64_t (\w+);", body)
    assert names == ["rays", "hit_rays", "exact_rays", "exact_tests"]
    assert [f[0] for f in _capi.esc_gbuffer_stats._fields_] == names and C.sizeof(_capi.esc_gbuffer_stats) == 32
    for m in ("gbuffer_rays", "gbuffer", "render_gbuffer", "gbuffer_stats"):
        assert callable(getattr(esc.Renderer, m))
    assert "position = fl(o + fl(d*t))" in text and "NOT flipped towards the ray" in text
    assert text.index("int esc_add_light(") < text.index("int esc_gbuffer_rays(") < text.index("int esc_filter_guided(")


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    st = _capi.esc_gbuffer_stats()
    calls = {
        "esc_gbuffer_rays": lambda: lib.esc_gbuffer_rays(None, 0, None, None, 0, None, None, None, None, None, None),
        "esc_render_gbuffer": lambda: lib.esc_render_gbuffer(None, C.byref(cam), 4, 4, 0, None, None, None, None, None,
                                                             None),
        "esc_last_gbuffer_stats": lambda: lib.esc_last_gbuffer_stats(None, C.byref(st)),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)


@pytest.mark.parametrize("name", ac.SCENES)
def test_restatement_invariants(name):
    g = fc.traced_guides(name)
    a = ac.want(name, "frame", 1)
    has = g["has"]
    # the hit is the ambient restatement's
    assert np.array_equal(has, a["has"]) and g["t"].tobytes() == a["t"].tobytes()
    assert np.array_equal(g["geom"], a["geom"]) and np.array_equal(g["prim"], a["prim"])
    # a miss: +0 everywhere, t = FLT_MAX, ids -1
    for key in ("normal", "position", "albedo"):
        assert g[key].shape == (len(has), 3) and g[key].dtype == np.float32
        assert not g[key][~has].view(np.uint32).any(), key
    assert (g["t"][~has] == FLT_MAX).all() and (g["geom"][~has] == -1).all() and (g["prim"][~has] == -1).all()
    # a hit: a unit normal (to rounding), the position o + d*t, some colour
    ln = np.sqrt((g["normal"][has].astype(np.float64) ** 2).sum(1))
    assert np.abs(ln - 1).max() < 1e-6
    o, d = ac.rays(name, "frame")
    assert_same(g["position"][has], ((o + (d * g["t"][:, None]).astype(F32)).astype(F32))[has], name + " position")
    assert g["albedo"][has].any()
    # the normal is not flipped towards the ray: in some scene it points along it
    print(name, "hits whose normal points along the ray:", int(((g["normal"] * d).sum(1) > 0)[has].sum()))
