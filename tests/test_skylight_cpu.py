"""Sky lighting (esc_skylight_rays and its companions): the C ABI, its binding, the viewer's --skylight parsing,
the conditions every case of tests/skylight_cases.py has to meet and the invariants of the restatement of
tests/skylight_lib.py -- all checked without a GPU (the library loads without one; only esc_context_create
needs a device).  Floats compare bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
import ambient_lib as al
import environment_lib as el
import esctp1raytracer_amd as esc
import skylight_cases as sc
import skylight_lib as sl
from esctp1raytracer_amd import _capi
from ray_oracle import F32, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esc_skylight_rays", "esc_render_skylight", "esc_add_light")
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")
SKY = "0.2,0.4,1/1,1,1/0.3,0.2,0.1"
K = sc.K
IDS = [f"{s}-{r}-{k}" for s, r, k in sc.CASES]


def test_skylight_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert len(_capi.SIGNATURES["esc_skylight_rays"][1]) == 12
    assert len(_capi.SIGNATURES["esc_render_skylight"][1]) == 9
    assert len(_capi.SIGNATURES["esc_add_light"][1]) == 6
    for m in ("skylight_rays", "skylight", "render_skylight", "add_light"):
        assert callable(getattr(esc.Renderer, m))
    # the options struct is the ambient one, unchanged
    assert [f[0] for f in _capi.esc_ambient_options._fields_] == \
        ["samples", "sets", "radius", "bias", "seed", "pixel_base", "flags"]
    assert C.sizeof(_capi.esc_ambient_options) == 32
    # the definition is in the header, after the ambient block, and the environment no longer disowns it
    assert header.index("int esc_last_ambient_stats(") < header.index("int esc_skylight_rays(")
    assert "sky_c = fl(s_c / float(K))" in header and "light_c = fl(kd_c * sky_c)" in header
    assert "Out of scope: the environment as a light source" not in header


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    opts = _capi.esc_ambient_options(8, 4, 1.0, 1e-4, 0, 0, 0)
    calls = {
        "esc_skylight_rays": lambda: lib.esc_skylight_rays(None, 0, None, None, C.byref(opts), None, None, None,
                                                           None, None, None, None),
        "esc_render_skylight": lambda: lib.esc_render_skylight(None, C.byref(cam), 4, 4, C.byref(opts), None, None,
                                                               None, None),
        "esc_add_light": lambda: lib.esc_add_light(None, 0, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)
    # null options next to a null context are still the context's error, not a crash
    assert lib.esc_skylight_rays(None, 0, None, None, None, None, None, None, None, None, None, None) == \
        _capi.ESC_ERR_INVALID
    assert lib.esc_render_skylight(None, None, 4, 4, None, None, None, None, None) == _capi.ESC_ERR_INVALID


@pytest.mark.parametrize("args,needs", [
    (["--ao", "8", "--ao-radius", "0.5", "--skylight"], "--sky"),
    (["--sky", SKY, "--skylight"], "--ao"),
    (["--sky", SKY, "--ao", "8", "--skylight"], "--ao"),
    (["--sky", SKY, "--ao", "8", "--ao-radius", "0.5", "--skylight", "--ispc"], "--ispc"),
    (["--sky", SKY, "--ao", "8", "--ao-radius", "0.5", "--skylight", "--gpus", "2"], "one GPU"),
], ids=["no-sky", "no-ao", "no-radius", "ispc", "gpus"])
def test_viewer_rejects_bad_skylight(args, needs, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--skylight" in r.stderr and needs in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()


def test_viewer_usage_names_skylight():
    r = subprocess.run([VIEWER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--skylight" in r.stdout


# ---- the conditions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ray_set,k", sc.CASES, ids=IDS)
def test_case_condition(name, ray_set, k):
    sc.check_condition(name, ray_set, k)


def test_open_samples_fall_on_all_six_faces():
    faces = sc.open_faces()
    print("open samples per face (+x, -x, +y, -y, +z, -z):", faces.tolist())
    assert (faces > 0).all(), faces


# ---- invariants of the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name,ray_set,k", sc.CASES, ids=IDS)
def test_restatement_invariants(name, ray_set, k):
    a = ac.want(name, ray_set, k)
    has = a["has"]
    # all ones: sky == vis in all three channels, light == fl(kd * vis); nothing for a miss
    one = sc.want(name, ray_set, k, "ones")
    for c in range(3):
        assert_same(one["sky"][has, c], a["vis"][has], f"{name} ones sky channel {c}")
    assert_same(one["light"][has], (one["kd"][has] * a["vis"][has, None]).astype(F32), name + " ones light")
    assert not one["sky"][~has].view(np.uint32).any() and not one["light"][~has].view(np.uint32).any()
    # all zeros: zero
    zero = sc.want(name, ray_set, k, "zeros")
    assert not zero["sky"].any() and not zero["light"].any()
    # one open sample: fl(env(w) / K) of that direction
    w = sc.want(name, ray_set, k)
    single = np.nonzero(a["count"][has] == 1)[0]
    sd = a["sample_d"].reshape(-1, K, 3)
    for j in single:
        kk = int(np.nonzero(w["open"][j])[0][0])
        e = el.env_ref(sc.cube(), sd[j, kk][None])[0]
        assert_same(w["sky"][has][j], (e / F32(K)).astype(F32), f"{name} ray with one open sample")
    # kd is the material's, and some hit is coloured
    assert w["kd"][has].any() and not w["kd"][~has].any()
    assert w["light"].shape == (len(has), 3) and w["light"].dtype == np.float32


def test_some_ray_has_exactly_one_open_sample():
    n = sum(int((ac.want(*c)["count"][ac.want(*c)["has"]] == 1).sum()) for c in sc.CASES)
    print("rays with exactly one open sample over all cases:", n)
    assert n >= 1


def test_miss_batch_is_zero():
    name = "CornellBox-Original"
    d, eye, _, _ = ac.scene(name)
    o = np.tile(np.array(eye, F32), (33, 1))
    away = np.tile(np.array([0, 0, 1], F32), (33, 1))  # out of the box's open front
    a = al.ambient(d, o, away, ac.table(), 1.0, 1e-3, 5, 0)
    assert not a["has"].any()
    w = sl.skylight(d, a, sc.cube(), K)
    assert w["sky"].shape == (33, 3) and not w["sky"].view(np.uint32).any() and not w["light"].view(np.uint32).any()
    assert (a["count"] == K).all() and (a["vis"] == 1).all()


def test_faces_cube_is_one_colour_per_face():
    name, ray_set, k = sc.CASES[0]
    a = ac.want(name, ray_set, k)
    w = sc.want(name, ray_set, k, "faces")
    parts = el.env_parts(sc.cube("faces"), a["sample_d"])
    ok = parts["defined"]
    assert_same(w["env"].reshape(-1, 3)[ok], sc.cube("faces")[parts["face"][ok], 0, 0], "R == 1")
