"""Temporal accumulation (esc_temporal_accumulate): the C ABI, its binding, the viewer's --temporal parsing, the
conditions the cases of tests/temporal_cases.py have to meet and the invariants of the restatement of
tests/temporal_lib.py -- all checked without a GPU (the library loads without one; only esc_context_create
needs a device).  Floats compare bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import esctp1raytracer_amd as esc
import temporal_cases as tc
import temporal_lib as tl
from esctp1raytracer_amd import _capi
from ray_oracle import F32, FLT_MAX, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")


def header():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        return f.read()


def struct_fields(text, name):
    """the member names of `typedef struct name { ... } name;` in the header, arrays with their length"""
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:  # `const int32_t *geom, *prim` declares two
            first, *more = decl.split(",")
            names += [re.search(r"(\w+(?:\[\d+\])?)\s*$", first).group(1)] + [m.strip(" *") for m in more]
    return names


def test_temporal_entry_points_declared_and_bound():
    text = header()
    lib = _capi.load()
    for name, nargs in (("esc_temporal_accumulate", 13), ("esc_last_temporal_stats", 2)):
        assert re.search(r"\bint " + name + r"\(", text), name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
        assert len(_capi.SIGNATURES[name][1]) == nargs
    fields = {"esc_guides": ["normal", "position", "geom", "prim"],
              "esc_temporal_options": ["taps", "max_history", "normal_cos", "plane_dist", "same_object", "reserved[3]"],
              "esc_temporal_stats": ["pixels", "hit_pixels", "reused_pixels", "taps_tested", "taps_accepted"]}
    sizes = {"esc_guides": 4 * C.sizeof(C.c_void_p), "esc_temporal_options": 32, "esc_temporal_stats": 40}
    for name, want in fields.items():
        assert struct_fields(text, name) == want, name
        cls = getattr(_capi, name)
        assert [f[0] for f in cls._fields_] == [w.split("[")[0] for w in want], name
        assert C.sizeof(cls) == sizes[name], name
    for m in ("temporal_accumulate", "temporal_stats"):
        assert callable(getattr(esc.Renderer, m))
    for m in ("push", "reset"):
        assert callable(getattr(esc.TemporalAccumulator, m))
    assert isinstance(esc.TemporalAccumulator.history_n, property)
    # the definition is in the header in full
    for piece in ("c   = cross(V, v);          det = dot(Hh, c)",
                  "x   = dot(A, c) / det;      y = dot(Hh, cross(A, v)) / det;      z = dot(Hh, cross(V, A)) / det",
                  "fx  = (-x) * float(W - 1);  fy = (-y) * float(H - 1)",
                  "valid = z > 0 && fx >= -1.f && fx <= float(W) && fy >= -1.f && fy <= float(H)",
                  "taps == 1:  x0 = floorf(fx + 0.5f);  y0 = floorf(fy + 0.5f)",
                  "k = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay)",
                  "skip unless history_n[q] >= 1",
                  "acc_c = fl(acc_c + fl(k * history[q]_c));   ws = fl(ws + k);   n = min(n, history_n[q])",
                  "m = min(n, M - 1) + 1;   alpha = 1.f / float(m)",
                  "out[p]_c = fl(hc + fl(fl(current[p]_c - hc) * alpha))",
                  "Out of scope: motion vectors"):
        assert piece in text, piece


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    o = _capi.esc_temporal_options(4, 32, 0.9, 0.1, 1)
    g = _capi.esc_guides()
    cam = _capi.esc_camera()
    st = _capi.esc_temporal_stats()
    calls = {
        "esc_temporal_accumulate": lambda: lib.esc_temporal_accumulate(
            None, C.byref(cam), 4, 4, 1, None, C.byref(g), None, None, C.byref(g), C.byref(o), None, None),
        "esc_last_temporal_stats": lambda: lib.esc_last_temporal_stats(None, C.byref(st)),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)
    assert lib.esc_temporal_accumulate(None, None, 4, 4, 1, None, None, None, None, None, None, None,
                                       None) == _capi.ESC_ERR_INVALID


# ---- the conditions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", tc.TRACED, ids=tc.TRACED_IDS)
def test_traced_case_condition(name, which):
    tc.check_traced(name, which)


def test_every_stop_rejects_over_the_traced_cases():
    on, off = tc.traced_rejects(True), tc.traced_rejects(False)
    print("rejected taps with same_object:", on, "without:", off)
    assert all(on[s] >= 1 for s in tl.STOPS), on
    assert off["object"] == 0 and off["normal"] >= 1 and off["plane"] >= 1, off
    # "missing" needs sky in the previous frame, "history" the zeros planted in history_n
    assert any(not tc.frame(n, w, tc.SEEDS[1])["guides"]["has"].all() for n, w in tc.TRACED)


def test_every_stop_rejects_over_the_synthetic_cases():
    tc.check_synthetic()


def test_synthetic_data_is_what_it_claims():
    g = tc.synthetic(130, 70)
    hn = g["history_n"]
    for v in (0, 1, tc.MAX_HISTORY, tc.INT32_MAX, -1, -tc.INT32_MAX - 1):
        assert (hn == v).any(), v
    for k in range(8):
        assert (g["kind"] == k).any(), k
    assert np.isnan(g["cur"]["position"]).any() and np.isinf(g["cur"]["position"]).any()
    assert np.isnan(g["cur"]["normal"]).any() and np.isinf(g["cur"]["normal"]).any()
    assert np.isnan(g["prev"]["normal"]).any() and np.isnan(g["prev"]["position"]).any()
    for ch in (1, 3):
        for what in ("current", "history"):
            a = g[f"{what}{ch}"]
            assert np.isnan(a).any() and np.isinf(a).any(), (what, ch)
    assert ((g["cur"]["geom"] < 0) & (g["cur"]["prim"] >= 0)).any(), "no spheres"
    # a NaN or infinite value in an accepted history tap or in current reaches the output, as written
    out, _, st = tc.synthetic_want(130, 70)
    assert (~np.isfinite(out)).sum() > (~np.isfinite(g["current1"])).sum() - 40


# ---- invariants of the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", tc.SYNTHETIC, ids=tc.SYNTHETIC_IDS)
def test_restatement_invariants(W, H):
    g = tc.synthetic(W, H)
    hit = (g["cur"]["geom"] >= 0) | (g["cur"]["prim"] >= 0)
    kw = dict(max_history=tc.MAX_HISTORY, normal_cos=tc.NORMAL_COS, plane_dist=tc.SYN_PLANE)
    for ch in (1, 3):
        cur, hist = g[f"current{ch}"], g[f"history{ch}"]
        for taps in (1, 4):
            # a first frame: all-zero history_n gives out == current and n = hit
            out, n, st = tl.accumulate(cur, g["cur"], g["prev_cam"], hist, np.zeros((H, W), np.int32), g["prev"],
                                       taps, **kw)
            assert out.tobytes() == cur.tobytes() and np.array_equal(n, hit.astype(np.int32))
            assert st["taps_accepted"] == 0 and st["reused_pixels"] == 0
            assert st["missing"] + st["history"] == st["taps_tested"]
            # a constant history equal to current stays constant, bit for bit: any value under one tap of weight
            # 1; under four taps the values whose products with the weights are exact (powers of two)
            for v in (F32(0.3), F32(1e-40), F32(-7.77), F32(3.0e38)) if taps == 1 else (F32(1), F32(0.5), F32(-4)):
                const = np.full(cur.shape, v, F32)
                out, n, st = tl.accumulate(const, g["cur"], g["prev_cam"], const, g["history_n"], g["prev"], taps, **kw)
                assert_same(out, const, f"{W}x{H} taps {taps} constant {v}")
                assert st["reused_pixels"] > 0 or W * H <= 4
            # pixels without a hit are copied and carry no history; the stats add up
            out, n, st = tc.synthetic_want(W, H, ch, taps)
            assert out[~hit].tobytes() == cur[~hit].tobytes() and (n[~hit] == 0).all()
            assert ((n[hit] >= 1) & (n[hit] <= tc.MAX_HISTORY)).all()
            assert st["taps_tested"] == st["taps_accepted"] + sum(st[s] for s in tl.STOPS)
            assert st["pixels"] == W * H and st["hit_pixels"] == int(hit.sum())
            assert st["reused_pixels"] <= st["taps_accepted"] <= st["taps_tested"] <= taps * st["hit_pixels"]


def test_still_camera_is_the_running_mean_then_the_exponential_average():
    """same camera, taps 1: after pushes of I_0 .. I_f, n = min(f + 1, M) and the value is the recurrence
    a_f = a_{f-1} + (I_f - a_{f-1}) * (1 / n_f)"""
    name = "CornellBox-Sphere"
    cam = tc.camera(name)
    g = tc.frame(name, "same", tc.SEEDS[0])["guides"]
    hit = g["has"].reshape(tc.H, tc.W)
    rng = np.random.default_rng(3)
    imgs = [rng.random((tc.H, tc.W)).astype(F32) for _ in range(7)]
    for M in (1000, 3):
        acc, n = np.zeros((tc.H, tc.W), F32), np.zeros((tc.H, tc.W), np.int32)
        want = None
        for f, img in enumerate(imgs):
            acc, n, st = tl.accumulate(img, g, cam, acc, n, g, 1, M, tc.NORMAL_COS, tc.traced_plane(name))
            m = min(f + 1, M)
            want = img if f == 0 else (want + ((img - want).astype(F32) * (F32(1) / F32(m))).astype(F32)).astype(F32)
            assert (n[hit] == m).all() and (n[~hit] == 0).all(), (M, f)
            assert_same(acc[hit], want[hit], f"M {M} frame {f}")
            assert st["reused_pixels"] == (0 if f == 0 else int(hit.sum()))


def test_tap_order_is_another_sum():
    W, H = 33, 19
    g = tc.synthetic(W, H)
    a, na, sa = tc.synthetic_want(W, H, 1, 4)
    b, nb, sb = tc.synthetic_want(W, H, 1, 4, reverse=True)
    fin = np.isfinite(a) & np.isfinite(b)
    assert sa == sb and np.array_equal(na, nb) and (a.view(np.uint32) != b.view(np.uint32))[fin].any()


def test_stops_off_accept_every_tested_tap_with_history():
    W, H = 65, 9
    g = tc.synthetic(W, H)
    prev = dict(g["prev"], normal=np.nan_to_num(g["prev"]["normal"]), position=np.nan_to_num(g["prev"]["position"], posinf=0),
                geom=np.zeros((H, W), np.int32))
    cur = dict(g["cur"], normal=np.nan_to_num(g["cur"]["normal"], neginf=0))
    for pd in (FLT_MAX, np.inf):
        _, _, st = tl.accumulate(g["current1"], cur, g["prev_cam"], g["history1"], np.ones((H, W), np.int32), prev, 4,
                                 tc.MAX_HISTORY, -np.inf, pd, same_object=False)
        assert st["taps_accepted"] == st["taps_tested"] > 0, st


# ---- the viewer --------------------------------------------------------------------------------------------
AO = ["--ao", "8", "--ao-radius", "0.5"]


@pytest.mark.parametrize("args,needs", [
    (["--temporal", "3"], "--temporal needs --ao"),
    (AO + ["--temporal-step", "0.1,0,0"], "--temporal-step, --temporal-max and --temporal-taps need --temporal"),
    (AO + ["--temporal-max", "8"], "--temporal-step, --temporal-max and --temporal-taps need --temporal"),
    (AO + ["--temporal-taps", "4"], "--temporal-step, --temporal-max and --temporal-taps need --temporal"),
    (AO + ["--temporal", "0"], "--temporal must be a whole number from 1 to 64, got 0"),
    (AO + ["--temporal", "65"], "--temporal must be a whole number from 1 to 64, got 65"),
    (AO + ["--temporal", "3", "--temporal-max", "0"], "--temporal-max must be a whole number from 1 to 65536, got 0"),
    (AO + ["--temporal", "3", "--temporal-max", "65537"],
     "--temporal-max must be a whole number from 1 to 65536, got 65537"),
    (AO + ["--temporal", "3", "--temporal-taps", "2"], "--temporal-taps must be 1 or 4, got 2"),
    (AO + ["--temporal", "3", "--temporal-step", "0.1,nan,0"],
     "--temporal-step needs x,y,z with three finite numbers, got 0.1,nan,0"),
    (AO + ["--temporal", "3", "--temporal-step", "0.1,0"],
     "--temporal-step needs x,y,z with three finite numbers, got 0.1,0"),
    (AO + ["--temporal", "3", "--ao-seed", "5"], "--temporal seeds frame f with f: not with --ao-seed"),
    (AO + ["--temporal", "3", "--denoise-plane", "-1"], "--denoise-plane must be a finite number >= 0, got -1"),
], ids=["no-ao", "step-alone", "max-alone", "taps-alone", "zero", "sixty-five", "max-zero", "max-large", "taps-two",
        "step-nan", "step-short", "ao-seed", "negative-plane"])
def test_viewer_rejects_bad_temporal(args, needs, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert needs in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()


def test_viewer_usage_names_temporal():
    r = subprocess.run([VIEWER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--temporal N", "--temporal-step", "--temporal-max", "--temporal-taps"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("name", tc.SEQ_SCENES)
def test_sequence_condition(name):
    tc.check_sequence(name)
