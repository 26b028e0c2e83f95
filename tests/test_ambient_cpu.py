"""Ambient occlusion (esc_ambient_rays and its companions): the C ABI, its binding, the viewer's --ao parsing,
the host-side table generator, the restatement's tangent frame and the condition every case of
tests/ambient_cases.py has to meet -- all checked without a GPU (the library loads without one; only
esc_context_create needs a device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
import ambient_lib as al
import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi
from ray_oracle import F32, dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esc_set_ambient_table", "esc_ambient_cosine_table", "esc_ambient_rays", "esc_render_ambient",
           "esc_modulate", "esc_last_ambient_stats")
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")


def test_ambient_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [f[0] for f in _capi.esc_ambient_options._fields_] == \
        ["samples", "sets", "radius", "bias", "seed", "pixel_base", "flags"]
    assert [f[0] for f in _capi.esc_ambient_stats._fields_] == \
        ["rays", "hit_rays", "samples", "occluded_samples", "exact_rays", "exact_tests"]
    for m in ("set_ambient_table", "ambient_rays", "ambient", "render_ambient", "modulate", "ambient_stats"):
        assert callable(getattr(esc.Renderer, m))
    assert callable(esc.ambient_table)


def test_ambient_struct_layouts_match_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>\n#include "esctp1_rt.h"\n']
    for name in ("esc_ambient_options", "esc_ambient_stats"):
        st = getattr(_capi, name)
        lines.append(f"_Static_assert(sizeof({name}) == {C.sizeof(st)}, \"size of {name}\");\n")
        lines += [f"_Static_assert(offsetof({name}, {n}) == {getattr(st, n).offset}, \"{name}.{n}\");\n"
                  for n, _ in st._fields_]
    # the structs that were there before keep their layout
    for name in ("esc_shade_stats", "esc_render_options", "esc_adaptive_options", "esc_adaptive_stats",
                 "esc_trace_options"):
        lines.append(f"_Static_assert(sizeof({name}) == {C.sizeof(getattr(_capi, name))}, \"{name}\");\n")
    lines.append("int main(void) { return 0; }\n")
    src = tmp_path / "layout.c"
    src.write_text("".join(lines))
    r = subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    opts = _capi.esc_ambient_options(8, 4, 1.0, 1e-4, 0, 0, 0)
    table = np.zeros((4, 8, 3), np.float32)
    tp = table.ctypes.data_as(C.POINTER(C.c_float))
    calls = {
        "esc_set_ambient_table": lambda: lib.esc_set_ambient_table(None, 4, 8, tp),
        "esc_ambient_rays": lambda: lib.esc_ambient_rays(None, 0, None, None, C.byref(opts), None, None, None, None,
                                                         None),
        "esc_render_ambient": lambda: lib.esc_render_ambient(None, C.byref(cam), 4, 4, C.byref(opts), None, None),
        "esc_modulate": lambda: lib.esc_modulate(None, 0, None, None, None, None),
        "esc_last_ambient_stats": lambda: lib.esc_last_ambient_stats(None, C.byref(_capi.esc_ambient_stats())),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)
    # null options next to a null context are still the context's error, not a crash
    assert lib.esc_ambient_rays(None, 0, None, None, None, None, None, None, None, None) == _capi.ESC_ERR_INVALID
    assert lib.esc_render_ambient(None, None, 4, 4, None, None, None) == _capi.ESC_ERR_INVALID


@pytest.mark.parametrize("args", [["--ao", "8"], ["--ao", "8", "--ao-radius", "0.5", "--gpus", "2"],
                                  ["--ao", "0", "--ao-radius", "0.5"], ["--ao", "65", "--ao-radius", "0.5"],
                                  ["--ao", "8x", "--ao-radius", "0.5"], ["--ao", "8", "--ao-radius", "0"],
                                  ["--ao", "8", "--ao-radius", "-1"], ["--ao", "8", "--ao-radius", "nan"],
                                  ["--ao", "8", "--ao-radius", "inf"], ["--ao", "8", "--ao-radius", "0.5", "--ao-sets", "0"],
                                  ["--ao", "8", "--ao-radius", "0.5", "--ao-sets", "65"],
                                  ["--ao", "8", "--ao-radius", "0.5", "--ao-bias", "-1e-3"],
                                  ["--ao", "8", "--ao-radius", "0.5", "--ao-bias", "nan"],
                                  ["--ao", "8", "--ao-radius", "0.5", "--ao-seed", "x"],
                                  ["--ao-radius", "0.5"], ["--ao-sets", "4"], ["--ao", "8", "--ao-radius", "0.5", "--ispc"]],
                         ids=["no-radius", "gpus", "zero", "too-many", "trailing", "radius-zero", "radius-negative",
                              "radius-nan", "radius-inf", "sets-zero", "sets-too-many", "bias-negative", "bias-nan",
                              "seed", "radius-alone", "sets-alone", "ispc"])
def test_viewer_rejects_bad_ao(args, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--ao" in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()


def test_generator_properties():
    t = esc.ambient_table(64, 64, 5)
    assert t.shape == (64, 64, 3) and t.dtype == np.float32
    assert esc.ambient_table(64, 64, 5).tobytes() == t.tobytes()  # deterministic in (sets, samples, seed)
    assert esc.ambient_table(64, 64, 6).tobytes() != t.tobytes()
    assert esc.ambient_table(64, 32, 5).tobytes() != np.ascontiguousarray(t[:, :32]).tobytes()
    assert esc.ambient_table(32, 64, 5).tobytes() != np.ascontiguousarray(t[:32]).tobytes()
    assert np.isfinite(t).all()
    assert (t[..., 2] > 0).all()
    n2 = (t.astype(np.float64) ** 2).sum(-1)
    print("largest | |v|^2 - 1 |:", np.abs(n2 - 1).max(), " mean z:", t[..., 2].astype(np.float64).mean())
    assert np.abs(n2 - 1).max() <= 1e-6
    for a in range(64):  # sets differ
        for b in range(a):
            assert t[a].tobytes() != t[b].tobytes(), (a, b)
    # cosine-weighted: E z = 2/3, sigma 0.236 per sample, 0.0037 over 4096: 0.02 is beyond 5 sigma
    assert abs(t[..., 2].astype(np.float64).mean() - 2.0 / 3.0) <= 0.02
    # the azimuth is uniform: by symmetry E x = E y = 0 (sigma 0.5 per sample, 0.0078 over 4096)
    assert abs(t[..., 0].astype(np.float64).mean()) <= 0.04 and abs(t[..., 1].astype(np.float64).mean()) <= 0.04
    lib = _capi.load()
    buf = np.zeros(3, np.float32)
    for sets, samples in ((0, 8), (8, 0), (65, 8), (8, 65), (-1, 8)):
        assert lib.esc_ambient_cosine_table(sets, samples, 0, buf.ctypes.data_as(C.POINTER(C.c_float))) == \
            _capi.ESC_ERR_INVALID
        assert "esc_ambient_cosine_table" in lib.esc_last_error().decode()
    assert lib.esc_ambient_cosine_table(4, 8, 0, None) == _capi.ESC_ERR_INVALID


@pytest.mark.parametrize("name", ac.SCENES)
def test_restatement_frame_is_orthonormal(name):
    worst = 0.0
    for ray_set in ac.RAY_SETS:
        o, dirs = ac.rays(name, ray_set)
        _, has, Nf, _, T, B = al.hit_frames(ac.scene(name)[0], o, dirs, 1e-4)
        assert has.any()
        T, B, Nf = (v[has].astype(np.float64) for v in (T, B, Nf))
        for what, v in (("T.Nf", (T * Nf).sum(-1)), ("T.B", (T * B).sum(-1)), ("|T|^2 - 1", (T * T).sum(-1) - 1),
                        ("B.Nf", (B * Nf).sum(-1)), ("|B|^2 - 1", (B * B).sum(-1) - 1)):
            worst = max(worst, float(np.abs(v).max()))
            assert np.abs(v).max() <= 1e-6, (name, ray_set, what, np.abs(v).max())
    print(name, "worst deviation of the frame:", worst)


def test_frame_at_the_poles():
    # Nf = (0, 0, +-1) and its neighbourhood: the denominator sg + Nf.z stays at magnitude >= 1
    Nf = np.array([[0, 0, 1], [0, 0, -1], [1, 0, -0.0], [1, 0, 0.0], [1e-20, -1e-20, -1], [0.6, 0, -0.8]], F32)
    T, B = al.frame(Nf)
    assert np.isfinite(T).all() and np.isfinite(B).all()
    for v in (dot(T, Nf), dot(T, B), dot(B, Nf)):
        assert np.abs(v).max() <= 1e-6
    # right-handed: T x B = Nf
    assert np.abs(np.cross(T.astype(np.float64), B.astype(np.float64)) - Nf).max() <= 1e-6


@pytest.mark.parametrize("name,ray_set,k", ac.CASES, ids=[f"{s}-{r}-{k}" for s, r, k in ac.CASES])
def test_case_condition(name, ray_set, k):
    ac.check_condition(name, ray_set, k)


def test_restatement_samples_are_what_it_says():
    """the sample rays the restatement hands out are the rays it counted: occlusion asked again per ray"""
    from ray_oracle import ref_queries
    name, ray_set, k = "CornellBox-Sphere", "surface", 1
    w = ac.want(name, ray_set, k)
    radius, _ = ac.setting(name, k)
    K = ac.TABLE_SAMPLES
    nh = int(w["has"].sum())
    assert w["sample_o"].shape == (nh * K, 3) and w["sample_d"].shape == (nh * K, 3)
    _, occ = ref_queries(ac.scene(name)[0], w["sample_o"], w["sample_d"], np.full(nh * K, radius, F32))
    assert np.array_equal(K - occ.reshape(nh, K).sum(1), w["count"][w["has"]])
    assert np.array_equal(w["count"][~w["has"]], np.full(int((~w["has"]).sum()), K))
    assert np.array_equal(w["vis"].view(np.uint32), (w["count"].astype(F32) / F32(K)).astype(F32).view(np.uint32))
    d2 = (w["sample_d"].astype(np.float64) ** 2).sum(-1)
    assert np.abs(d2 - 1).max() <= 7.5 * 2.0 ** -24, "a sample direction outside precondition (c) of the filtered sweep"
