"""Adaptive supersampling (esc_render_adaptive / esc_last_adaptive_stats): the C ABI, its binding and the
viewer's --adaptive parsing, checked without a GPU (the library loads without one; only
esc_context_create needs a device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esc_render_adaptive", "esc_last_adaptive_stats")
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")


def test_adaptive_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [f[0] for f in _capi.esc_adaptive_options._fields_] == ["spp", "threshold", "band_rows", "reserved"]
    assert [f[0] for f in _capi.esc_adaptive_stats._fields_] == \
        ["pixels", "refined_pixels", "samples", "hit_rays", "shadow_rays", "exact_rays", "exact_tests"]
    for m in ("render_adaptive", "adaptive_stats"):
        assert callable(getattr(esc.Renderer, m))


def test_adaptive_struct_layouts_match_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>\n#include "esctp1_rt.h"\n']
    for name in ("esc_adaptive_options", "esc_adaptive_stats"):
        st = getattr(_capi, name)
        lines.append(f"_Static_assert(sizeof({name}) == {C.sizeof(st)}, \"size of {name}\");\n")
        lines += [f"_Static_assert(offsetof({name}, {n}) == {getattr(st, n).offset}, \"{name}.{n}\");\n"
                  for n, _ in st._fields_]
    # the structs that were there before keep their layout
    lines.append(f"_Static_assert(sizeof(esc_shade_stats) == {C.sizeof(_capi.esc_shade_stats)}, \"s\");\n")
    lines.append(f"_Static_assert(sizeof(esc_render_options) == {C.sizeof(_capi.esc_render_options)}, \"o\");\n")
    lines.append("int main(void) { return 0; }\n")
    src = tmp_path / "layout.c"
    src.write_text("".join(lines))
    r = subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    opts = _capi.esc_render_options()
    aopts = _capi.esc_adaptive_options(4, 0.05, 0, 0)
    calls = {
        "esc_render_adaptive": lambda: lib.esc_render_adaptive(None, C.byref(cam), 4, 4, C.byref(opts),
                                                               C.byref(aopts), None, None, None),
        "esc_last_adaptive_stats": lambda: lib.esc_last_adaptive_stats(None, C.byref(_capi.esc_adaptive_stats())),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)
    # a null options pointer next to a null context is still the context's error, not a crash
    assert lib.esc_render_adaptive(None, C.byref(cam), 4, 4, C.byref(opts), None, None, None, None) == \
        _capi.ESC_ERR_INVALID


@pytest.mark.parametrize("args", [["--spp", "4", "--adaptive", "-1"], ["--spp", "4", "--adaptive", "nan"],
                                  ["--spp", "4", "--adaptive", "inf"], ["--spp", "4", "--adaptive", "0.1x"],
                                  ["--adaptive", "0.1", "--bounces", "2"],
                                  ["--spp", "4", "--adaptive", "0.1", "--bounces", "2"],
                                  ["--adaptive", "0.1"]],
                         ids=["negative", "nan", "inf", "trailing", "bounces", "spp-bounces", "no-spp"])
def test_viewer_rejects_bad_adaptive(args, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--adaptive" in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()
