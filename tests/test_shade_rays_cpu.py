"""Shading of caller-supplied rays, camera rays and supersampled frames (esc_camera_rays /
esc_shade_rays / esc_render_supersampled / esc_last_shade_stats): the C ABI, its binding and the
viewer's --spp parsing, checked without a GPU (the library loads without one; only
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
ENTRIES = ("esc_camera_rays", "esc_shade_rays", "esc_render_supersampled", "esc_last_shade_stats")
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")


def _last_error(lib):
    return lib.esc_last_error().decode()


def test_shade_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [f[0] for f in _capi.esc_shade_stats._fields_] == \
        ["rays", "hit_rays", "shadow_rays", "exact_rays", "exact_tests"]
    assert [f[0] for f in _capi.esc_query_stats._fields_] == ["rays", "exact_rays", "exact_tests"]
    for m in ("camera_rays", "shade_rays", "shade", "render_supersampled", "shade_stats"):
        assert callable(getattr(esc.Renderer, m))


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    opts = _capi.esc_render_options()
    calls = {
        "esc_camera_rays": lambda: lib.esc_camera_rays(None, C.byref(cam), 4, 4, 0, 4, None, None, None),
        "esc_shade_rays": lambda: lib.esc_shade_rays(None, 4, None, None, 0, C.byref(opts), None, None, None,
                                                     None, None),
        "esc_render_supersampled": lambda: lib.esc_render_supersampled(None, C.byref(cam), 4, 4, 4,
                                                                       C.byref(opts), None, None),
        "esc_last_shade_stats": lambda: lib.esc_last_shade_stats(None, C.byref(_capi.esc_shade_stats())),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = _last_error(lib)
        assert msg and name in msg and "ctx" in msg, (name, msg)


def test_shade_stats_layout_matches_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "esctp1_rt.h"\n'
                   f"_Static_assert(sizeof(esc_shade_stats) == {C.sizeof(_capi.esc_shade_stats)}, \"size\");\n"
                   + "".join(f"_Static_assert(offsetof(esc_shade_stats, {n}) == "
                             f"{getattr(_capi.esc_shade_stats, n).offset}, \"{n}\");\n"
                             for n, _ in _capi.esc_shade_stats._fields_)
                   + f"_Static_assert(sizeof(esc_query_stats) == {C.sizeof(_capi.esc_query_stats)}, \"q\");\n"
                   + "int main(void) { return 0; }\n")
    r = subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("spp", ["0", "3", "81"])
def test_viewer_rejects_bad_spp(spp, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, "--spp", spp, "-w", "8,6", "-o", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--spp" in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()
