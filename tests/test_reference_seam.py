"""Compile + link test of the reference-side seam.

The reference's host code reaches the render path through ONE header, the ISPC-generated
`trace_ispc.h` (/root/reference/src/main.cpp:25, src/simplify/flatten_iscp.h:3), and one call,
`ispc::trace(...)` (main.cpp:619-624).  include/trace_ispc.h is the product's replacement for
that header.  The oracle build (oracle/Makefile, `ref`) compiles the reference's own main.cpp and
flatten_iscp.cpp UNTOUCHED, where they lie, against it into oracle/_ref/seam/ (plus the other
reference objects main.cpp needs); this test links those objects with libesctp1rt.so.

Link only.  The relinked binary is never run: the reference's flatten_scene_ispc leaves
`ispc_light.light_faces` dangling (flatten_iscp.cpp:39,103, defect I4), so its --ispc path is
undefined before it reaches `trace` (INTEGRATION.md 1 says what to replace).
The link test skips when oracle/_ref/seam/ was not built (no reference sources at build time).
Outputs go to tmp_path.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "esctp1raytracer_amd", "lib")
SEAM = os.path.join(ROOT, "oracle", "_ref", "seam")
# main.o and flatten_iscp.o include trace_ispc.h -- the seam proper; the rest is the reference's
# link line (CMakeLists.txt:22 minus the ISPC object)
SEAM_OBJS = ["main.o", "flatten_iscp.o", "sceneloader.o", "flatten.o", "aabb.o", "bvh.o",
             "c_vec.o", "c_triangle.o"]


def _run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    assert p.returncode == 0, f"{' '.join(cmd)}\n{p.stdout}\n{p.stderr}"
    return p


@pytest.mark.skipif(not all(os.path.exists(os.path.join(SEAM, o)) for o in SEAM_OBJS),
                    reason="oracle/_ref/seam not built (needs the reference sources at build time)")
def test_reference_host_compiles_and_links_against_the_library(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    assert os.path.exists(os.path.join(LIBDIR, "libesctp1rt.so"))
    objs = [os.path.join(SEAM, o) for o in SEAM_OBJS]
    # main.o must reference the plain C symbol `trace` (undefined, to be bound by the library)
    nm = _run(["nm", "-u", objs[0]], tmp_path).stdout.split()
    assert "trace" in nm, "main.cpp does not call the C symbol `trace`"
    exe = str(tmp_path / "ESCViewer2021_relinked")
    _run([cxx] + objs + ["-pthread", f"-L{LIBDIR}", "-lesctp1rt", f"-Wl,-rpath,{LIBDIR}",
                         "-Wl,--no-undefined", "-o", exe], tmp_path)
    # `trace` is resolved by OUR library, nothing else defines it
    dyn = _run(["nm", "-D", "--undefined-only", exe], tmp_path).stdout.split()
    assert "trace" in dyn
    ldd = _run(["ldd", exe], tmp_path).stdout
    assert "libesctp1rt.so" in ldd
    # NOT run: see the module docstring


def test_c_and_cxx_declarations_of_trace_agree(tmp_path):
    """A C caller (esctp1_rt.h, pointer) and the reference's C++ caller (trace_ispc.h, reference)
    must produce the same call: compile both and compare the symbol they reference."""
    cxx = shutil.which("g++")
    (tmp_path / "c_side.c").write_text(
        '#include "esctp1_rt.h"\n'
        "void call_c(ispc_cam *c, float *img) { trace(4, 4, c, 0, 0, 0, 0, 0, 0, img, 0, 0); }\n")
    (tmp_path / "cxx_side.cpp").write_text(
        '#include "trace_ispc.h"\n'
        "void call_cxx(ispc::ispc_cam &c, float *img) {"
        " ispc::trace(4, 4, c, 0, nullptr, 0, nullptr, 0, nullptr, img, 0, 0); }\n")
    _run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", "-c", "c_side.c"], tmp_path)
    _run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", "-c", "cxx_side.cpp"],
         tmp_path)
    for o in ("c_side.o", "cxx_side.o"):
        assert "trace" in _run(["nm", "-u", o], tmp_path).stdout.split()
