"""Refraction (esc_trace_rays_ex / esc_render_traced_ex / esc_last_transmit_stats and the transmission
side table of a scene): the C ABI, its binding, the loader's Tf / Ni / illum and the viewer's --refract /
--fresnel parsing, checked without a GPU (the library loads without one; only esc_context_create needs a
device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import esctp1raytracer_amd as esc
import oracle_lib as ol
from esctp1raytracer_amd import _capi
from model_files import models  # noqa: F401  (the fixture that unpacks cornell_models.tar.gz)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")
F32 = np.float32
ENTRIES = {"esc_trace_rays_ex": 9, "esc_render_traced_ex": 9, "esc_last_transmit_stats": 2,
           "esc_scene_set_geometry_transmission": 3, "esc_scene_get_geometry_transmission": 3,
           "esc_scene_set_sphere_transmission": 4, "esc_scene_get_sphere_transmission": 2}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name, n_args in ENTRIES.items():
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(_capi.SIGNATURES[name][1])
    P, I32, I64, U32, F = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float
    opts, topts = C.POINTER(_capi.esc_render_options), C.POINTER(_capi.esc_trace_options)
    assert _capi.SIGNATURES["esc_trace_rays_ex"][1] == [P, I64, P, P, U32, opts, topts, P, P]
    assert _capi.SIGNATURES["esc_render_traced_ex"][1] == [P, C.POINTER(_capi.esc_camera), I32, I32, I32, opts,
                                                           topts, P, P]
    assert [(n, t) for n, t in _capi.esc_trace_options._fields_] == \
        [("max_depth", I32), ("bias", F), ("transmission", I32), ("reserved", I32)]
    assert [n for n, _ in _capi.esc_transmit_stats._fields_] == ["refracted", "fresnel_reflected", "total_internal"]
    assert C.sizeof(_capi.esc_trace_options) == 16 and C.sizeof(_capi.esc_transmit_stats) == 24
    assert (esc.ESC_TRANSMIT_OFF, esc.ESC_TRANSMIT_REFRACT, esc.ESC_TRANSMIT_FRESNEL) == (0, 1, 2)
    for m in ("trace_rays", "trace", "render_traced", "transmit_stats"):
        assert callable(getattr(esc.Renderer, m))
    import inspect
    for m in ("trace_rays", "trace", "render_traced"):
        assert inspect.signature(getattr(esc.Renderer, m)).parameters["transmission"].default == "off"
    for m in ("set_transmission", "set_sphere_transmission", "transmission", "sphere_transmission"):
        assert callable(getattr(esc.Scene, m))


def test_struct_layouts_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "a C compiler is needed to check the header's layouts"
    src = tmp_path / "layout.c"
    text = '#include <stddef.h>\n#include "esctp1_rt.h"\n'
    for T, name in ((_capi.esc_trace_options, "esc_trace_options"), (_capi.esc_transmit_stats, "esc_transmit_stats")):
        text += f"_Static_assert(sizeof({name}) == {C.sizeof(T)}, \"size\");\n"
        text += "".join(f"_Static_assert(offsetof({name}, {n}) == {getattr(T, n).offset}, \"{n}\");\n"
                        for n, _ in T._fields_)
    text += "_Static_assert(sizeof(esc_trace_options) == 16 && sizeof(esc_transmit_stats) == 24, \"sizes\");\n"
    text += "_Static_assert(ESC_TRANSMISSION_FLOATS == 4 && ESC_MATERIAL_FLOATS == 13, \"floats\");\n"
    text += "_Static_assert(ESC_TRANSMIT_OFF == 0 && ESC_TRANSMIT_REFRACT == 1 && ESC_TRANSMIT_FRESNEL == 2, \"m\");\n"
    # the older structs keep their layout
    text += f"_Static_assert(sizeof(esc_trace_stats) == {C.sizeof(_capi.esc_trace_stats)}, \"t\");\n"
    text += "int main(void) { return 0; }\n"
    src.write_text(text)
    r = subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_invalid_with_a_message():
    lib = _capi.load()
    cam = _capi.esc_camera()
    opts = _capi.esc_render_options()
    to = _capi.esc_trace_options(2, 0.0, 1, 0)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails on an argument checked before the context
    sc = esc.Scene()
    t4 = (C.c_float * 4)()
    calls = [
        ("esc_trace_rays_ex", "ctx", lambda: lib.esc_trace_rays_ex(None, 4, None, None, 0, C.byref(opts), C.byref(to),
                                                                   None, None)),
        ("esc_render_traced_ex", "ctx", lambda: lib.esc_render_traced_ex(None, C.byref(cam), 4, 4, 1, C.byref(opts),
                                                                        C.byref(to), None, None)),
        ("esc_last_transmit_stats", "ctx", lambda: lib.esc_last_transmit_stats(None, C.byref(_capi.esc_transmit_stats()))),
        ("esc_last_transmit_stats", "out", lambda: lib.esc_last_transmit_stats(fake, None)),
        ("esc_trace_rays_ex", "options", lambda: lib.esc_trace_rays_ex(fake, 4, None, None, 0, C.byref(opts), None,
                                                                       None, None)),
        ("esc_trace_rays_ex", "opts", lambda: lib.esc_trace_rays_ex(fake, 4, None, None, 0, None, C.byref(to), None,
                                                                    None)),
        ("esc_render_traced_ex", "options", lambda: lib.esc_render_traced_ex(fake, C.byref(cam), 4, 4, 1, C.byref(opts),
                                                                            None, None, None)),
    ]
    for mode, reserved, word in ((3, 0, "transmission"), (-1, 0, "transmission"), (1, 1, "reserved"),
                                 (0, -7, "reserved")):
        bad = _capi.esc_trace_options(2, 0.0, mode, reserved)
        calls.append(("esc_trace_rays_ex", word, lambda bad=bad: lib.esc_trace_rays_ex(
            fake, 4, None, None, 0, C.byref(opts), C.byref(bad), None, None)))
        calls.append(("esc_render_traced_ex", word, lambda bad=bad: lib.esc_render_traced_ex(
            fake, C.byref(cam), 4, 4, 1, C.byref(opts), C.byref(bad), None, None)))
    for geom in (-1, 0, 5):  # an empty scene has no geometry 0
        calls.append(("esc_scene_set_geometry_transmission", "range",
                      lambda geom=geom: lib.esc_scene_set_geometry_transmission(sc._h, geom, t4)))
        calls.append(("esc_scene_get_geometry_transmission", "range",
                      lambda geom=geom: lib.esc_scene_get_geometry_transmission(sc._h, geom, t4)))
    for first, n in ((-1, 1), (0, 1), (1, 0), (0, -1)):
        calls.append(("esc_scene_set_sphere_transmission", "", lambda first=first, n=n:
                      lib.esc_scene_set_sphere_transmission(sc._h, first, n, t4)))
    calls.append(("esc_scene_set_geometry_transmission", "argument",
                  lambda: lib.esc_scene_set_geometry_transmission(None, 0, t4)))
    calls.append(("esc_scene_get_sphere_transmission", "argument",
                  lambda: lib.esc_scene_get_sphere_transmission(None, t4)))
    for name, word, call in calls:
        assert call() == _capi.ESC_ERR_INVALID, (name, word)
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and word in msg, (name, word, msg)
    with pytest.raises(ValueError, match="transmission"):
        esc.Renderer.trace_rays(None, None, None, None, max_depth=1, bias=0.0, transmission="glass")


def _small_scene():
    sc = esc.Scene()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    for k in range(3):
        sc.add_geometry(tri + k, [[0, 1, 2]], ol.material13(kd=(0.5, 0.5, 0.5)))
    sc.add_spheres(np.array([[0, 0, 0, 1], [3, 0, 0, 1], [6, 0, 0, 1], [9, 0, 0, 1]], F32),
                   np.tile(ol.material13(kd=(0.2, 0.3, 0.4), ks=(0.1, 0.2, 0.3), Ns=7.0), (4, 1)))
    return sc


def test_set_get_round_trip_and_defaults():
    sc = _small_scene()
    for g in range(3):
        tf, ni = sc.transmission(g)
        assert tf.tolist() == [0, 0, 0] and ni == 1 and tf.dtype == F32
    tf, ni = sc.sphere_transmission()
    assert tf.shape == (4, 3) and ni.shape == (4,) and not tf.any() and (ni == 1).all()
    odd = np.array([[0.1, 0.2, 0.3, 1.5], [np.nan, -1.0, np.inf, -2.5], [-0.0, 1e-45, 3e38, np.nan],
                    [0, 0, 0, 0]], F32)
    odd[1, 0] = np.array([0x7fc01234], np.uint32).view(F32)[0]  # a NaN with a payload comes back as it went in
    for g, row in ((1, odd[0]), (2, odd[1]), (0, odd[2])):
        sc.set_transmission(g, row[:3], row[3])
    for g, row in ((1, odd[0]), (2, odd[1]), (0, odd[2])):
        tf, ni = sc.transmission(g)
        assert np.array_equal(_bits(tf), _bits(row[:3])) and _bits(ni) == _bits(row[3])
    sc.set_sphere_transmission(1, odd[1:3, :3], odd[1:3, 3])
    tf, ni = sc.sphere_transmission()
    want = np.array([[0, 0, 0, 1], odd[1], odd[2], [0, 0, 0, 1]], F32)
    assert np.array_equal(_bits(tf), _bits(want[:, :3])) and np.array_equal(_bits(ni), _bits(want[:, 3]))
    sc.set_sphere_transmission(0, odd[:, :3], odd[:, 3])
    tf, ni = sc.sphere_transmission()
    assert np.array_equal(_bits(tf), _bits(odd[:, :3])) and np.array_equal(_bits(ni), _bits(odd[:, 3]))
    sc.set_sphere_transmission(4, np.zeros((0, 3), F32), np.zeros(0, F32))  # n == 0 at the end is in range
    with pytest.raises(esc.EscError):
        sc.set_sphere_transmission(3, odd[:2, :3], odd[:2, 3])
    with pytest.raises(esc.EscError):
        sc.set_transmission(3, (0, 0, 0), 1)
    # the 13-float materials are what they were
    for g in range(3):
        assert np.array_equal(sc.geometry(g)["material"], ol.material13(kd=(0.5, 0.5, 0.5)))
    sp, mats = sc.spheres()
    assert mats.shape == (4, 13) and np.array_equal(mats[2], ol.material13(kd=(0.2, 0.3, 0.4), ks=(0.1, 0.2, 0.3), Ns=7.0))
    # spheres added after a set are opaque
    sc.add_spheres(np.array([[12, 0, 0, 1]], F32), ol.material13()[None])
    tf, ni = sc.sphere_transmission()
    assert tf.shape == (5, 3) and not tf[4].any() and ni[4] == 1 and np.array_equal(_bits(tf[:4]), _bits(odd[:, :3]))


def _group_names(obj_path):
    with open(obj_path) as f:
        return [ln.split()[1] for ln in f if ln.startswith("g ") and len(ln.split()) > 1]


def _within_one_ulp(x, decimal):
    want = F32(decimal)
    return abs(int(_bits(x).astype(np.int64).reshape(-1)[0]) - int(_bits(want).astype(np.int64).reshape(-1)[0])) <= 1


GLASS = {"rightSphere": 2.5, "water": 1.33}


@pytest.mark.parametrize("name, transmissive", [("CornellBox-Sphere", ["rightSphere"]),
                                                ("CornellBox-Water", ["rightSphere", "water"]),
                                                ("water", ["water"]), ("CornellBox-Original", []),
                                                ("CornellBox-Mirror", [])])
def test_loader_keeps_tf_and_ni_under_a_transparent_illum(models, name, transmissive):  # noqa: F811
    path = os.path.join(models, "cornell", name + ".obj")
    sc = esc.Scene.load_obj(path)
    if transmissive:  # one geometry per `g` group, in the file's order
        names = _group_names(path)
        assert len(names) == sc.info()["n_geometry"]
        assert [n for n in names if n in GLASS] == transmissive
    else:  # every geometry must be opaque, whatever it is called
        names = [str(g) for g in range(sc.info()["n_geometry"])]
        assert len(names) >= 7
    if name == "CornellBox-Sphere":
        assert "light" in names  # Tf 1 1 1 under illum 2: must stay opaque
    for g, n in enumerate(names):
        tf, ni = sc.transmission(g)
        if n in transmissive:
            assert all(_within_one_ulp(c, "0.10") for c in tf), (n, tf)
            assert _within_one_ulp(ni, str(GLASS[n])), (n, ni)
        else:
            assert tf.tolist() == [0, 0, 0] and ni == 1, (n, tf, ni)
        assert sc.geometry(g)["material"].shape == (13,)
    # the loader dump of the reference still describes what geometry() returns
    d = ol.load_dump(name) if os.path.exists(os.path.join(ol.GOLDEN_DIR, f"loader_{name}.npz")) else None
    if d is not None:
        for g in range(len(names)):
            assert np.array_equal(_bits(sc.geometry(g)["material"]), _bits(d["geometry"][g]["material"]))


def test_viewer_usage_names_both_flags():
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    r = subprocess.run([VIEWER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--refract" in r.stdout and "--fresnel" in r.stdout and "--bounces" in r.stdout


@pytest.mark.parametrize("args, text", [(["--refract"], "--refract needs --bounces"),
                                        (["--fresnel"], "--fresnel needs --bounces"),
                                        (["--refract", "--spp", "4"], "--refract needs --bounces"),
                                        (["--bounces", "2", "--refract", "--fresnel"],
                                         "--refract and --fresnel exclude each other"),
                                        (["--bounces", "2", "--fresnel", "--gpus", "2"], "--bounces renders on one GPU")])
def test_viewer_rejects_bad_transmission_arguments(args, text, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert text in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()
