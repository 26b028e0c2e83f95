"""The environment cube map (esc_set_environment and its companions) without a GPU: the C ABI and its
binding, null and invalid arguments, the host-side sky generator and the host build of the kernels' lookup
code against the numpy restatements of tests/environment_lib.py bit for bit, the conditions every case of
tests/environment_cases.py has to meet, and the viewer's --sky parsing.  The library loads without a device;
only esc_context_create needs one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import environment_cases as ec
import environment_lib as el
import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi
from ray_oracle import F32, FRESNEL, REFRACT, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esc_set_environment", "esc_get_environment_res", "esc_environment_sky", "esc_environment_rays",
           "esc_environment_lookup_host")
VIEWER = os.path.join(ROOT, "bin", "ESCViewer2021")
SKY = ((0.1, 0.3, 0.9), (0.8, 0.8, 0.7), (0.2, 0.15, 0.1))


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_environment_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert re.search(r"#define ESC_ENV_MAX_RES 1024\b", header)
    for m in ("set_environment", "environment_rays", "environment"):
        assert callable(getattr(esc.Renderer, m))
    assert isinstance(esc.Renderer.environment_res, property)
    assert callable(esc.environment_sky)


def test_header_compiles_as_c_and_structs_keep_their_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>\n#include "esctp1_rt.h"\n']
    # the new entry points with the types the binding passes
    lines.append("int (*p1)(esc_context *, int32_t, const float *) = esc_set_environment;\n")
    lines.append("int (*p2)(esc_context *, int32_t *) = esc_get_environment_res;\n")
    lines.append("int (*p3)(int32_t, const float *, const float *, const float *, float *) = esc_environment_sky;\n")
    lines.append("int (*p4)(esc_context *, int64_t, const float *, float *, uint8_t *) = esc_environment_rays;\n")
    lines.append("int (*p5)(int32_t, const float *, int64_t, const float *, float *) = esc_environment_lookup_host;\n")
    lines.append("_Static_assert(ESC_ENV_MAX_RES == 1024, \"cap\");\n")
    for name in ("esc_shade_stats", "esc_render_options", "esc_adaptive_options", "esc_adaptive_stats",
                 "esc_trace_options", "esc_trace_stats", "esc_transmit_stats", "esc_ambient_options",
                 "esc_ambient_stats"):  # no struct changes layout
        lines.append(f"_Static_assert(sizeof({name}) == {C.sizeof(getattr(_capi, name))}, \"{name}\");\n")
    lines.append("int main(void) { return 0; }\n")
    src = tmp_path / "layout.c"
    src.write_text("".join(lines))
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-Wno-unused-variable", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_invalid_arguments():
    lib = _capi.load()
    cube = np.zeros((6, 2, 2, 3), F32)
    res = C.c_int32(7)
    calls = {
        "esc_set_environment": lambda: lib.esc_set_environment(None, 2, _f(cube)),
        "esc_get_environment_res": lambda: lib.esc_get_environment_res(None, C.byref(res)),
        "esc_environment_rays": lambda: lib.esc_environment_rays(None, 0, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _capi.ESC_ERR_INVALID, name
        msg = lib.esc_last_error().decode()
        assert msg and name in msg and "ctx" in msg, (name, msg)
    assert lib.esc_set_environment(None, 0, None) == _capi.ESC_ERR_INVALID
    col = np.zeros(3, F32)
    out = np.zeros(6 * 3, F32)
    for r_ in (0, -1, 1025):
        assert lib.esc_environment_sky(r_, _f(col), _f(col), _f(col), _f(out)) == _capi.ESC_ERR_INVALID
        assert "esc_environment_sky" in lib.esc_last_error().decode()
        assert lib.esc_environment_lookup_host(r_, _f(cube), 1, _f(col), _f(out)) == _capi.ESC_ERR_INVALID
        assert "esc_environment_lookup_host" in lib.esc_last_error().decode()
    for args in ((None, _f(col), _f(col), _f(out)), (_f(col), None, _f(col), _f(out)),
                 (_f(col), _f(col), None, _f(out)), (_f(col), _f(col), _f(col), None)):
        assert lib.esc_environment_sky(1, *args) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_lookup_host(2, None, 1, _f(col), _f(out)) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_lookup_host(2, _f(cube), 1, None, _f(out)) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_lookup_host(2, _f(cube), 1, _f(col), None) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_lookup_host(2, _f(cube), -1, _f(col), _f(out)) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_lookup_host(2, _f(cube), 0, None, None) == _capi.ESC_OK
    with pytest.raises(ValueError):
        esc.environment_lookup_host(np.zeros((6, 2, 3, 3), F32), np.zeros((1, 3), F32))


@pytest.mark.parametrize("res", [1, 2, 5, 64])
def test_sky_equals_the_float64_restatement(res):
    got = esc.environment_sky(res, *SKY)
    want = el.sky_ref(res, *SKY)
    assert got.shape == (6, res, res, 3) and got.dtype == np.float32
    assert got.tobytes() == want.tobytes()
    # +y is the zenith's side, -y the ground's
    assert np.all(got[2, ..., 2] > got[3, ..., 2])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[4], got[5])  # D.x, D.z enter squared


def test_sky_at_the_poles_and_the_horizon():
    got = esc.environment_sky(1, *SKY)  # one texel per face: D = +-axis
    for f, col in ((2, SKY[0]), (3, SKY[2]), (0, SKY[1]), (1, SKY[1]), (4, SKY[1]), (5, SKY[1])):
        assert np.array_equal(got[f, 0, 0], np.array(col, F32)), f


@pytest.mark.parametrize("res", ec.LOOKUP_RES)
def test_direction_set_condition(res):
    ec.check_directions(res, verbose=True)


@pytest.mark.parametrize("res", ec.LOOKUP_RES)
def test_host_lookup_equals_the_restatement(res):
    cube = el.random_cube(res)
    got = esc.environment_lookup_host(cube, ec.DIRECTIONS)
    want = el.env_parts(cube, ec.DIRECTIONS)
    assert_same(got, want["rgb"], f"R = {res}")
    assert not got[~want["defined"]].view(np.uint32).any()  # an undefined direction: +0, not -0
    assert got[want["defined"]].any()


@pytest.mark.parametrize("res", [1, 3, 64])
def test_a_constant_cube_returns_its_colour_exactly(res):
    col = np.array([0.1, 1.7, 3e-39], F32)  # a subnormal channel too
    cube = np.broadcast_to(col, (6, res, res, 3)).copy()
    got = esc.environment_lookup_host(cube, ec.DIRECTIONS)
    ok = el.env_parts(cube, ec.DIRECTIONS)["defined"]
    assert np.array_equal(got[ok].view(np.uint32), np.broadcast_to(col, got[ok].shape).view(np.uint32))
    assert_same(el.env_ref(cube, ec.DIRECTIONS), got, "restatement")


def test_one_texel_per_face_and_the_face_order():
    cube = np.zeros((6, 1, 1, 3), F32)
    cube[:, 0, 0, 0] = np.arange(1, 7)
    dirs = np.array([[2, 1, -1], [-2, 1, 1], [0.5, 3, 1], [0, -1, 0.5], [0.1, 0.2, 0.3], [0, 0, -1e-40],
                     [1, 1, 1], [-1, 1, 1], [0, -1, 1]], F32)
    got = esc.environment_lookup_host(cube, dirs)[:, 0]
    # ties go to the lower axis: x over y over z
    assert got.tolist() == [1, 2, 3, 4, 5, 6, 1, 2, 4]


def test_texel_centres_and_the_bilinear_weights():
    R = 4
    cube = el.random_cube(R, 5)
    # direction through the centre of texel (face +z, j, i): a = x = ((i + 0.5)/R)*2 - 1, b = y likewise
    for (j, i) in ((0, 0), (1, 2), (3, 3)):
        d = np.array([[((i + 0.5) / R) * 2 - 1, ((j + 0.5) / R) * 2 - 1, 1.0]], F32)
        assert np.array_equal(esc.environment_lookup_host(cube, d)[0], cube[4, j, i])
        assert np.array_equal(esc.environment_lookup_host(cube, -d)[0], cube[5, R - 1 - j, R - 1 - i])
    # no mirroring per face: on -x, a is still d.y and b still d.z
    d = np.array([[-1.0, ((2 + 0.5) / R) * 2 - 1, ((1 + 0.5) / R) * 2 - 1]], F32)
    assert np.array_equal(esc.environment_lookup_host(cube, d)[0], cube[1, 1, 2])
    # half way between two centres of a row: the mean, in the definition's operation order
    d = np.array([[0.0, ((1 + 0.5) / R) * 2 - 1, 1.0]], F32)  # x = 1.5: i0 = 1, fx = 0.5
    a, b = cube[4, 1, 1], cube[4, 1, 2]
    assert np.array_equal(esc.environment_lookup_host(cube, d)[0], (a + ((b - a).astype(F32) * F32(0.5)).astype(F32)))
    # the length of d does not matter
    dirs = ec.DIRECTIONS[ec.DIRECTION_CLASS == "normal"][:512]
    assert_same(esc.environment_lookup_host(cube, dirs * F32(4)), esc.environment_lookup_host(cube, dirs), "scaled")


@pytest.mark.parametrize("name", ec.TRACE_NAMES)
def test_trace_case_condition(name):
    ec.check_trace_case(name, verbose=True)


@pytest.mark.parametrize("mode", [REFRACT, FRESNEL])
def test_glass_case_condition(mode):
    ec.check_glass_case(mode, verbose=True)


def test_the_oracle_callable_changes_only_the_misses():
    """with a cube of zeros the restatement with the rule is the restatement without it, bit for bit, and
    with the random cube every ray that misses at level 0 has env(d) as its colour"""
    name = "cornell_mixed"
    d, o, a = ec.case_rays(name)
    plain = ec.want(name, 2, cube=None)
    zero = ec.want(name, 2, cube=np.zeros((6, 8, 8, 3), F32), key="zero")
    assert_same(zero["rgb"], plain["rgb"], "zeros")
    assert zero["depth_rays"] == plain["depth_rays"]
    w = ec.want(name, 2)
    assert w["depth_rays"] == plain["depth_rays"] and w["hit_rays0"] == plain["hit_rays0"]
    from ray_oracle import ref_queries
    hit, _ = ref_queries(d, o, w["dirs"])
    miss = (hit["geom"] < 0) & (hit["prim"] < 0)
    assert miss.sum() >= 10
    assert_same(w["rgb"][miss], el.env_ref(ec.TRACE_CUBE, w["dirs"][miss]), "level-0 misses")
    assert (w["rgb"][miss] != plain["rgb"][miss]).any()


@pytest.mark.parametrize("args,word", [
    (["--sky"], "--sky"), (["--sky", "1,1,1/1,1,1"], "--sky"), (["--sky", "1,1,1/1,1,1/1,1"], "--sky"),
    (["--sky", "1,1,1/1,1,1/1,1,x"], "--sky"), (["--sky", "1,1,1/1,1,1/1,1,nan"], "--sky"),
    (["--sky", "1,1,1/1,1,1/1,1,1/"], "--sky"), (["--sky", "1,1,1/1,1,1/1,1,inf"], "--sky"),
    (["--sky-res", "8"], "--sky-res"), (["--sky", "1,1,1/1,1,1/1,1,1", "--sky-res", "0"], "--sky-res"),
    (["--sky", "1,1,1/1,1,1/1,1,1", "--sky-res", "1025"], "--sky-res"),
    (["--sky", "1,1,1/1,1,1/1,1,1", "--sky-res", "8x"], "--sky-res"),
    (["--sky", "1,1,1/1,1,1/1,1,1", "--gpus", "2"], "--sky"), (["--sky", "1,1,1/1,1,1/1,1,1", "--ispc"], "--sky"),
    (["--sky", "1,1,1/1,1,1/1,1,1", "--adaptive", "0.1", "--spp", "4"], "--sky")],
    ids=["no-value", "two-colours", "short-colour", "not-a-number", "nan", "trailing", "inf", "res-alone", "res-zero",
         "res-too-large", "res-trailing", "gpus", "ispc", "adaptive"])
def test_viewer_rejects_bad_sky(args, word, tmp_path):
    assert os.path.exists(VIEWER), "build the viewer (make / __graft_entry__.build())"
    out = tmp_path / "x.ppm"
    r = subprocess.run([VIEWER, *args, "-w", "8,6", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert word in r.stderr, r.stderr
    assert "device" not in r.stderr.lower(), r.stderr  # rejected while parsing, before any device
    assert not out.exists()
