"""Batched ray queries (esc_intersect_rays / esc_occluded_rays / esc_last_query_stats): the C ABI
and its binding, checked without a GPU (the library loads without one; only esc_context_create
needs a device)."""
import ctypes as C
import os
import re

import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esc_intersect_rays", "esc_occluded_rays", "esc_last_query_stats")


def test_query_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "esctp1_rt.h")) as f:
        header = f.read()
    assert re.search(r"typedef struct \{\s*uint64_t rays;.*?uint64_t exact_rays;.*?uint64_t exact_tests;"
                     r".*?\} esc_query_stats;", header, re.S)
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [f[0] for f in _capi.esc_query_stats._fields_] == ["rays", "exact_rays", "exact_tests"]
    assert C.sizeof(_capi.esc_query_stats) == 24
    for m in ("intersect_rays", "occluded_rays", "intersect", "occluded", "query_stats"):
        assert callable(getattr(esc.Renderer, m))


def _last_error(lib):
    return lib.esc_last_error().decode()


def test_null_context_is_invalid_with_a_message():
    lib = _capi.load()
    rc = lib.esc_intersect_rays(None, 4, None, None, None, None, None, None, None, 0)
    assert rc == _capi.ESC_ERR_INVALID
    assert "esc_intersect_rays" in _last_error(lib) and "ctx" in _last_error(lib)
    rc = lib.esc_occluded_rays(None, 4, None, None, None, None, 0)
    assert rc == _capi.ESC_ERR_INVALID
    assert "esc_occluded_rays" in _last_error(lib) and "ctx" in _last_error(lib)
    st = _capi.esc_query_stats()
    rc = lib.esc_last_query_stats(None, C.byref(st))
    assert rc == _capi.ESC_ERR_INVALID
    assert "esc_last_query_stats" in _last_error(lib) and "ctx" in _last_error(lib)
