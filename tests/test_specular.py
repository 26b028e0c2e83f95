"""The Phong highlight ks * pow(dot(N, H), Ns) on the GPU, bit for bit (phong_add in csrc/rt_shade.h).

Device powf and glibc powf differ in the last bit, so every older test that meets a specular material
compares with a tolerance.  Here the renderer itself reports its powf: a probe scene (specular_lib.py)
makes a frame equal to the power per lit pixel, the oracle's replaceable pow (rt_oracle.h ORC_POW_*)
says which base x = dot(N, H) and exponent that pixel has, and then
  3a  every GPU path gives the same probe frame, lit exactly where the oracle's is, and each value lies
      within K = 2 fp32 steps of the exact x^Ns (mpmath): 1 for "device and glibc differ in the last
      bit" (the project's statement), 1 for glibc against exact (test_specular_cpu.py asserts that).
      With Ns in {16.5, 64, 120} one step of x moves x^Ns by >= Ns / 2 >= 8 steps, so this pins x;
  3b  with the measured powers fed back into the oracle as a table, frames of scenes with real specular
      materials are compared bit for bit, with no table miss; traced rays (the `_ns` cases of
      ray_cases.py, a refraction case) take their table level by level from `shade`;
  3c  with two and three lights the oracle's frames under powers 2 steps below and above the exact one
      bracket the GPU frame value by value (everything after the power is monotone for ks >= 0);
  4   where ks == +-0 the colour depends only on whether the power is finite and >= +0, so frames equal
      the oracle's bit for bit at every edge of the kernels' run-time skip of the term."""
import numpy as np
import pytest

import oracle_lib as ol
import specular_lib as sl
from ray_cases import TRACE_SETTINGS, camera_targets, product
from ray_oracle import FRESNEL, MODE_NAME, REFRACT, assert_same, oracle_trace, stats_of

pytestmark = pytest.mark.gpu
F32 = np.float32
K = 2


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def gpu_paths(esc):
    stages = (("smem", esc.ESC_STAGE_SMEM), ("lds", esc.ESC_STAGE_LDS), ("bvh", esc.ESC_STAGE_BVH))
    flags = (("default", 0), ("queue", esc.ESC_RENDER_SHADE_QUEUE), ("fused", esc.ESC_RENDER_SHADE_FUSED),
             ("exact", esc.ESC_RENDER_EXACT_ONLY))
    return [(f"{sn}/{fn}/px{px}", {"stage": sv, "flags": fv, "px": px})
            for sn, sv in stages for fn, fv in flags for px in (1, 2, 4)]


def shade_frame(r, cam, W, H, **kw):
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    return r.shade(o.cpu().numpy(), dd.cpu().numpy(), pixel_base=0, **kw)["rgb"].reshape(H, W, 3)


# ---- 3a ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sl.PROBE_CASES)
def test_probe_every_path_reports_the_same_power_within_k_of_exact(esc, r, name):
    d, eye, look, W, H, vfov, kw, fr = sl.probe_case_frames(name)
    x, ns = sl.check_probe_inputs(name)  # nl == 1, every Ns lit, the pinning share, the range of x
    r.upload(ol.scene_to_product(d))
    cam = esc.Camera.for_image(eye, look, W, H, vfov=vfov)
    first = None
    for what, opts in gpu_paths(esc) + [("shade", None)]:
        img = shade_frame(r, cam, W, H, **kw) if opts is None else r.render(cam, W, H, **kw, **opts)
        got = sl.split_frame(fr, img)  # lit exactly where the oracle's ONE frame is, black elsewhere
        if first is None:
            first = got
        diff = bits(got) != bits(first)
        assert not diff.any(), f"{name} {what}: {int(diff.sum())} powers differ from the first path's: x differs"
    steps = sl.steps_from_exact(x, ns, first)  # every lit pixel
    worst = sl.report_steps(f"{name}, device powf ({len(first)} lit pixels)", ns, steps)
    bad = np.flatnonzero(steps > K)
    assert len(bad) == 0, (f"{len(bad)} powers farther than {K} steps from exact, first (x, Ns, got): "
                           f"{[(float(x[i]), float(ns[i]), float(first[i])) for i in bad[:4]]}", worst)


# ---- 3b ---------------------------------------------------------------------------------------------
def real_scene(name):
    hashed = {"face_mode": ol.ORC_FACE_HASH}
    if name == "sphere":
        return ol.load_dump("CornellBox-Sphere"), sl.CORNELL_EYE, sl.CORNELL_LOOK, 96, 72, {**hashed, "seed": 7}
    if name == "sphere_all_specular":  # the dump's own specular pixels are few: ks and Ns on every material
        return (sl.with_specular(ol.load_dump("CornellBox-Sphere"), 3), sl.CORNELL_EYE, sl.CORNELL_LOOK, 96, 72,
                {**hashed, "seed": 7})
    if name == "water":
        return ol.load_dump("CornellBox-Water"), sl.CORNELL_EYE, sl.CORNELL_LOOK, 320, 240, {**hashed, "seed": 3}
    return ol.load_dump("CornellBox-Mirror"), sl.CORNELL_EYE, sl.CORNELL_LOOK, 128, 96, {**hashed, "seed": 5}


@pytest.mark.parametrize("name", ["sphere", "sphere_all_specular", "water", "mirror"])
def test_real_materials_bit_for_bit_through_the_measured_table(esc, r, name, bvh_tree):
    d, eye, look, W, H, kw = real_scene(name)
    assert len(d["light_sources"]) == 1  # nl == 1
    cam = esc.Camera.for_image(eye, look, W, H)

    def render_probe(probe):
        r.upload(ol.scene_to_product(probe))
        return r.render(cam, W, H, **kw)
    table = sl.table_from_probe(d, eye, look, W, H, render_probe, **kw)
    ref, misses = sl.oracle_with_table(d, eye, look, W, H, table, **kw)
    libm = ol.oracle_render(d, eye, look, W, H, threads=8, **kw)
    print(f"{name}: table of {len(table[0])} powers, {misses} misses; the frame under glibc's powf differs in "
          f"{int((bits(libm) != bits(ref)).sum())} of {ref.size} values")
    assert misses == 0
    r.upload(ol.scene_to_product(d))
    for what, stage in (("brute force", esc.ESC_STAGE_AUTO), ("BVH", esc.ESC_STAGE_BVH)):
        gpu, u8 = r.render(cam, W, H, want_u8=True, stage=stage, **kw)
        bad = bits(gpu) != bits(ref)
        assert not bad.any(), f"{name} {what}: {int(bad.sum())} of {ref.size} fp32 values differ"
        assert np.array_equal(u8, ol.oracle_quantise(ref))
    assert ref.sum() > 0


def gpu_shade_probe(r):
    def shade(probe, origins, targets, dirs, fixed_face, shadows):
        r.upload(ol.scene_to_product(probe))
        return r.shade(origins, dirs, fixed_face=fixed_face, shadows=shadows)["rgb"]
    return shade


@pytest.mark.parametrize("name", ["cornell_mixed_ns", "rand3_ns", "rand9_ns"])  # one light each (trace_ns_case)
def test_ns_trace_cases_bit_for_bit_through_level_tables(esc, r, name):
    """ray_cases.py's `_ns` cases at their settings: each level's rays (from the restatement; they
    depend on no power) are shaded on the probe scene, which gives the table for oracle_trace"""
    d, o, a = sl.trace_ns_case(name)
    one_face = all(len(d["geometry"][g]["face_index"]) == 1 for g in d["light_sources"])
    for max_depth, bias, shadows in TRACE_SETTINGS[1::3]:
        bias = float(F32(bias))
        levels, recording = sl.recorded_levels()
        first = oracle_trace(d, o, a, max_depth, bias, shadows=shadows, colours=recording)
        dirs, counts, hits0 = first["dirs"], first["depth_rays"], first["hit_rays0"]
        assert first["usable"].all() and counts[1] * 10 >= hits0 > 0 and counts[2] >= 1  # every ray is compared
        table = sl.table_from_levels(d, levels, gpu_shade_probe(r))
        with ol.pow_mode(ol.POW_TABLE, table=table):
            again = oracle_trace(d, o, a, max_depth, bias, shadows=shadows, colours=sl.ray_colours)
            misses = ol.pow_misses()
        want, counts2 = again["rgb"], again["depth_rays"]
        print(f"{name} depth {max_depth}: {len(o)} rays, levels {counts[:max_depth + 1]}, table of {len(table[0])} "
              f"powers, {misses} misses")
        assert misses == 0 and counts2 == counts
        r.upload(ol.scene_to_product(d))
        for mode in (esc.ESC_FACE_FIXED,) + ((esc.ESC_FACE_HASH,) if one_face else ()):
            for exact in (False, True):
                got = r.trace(o, dirs, max_depth=max_depth, bias=bias, shadows=shadows, face_mode=mode, seed=77,
                              pixel_base=1234, exact=exact)
                assert r.trace_stats()["depth_rays"] == counts
                assert_same(got["rgb"], want, f"{name} depth {max_depth} mode {mode} exact {exact}")
                assert np.array_equal(got["rgb8"], ol.oracle_quantise(want))


def test_refraction_with_exponents_bit_for_bit_through_level_tables(esc, r):
    d, o, a = sl.refraction_ns_case("slab")
    depth, bias, shadows = sl.REFRACTION_SETTING
    assert len(o) >= 64 and len(d["light_sources"]) == 1
    for mode in (REFRACT, FRESNEL):
        levels, recording = sl.recorded_levels()
        first = oracle_trace(d, o, a, depth, bias, mode, shadows=shadows, colours=recording)
        assert first["usable"].all() and first["refracted"] > 0 and first["depth_rays"][2] > 0
        table = sl.table_from_levels(d, levels, gpu_shade_probe(r))
        with ol.pow_mode(ol.POW_TABLE, table=table):
            want = oracle_trace(d, o, a, depth, bias, mode, shadows=shadows, colours=sl.ray_colours)
            misses = ol.pow_misses()
        print(f"slab {MODE_NAME[mode]}: {len(o)} rays, levels {want['depth_rays'][:depth + 1]}, table of "
              f"{len(table[0])} powers, {misses} misses")
        assert misses == 0 and want["depth_rays"] == first["depth_rays"]
        r.upload(product(d))
        for exact in (False, True):
            got = r.trace(o, want["dirs"], max_depth=depth, bias=bias, shadows=shadows, seed=77,
                          pixel_base=1234, exact=exact, transmission=MODE_NAME[mode])
            assert r.trace_stats()["depth_rays"] == want["depth_rays"]
            assert r.transmit_stats() == stats_of(want)
            assert_same(got["rgb"], want["rgb"], f"slab {MODE_NAME[mode]} exact {exact}")
            assert np.array_equal(got["rgb8"], ol.oracle_quantise(want["rgb"]))


# ---- 3c ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "three"])
def test_several_lights_inside_the_bracket(esc, r, name):
    d, eye, look, W, H = sl.bracket_scenes()[name]
    assert len(d["light_sources"]) == (2 if name == "two" else 3)
    with ol.pow_mode(ol.POW_ROUNDED, -K):
        lo = ol.oracle_render(d, eye, look, W, H, threads=8)
    with ol.pow_mode(ol.POW_ROUNDED, K):
        hi = ol.oracle_render(d, eye, look, W, H, threads=8)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
    width = sl.steps_between(lo, hi)
    print(f"{name}: widest bracket {int(width.max())} fp32 steps ({float((width > 0).mean()):.3f} of the values open)")
    r.upload(ol.scene_to_product(d))
    cam = esc.Camera.for_image(eye, look, W, H)
    for what, opts in (("queue", {"flags": esc.ESC_RENDER_SHADE_QUEUE}), ("fused", {"flags": esc.ESC_RENDER_SHADE_FUSED}),
                       ("BVH", {"stage": esc.ESC_STAGE_BVH})):
        gpu = r.render(cam, W, H, **opts)
        assert np.isfinite(gpu).all(), what
        assert np.array_equal(gpu == 0, lo == 0) and np.array_equal(gpu == 0, hi == 0), what
        out = (gpu < lo) | (gpu > hi)
        assert not out.any(), f"{name} {what}: {int(out.sum())} values outside the bracket"
    # trace at depth 3: every level's colour is such a frame value, weighted by products of ks >= 0
    o, a = camera_targets(eye, look, 24, 16)
    bias = float(F32(1e-4))
    # as case_rays does: only rays whose bounce directions the hand-built camera reproduces (no power has
    # a say in that), chosen by the oracle before the GPU is used; then every ray is compared
    keep = oracle_trace(d, o, a, 3, bias)["usable"]
    print(f"{name}: {int(keep.sum())} of {len(keep)} camera rays kept for the trace")
    assert keep.sum() >= 192
    o, a = o[keep], a[keep]
    with ol.pow_mode(ol.POW_ROUNDED, -K):
        low = oracle_trace(d, o, a, 3, bias)
    with ol.pow_mode(ol.POW_ROUNDED, K):
        high = oracle_trace(d, o, a, 3, bias)
    dirs, tlo, thi, counts = low["dirs"], low["rgb"], high["rgb"], low["depth_rays"]
    assert low["usable"].all() and high["usable"].all() and counts == high["depth_rays"] and counts[3] > 0, counts
    got = r.trace(o, dirs, max_depth=3, bias=bias)
    assert r.trace_stats()["depth_rays"] == counts
    rgb = got["rgb"]
    assert np.isfinite(rgb).all()
    out = (rgb < tlo) | (rgb > thi)
    print(f"{name}: trace depth 3, {len(o)} rays, levels {counts[:4]}, widest bracket "
          f"{int(sl.steps_between(tlo, thi).max())} fp32 steps")
    assert not out.any(), f"{name} trace: {int(out.sum())} values outside the bracket"


# ---- 4 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "spheres", "odd_patches"])
def test_the_skip_at_its_edges(esc, r, name):
    d, eye, look, W, H, vfov = sl.odd_patch_scene() if name == "odd_patches" else sl.edge_scene(name)
    ref = ol.oracle_render(d, eye, look, W, H, threads=8, vfov=vfov)
    ref8 = ol.oracle_quantise(ref)
    assert np.isnan(ref).any() and (np.isfinite(ref) & (ref > 0)).any()
    r.upload(ol.scene_to_product(d))
    cam = esc.Camera.for_image(eye, look, W, H, vfov=vfov)
    for what, opts in gpu_paths(esc):
        gpu, u8 = r.render(cam, W, H, want_u8=True, **opts)
        assert_same(gpu, ref, f"{name} {what}")
        assert np.array_equal(u8, ref8), f"{name} {what}: bytes"  # NaN pixels included
    assert_same(shade_frame(r, cam, W, H), ref, f"{name} shade")
    assert_same(shade_frame(r, cam, W, H, exact=True), ref, f"{name} shade, exact")
    if name != "cornell":  # no material reflects here (every ks is +-0): a deeper trace is the frame
        o, dd = r.camera_rays(cam, W, H)
        r.synchronize()
        got = r.trace(o.cpu().numpy(), dd.cpu().numpy(), max_depth=2, bias=1e-4)
        assert_same(got["rgb"].reshape(H, W, 3), ref, f"{name} trace")
        assert r.trace_stats()["depth_rays"][1] == 0
        return
    # the cornell scene has a mirror strip (Ns = 0: its own power is 1): at depth 2 a NaN colour is
    # multiplied by a weight and added (test_specular_cpu.py checks that the chosen rays do that)
    d, o, a = sl.edge_trace_rays()
    bias = float(F32(1e-4))
    res = oracle_trace(d, o, a, 2, bias)
    dirs, want, counts = res["dirs"], res["rgb"], res["depth_rays"]
    assert res["usable"].all() and counts[1] >= 20
    for exact in (False, True):
        got = r.trace(o, dirs, max_depth=2, bias=bias, exact=exact)
        assert r.trace_stats()["depth_rays"] == counts
        assert_same(got["rgb"], want, f"{name} trace, exact {exact}")
        assert np.array_equal(got["rgb8"], ol.oracle_quantise(want))
