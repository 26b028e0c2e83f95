"""The oracle's replaceable pow (oracle/rt_oracle.h ORC_POW_*) and everything tests/test_specular.py
takes for granted about the reference side, checked without a GPU: the setting restores; the BASE frame
of a probe scene is dot(N, H) as the pinned pieces restate it; ROUNDED is the exact power rounded and
moved; TABLE reproduces what it was filled with and counts what it lacks; glibc's powf lies within one
fp32 step of the exact power on every (x, Ns) the GPU tests use (the K = 2 they assert is 1 for "device
and glibc differ in the last bit" plus this 1); the brackets of 3c hold for the reference itself; and
the scenes of section 4 contain what they are there for."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import specular_lib as sl
from ray_cases import TRACE_SETTINGS
from ray_oracle import (EPS, F32, FRESNEL, MODE_NAME, REFRACT, dot, normalize, normals_and_ks, oracle_trace,
                        ref_queries, same_bits)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def sphere_frame(**kw):
    return ol.oracle_render(ol.load_dump("CornellBox-Sphere"), sl.CORNELL_EYE, sl.CORNELL_LOOK, 64, 48, threads=8,
                            face_mode=ol.ORC_FACE_HASH, seed=7, **kw)


def test_the_setting_restores():
    before = sphere_frame()
    for mode, steps in ((ol.POW_BASE, 0), (ol.POW_ONE, 0), (ol.POW_ROUNDED, 3)):
        with ol.pow_mode(mode, steps):
            inside = sphere_frame()
        assert (bits(inside) != bits(before)).any()
    with pytest.raises(ZeroDivisionError):
        with ol.pow_mode(ol.POW_EXPONENT):
            1 / 0
    assert ol.oracle().orc_pow_get_mode() == ol.POW_LIBM
    assert np.array_equal(bits(sphere_frame()), bits(before))
    fast = ol.oracle_fast()
    if fast is not None:  # the packet library follows the same setting
        d = ol.load_dump("CornellBox-Sphere")
        rows = list(range(0, 48, 5))
        with ol.pow_mode(ol.POW_BASE):
            a, _ = ol.oracle_render_rows(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, 64, 48, rows, fast=False)
            b, _ = ol.oracle_render_rows(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, 64, 48, rows, fast=True)
        c, _ = ol.oracle_render_rows(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, 64, 48, rows, fast=True)
        assert np.array_equal(bits(a), bits(b)) and (bits(b) != bits(c)).any()
        assert fast.orc_pow_get_mode() == ol.POW_LIBM
    assert ol.oracle().orc_pow_set_mode(ol.POW_ROUNDED, 5) == -1 and ol.oracle().orc_pow_set_mode(9, 0) == -1


def restated_x(d, eye, look, W, H, seed):
    """dot(N, H) of main.cpp:775-783 per pixel from the pinned pieces, NaN where the oracle's own
    frame has to say whether the pixel is lit (occlusion is not restated here)"""
    lib = ol.oracle()
    cam = ol.oracle_camera(eye, look, W, H)
    dirs = np.zeros((H * W, 3), F32)
    out = np.zeros(3, F32)
    for h in range(H):
        for w in range(W):
            lib.orc_camera_get_ray(C.byref(cam), C.c_float(F32(w) / F32(W - 1)), C.c_float(F32(h) / F32(H - 1)),
                                   ol.fp(out))
            dirs[h * W + w] = out
    o = np.tile(np.array(list(cam.origin), F32), (H * W, 1))
    hit, _ = ref_queries(d, o, dirs)
    N, _, has = normals_and_ks(d, hit, o, dirs)
    light = d["geometry"][d["light_sources"][0]]
    nf = len(light["face_index"])
    face = np.array([lib.orc_face_hash(seed, p, 0, nf) for p in range(H * W)])
    P = (light["vertex"][face] + F32(0)).astype(F32)
    with np.errstate(all="ignore"):
        hitp = (o + (dirs * (hit["t"] - EPS).astype(F32)[:, None]).astype(F32)).astype(F32)
        L = normalize((P - hitp).astype(F32))
        Hh = normalize(((N + L).astype(F32) * F32(2)).astype(F32))
        x = dot(N, Hh)
    x[~has] = np.nan
    return x.reshape(H, W)


@pytest.mark.parametrize("name", ["CornellBox-Original", "CornellBox-Sphere"])  # flat / smooth normals (S1)
def test_base_frame_is_the_restated_x(name):
    d = sl.probe_split(ol.load_dump(name))
    smooth = [len(g["normals"]) > 0 for g in d["geometry"]]  # every geometry of the Sphere dump has normals
    assert all(smooth) if name == "CornellBox-Sphere" else not any(smooth)
    W, H = 40, 30
    fr = sl.oracle_probe_frames(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, face_mode=ol.ORC_FACE_HASH, seed=7)
    x = restated_x(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, 7)
    lit = fr["lit"]
    assert lit.sum() > W * H // 4
    assert np.array_equal(bits(fr["base"][..., 1][lit]), bits(x[lit]))


def scene_pairs(n):
    x, ns = [], []
    for name in ("sphere", "original"):
        fr = sl.probe_case_frames(name)[-1]
        x.append(fr["base"][..., 1][fr["lit"]])
        ns.append(fr["expo"][..., 1][fr["lit"]])
    x, ns = np.concatenate(x), np.concatenate(ns)
    pick = np.random.default_rng(1).choice(len(x), n, replace=False)
    return x[pick], ns[pick]


def test_rounded_is_the_exact_power_rounded_and_moved():
    import mpmath
    lib = ol.oracle()
    x, ns = scene_pairs(3000)
    with mpmath.workprec(120):
        want = np.array([sl.round_to_f32(sl._exact(a, b)) for a, b in zip(x, ns)], F32)
    got = {}
    for k in range(-4, 5):
        with ol.pow_mode(ol.POW_ROUNDED, k):
            got[k] = np.array([lib.orc_pow(C.c_float(a), C.c_float(b)) for a, b in zip(x, ns)], F32)
    assert np.array_equal(bits(got[0]), bits(want))
    moves = want != 0  # a zero result stays
    assert moves.sum() > 2500 and (~moves).any()
    for k in range(1, 5):
        up, down = want.copy(), want.copy()
        for _ in range(k):
            up = np.where(up == 0, up, np.nextafter(up, F32(np.inf)))
            down = np.where(down == 0, down, np.nextafter(down, F32(-np.inf)))
        assert np.array_equal(bits(got[k]), bits(up)) and np.array_equal(bits(got[-k]), bits(down))
        assert (sl.steps_between(got[-k], got[k])[moves & (down != 0)] == 2 * k).all()
    with ol.pow_mode(ol.POW_ROUNDED, 4):  # NaN, inf and 0 results are left alone
        for a, b in ((np.nan, 2.0), (2.0, 1000.0), (0.5, 1000.0), (0.5, -1000.0), (0.0, 3.0)):
            with np.errstate(all="ignore"):
                v, w = lib.orc_pow(C.c_float(a), C.c_float(b)), float(F32(np.float64(a) ** np.float64(b)))
            assert (np.isnan(v) and np.isnan(w)) or v == w, (a, b, v, w)


def test_table_reproduces_its_source_and_counts_misses():
    d = ol.load_dump("CornellBox-Sphere")
    kw = {"face_mode": ol.ORC_FACE_HASH, "seed": 7}
    W, H = 96, 72
    libm = ol.oracle_render(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, threads=8, **kw)
    keys, vals = sl.table_from_probe(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, lambda probe: ol.oracle_render(
        probe, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, threads=8, **kw), **kw)
    assert len(keys) > 1000
    ref, misses = sl.oracle_with_table(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, (keys, vals), **kw)
    assert misses == 0 and np.array_equal(bits(ref), bits(libm))
    # an entry that exactly one pixel uses: the probe's base frame says how often each key occurs
    fr = sl.oracle_probe_frames(sl.probe_keep_ns(d), sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, **kw)
    used = ol.pow_key(fr["base"][..., 1][fr["lit"]], fr["expo"][..., 1][fr["lit"]])
    uk, cnt = np.unique(used, return_counts=True)
    drop = np.searchsorted(keys, uk[cnt == 1][0])
    short = (np.delete(keys, drop), np.delete(vals, drop))
    ref, misses = sl.oracle_with_table(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, short, **kw)
    assert misses == 1 and np.array_equal(bits(ref), bits(libm))
    # other values show in the frame (where ks != 0): the table is really what the oracle uses
    wrong = (vals * F32(2)).astype(F32)
    ref, misses = sl.oracle_with_table(d, sl.CORNELL_EYE, sl.CORNELL_LOOK, W, H, (keys, wrong), **kw)
    assert misses == 0 and (bits(ref) != bits(libm)).any()
    with pytest.raises(AssertionError):
        ol.pow_table([0.5, 0.5], [2.0, 2.0], [0.25, 0.26])


@pytest.mark.parametrize("name", sl.PROBE_CASES)
def test_probe_scenes_and_glibc_within_one_step(name):
    """what 3a needs from its inputs, and the half of K = 2 that is the reference's"""
    d, eye, look, W, H, vfov, kw, fr = sl.probe_case_frames(name)
    x, ns = sl.check_probe_inputs(name)
    libm = sl.split_frame(fr, ol.oracle_render(d, eye, look, W, H, threads=8, vfov=vfov, **kw))
    worst = sl.report_steps(f"{name}, glibc", ns, sl.steps_from_exact(x, ns, libm))
    assert max(worst.values()) <= 1.0
    pin = np.isin(ns, np.array(sl.PIN_NS, F32))
    assert (libm[pin] >= F32(2.0 ** -126)).all()  # normal numbers: a step of x shows as >= Ns / 2 steps


@pytest.mark.parametrize("name", ["two", "three"])
def test_brackets_hold_for_the_reference(name):
    d, eye, look, W, H = sl.bracket_scenes()[name]
    libm = ol.oracle_render(d, eye, look, W, H, threads=8)
    with ol.pow_mode(ol.POW_ROUNDED, -2):
        lo = ol.oracle_render(d, eye, look, W, H, threads=8)
    with ol.pow_mode(ol.POW_ROUNDED, 2):
        hi = ol.oracle_render(d, eye, look, W, H, threads=8)
    assert np.isfinite(libm).all() and (lo <= libm).all() and (libm <= hi).all()
    width = sl.steps_between(lo, hi)
    print(f"{name}: widest bracket {int(width.max())} fp32 steps, {float((width > 0).mean()):.3f} of the values open")
    assert width.max() > 0 and width.max() <= 64


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_edge_scenes_are_not_vacuous(name):
    d, eye, look, W, H, vfov = sl.edge_scene(name)
    img = ol.oracle_render(d, eye, look, W, H, threads=8, vfov=vfov)
    nan = np.isnan(img).any(axis=2)
    fine = np.isfinite(img).all(axis=2) & (img > 0).any(axis=2)
    zero = (img == 0).all(axis=2)
    print(f"edge scene {name}: {int(nan.sum())} NaN, {int(fine.sum())} ordinary, {int(zero.sum())} black pixels")
    assert nan.sum() > 50 and fine.sum() > 50 and zero.sum() > 0
    # scan_row adds every light's colour to a pixel that starts as +0, and (+0) + (-0) is +0: a frame
    # cannot hold a -0, whatever the materials are -- the sign of kd * d + ks * sp is not observable
    assert not np.signbit(img[img == 0]).any()
    # the materials cover both sides of material_spec_free's test
    mats = np.array([g["material"] for g in d["geometry"]] + list(d["sphere_materials"]))
    inside = (mats[:, 12] >= 0) & (mats[:, 12] <= 1024)
    assert inside.any() and (~inside).any() and np.isnan(mats[:, 12]).any()
    reflecting = (mats[:, 6:9] != 0).any(axis=1)  # only the mirror strip of the cornell scene (Ns = 0)
    assert reflecting.sum() == (1 if name == "cornell" else 0) and (mats[reflecting, 12] == 0).all()
    assert np.signbit(mats[:, 6:9]).any()


def test_odd_normals_defeat_an_unconditional_skip():
    """on the odd patches the materials are flagged, yet the power matters: taking 1 for it (what the
    kernels' skip does) changes pixels, so a skip that does not look at |N| is caught there"""
    d, eye, look, W, H, vfov = sl.odd_patch_scene()
    libm = ol.oracle_render(d, eye, look, W, H, threads=8, vfov=vfov)
    with ol.pow_mode(ol.POW_ONE):
        one = ol.oracle_render(d, eye, look, W, H, threads=8, vfov=vfov)
    differ = ~same_bits(libm, one).all(axis=2)
    print(f"odd patches: {int(differ.sum())} pixels depend on the power, {int(np.isnan(libm).any(axis=2).sum())} NaN")
    assert differ.sum() >= 20 and np.isfinite(one[differ]).all() and np.isnan(libm[differ]).any(axis=1).all()


def libm_shade(probe, origins, targets, dirs, fixed_face, shadows):
    """the oracle itself in the place of the renderer under test"""
    got, rgb = sl.ray_colours(probe, origins, targets, fixed_face, shadows)
    assert same_bits(got, dirs).all()
    return rgb


@pytest.mark.parametrize("name", ["cornell_mixed_ns", "rand3_ns", "rand9_ns"])
def test_level_tables_reproduce_the_traced_colours(name):
    """3b's gathering on the reference side alone: the table filled with glibc's powers, level by level,
    gives oracle_trace's own colours with no miss, so it holds every (x, Ns) a traced path meets"""
    d, o, a = sl.trace_ns_case(name)
    for max_depth, bias, shadows in TRACE_SETTINGS[1::3]:
        bias = float(F32(bias))
        levels, recording = sl.recorded_levels()
        first = oracle_trace(d, o, a, max_depth, bias, shadows=shadows, colours=recording)
        want, counts = first["rgb"], first["depth_rays"]
        assert first["usable"].all() and len(levels) == 1 + sum(c > 0 for c in counts[1:max_depth + 1])
        table = sl.table_from_levels(d, levels, libm_shade)
        with ol.pow_mode(ol.POW_TABLE, table=table):
            again = oracle_trace(d, o, a, max_depth, bias, shadows=shadows, colours=sl.ray_colours)
            misses = ol.pow_misses()
        # a zero `horizontal` (sl.ray_colours) changes no colour
        assert same_bits(oracle_trace(d, o, a, max_depth, bias, shadows=shadows)["rgb"], want).all()
        print(f"{name} depth {max_depth}: {len(o)} rays, levels {counts[:max_depth + 1]}, table of {len(table[0])}")
        assert misses == 0 and again["depth_rays"] == counts and same_bits(again["rgb"], want).all()


def test_refraction_level_tables_reproduce_the_traced_colours():
    d, o, a = sl.refraction_ns_case("slab")
    depth, bias, shadows = sl.REFRACTION_SETTING
    assert len(o) >= 64
    for mode in (REFRACT, FRESNEL):
        levels, recording = sl.recorded_levels()
        want = oracle_trace(d, o, a, depth, bias, mode, shadows=shadows, colours=recording)
        assert want["usable"].all() and want["refracted"] > 0 and want["depth_rays"][2] > 0
        table = sl.table_from_levels(d, levels, libm_shade)
        with ol.pow_mode(ol.POW_TABLE, table=table):
            again = oracle_trace(d, o, a, depth, bias, mode, shadows=shadows, colours=sl.ray_colours)
            misses = ol.pow_misses()
        assert misses == 0 and same_bits(again["rgb"], want["rgb"]).all()
        with ol.pow_mode(ol.POW_ONE):  # the exponents matter on these paths
            flat = oracle_trace(d, o, a, depth, bias, mode, shadows=shadows)["rgb"]
        n = int((~same_bits(flat, want["rgb"])).any(axis=1).sum())
        print(f"slab {MODE_NAME[mode]}: {len(o)} rays, levels {want['depth_rays'][:depth + 1]}, table of "
              f"{len(table[0])}, {n} rays depend on a power")
        assert n >= 16  # the case is not vacuous: paths whose colour a power decides


def test_edge_scene_trace_carries_nan_through_a_weight():
    """section 4's traced rays, chosen here: the mirror strip on the floor sends level-1 rays to surfaces
    whose colour is NaN, so a NaN colour times a weight reaches rays whose own colour is finite"""
    d, o, a = sl.edge_trace_rays()
    bias = float(F32(1e-4))
    c0 = oracle_trace(d, o, a, 0, bias)["rgb"]
    deep = oracle_trace(d, o, a, 2, bias)
    c2, counts = deep["rgb"], deep["depth_rays"]
    assert deep["usable"].all() and counts[1] >= 20, counts
    late = np.isnan(c2).any(axis=1) & np.isfinite(c0).all(axis=1)
    changed = ~same_bits(c2, c0).all(axis=1)
    print(f"edge trace: {len(o)} rays, levels {counts[:3]}, {int(changed.sum())} changed by level 1, {int(late.sum())} to NaN")
    assert late.sum() >= 3 and (changed & np.isfinite(c2).all(axis=1)).sum() >= 3
