"""Adaptive supersampling (Renderer.render_adaptive / adaptive_stats) against a composition of entry points
that are already pinned to the oracle:

    B = render(...)                      the 1-sample frame
    S = render_supersampled(..., spp)    every pixel with spp samples
    M = the 4-neighbour contrast rule of include/esctp1_rt.h, in numpy fp32 on B
    want = where(M, S, B)

Bits are compared (ray_oracle.assert_same); the u8 image is oracle_quantise(want), the mask is M, and the
stats count M.sum() pixels and spp * M.sum() samples.  B and S are rendered once per scene (and spp) and
shared by the cases.
"""
import ctypes as C
import os
import subprocess
import tarfile

import numpy as np
import pytest

import oracle_lib as ol
from ray_cases import CORNELL_EYE, CORNELL_LOOK
from ray_oracle import F32, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 97, 61  # odd: no multiple of the 64 x 8 tile or of a wave


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def mask_of(B, threshold):
    """M[h,w] = some 4-neighbour inside the frame and some channel has !(|B - B'| <= threshold), fp32"""
    thr = F32(threshold)
    with np.errstate(invalid="ignore"):
        eh = (~(np.abs(B[:, 1:] - B[:, :-1]) <= thr)).any(-1)
        ev = (~(np.abs(B[1:] - B[:-1]) <= thr)).any(-1)
    M = np.zeros(B.shape[:2], bool)
    M[:, 1:] |= eh
    M[:, :-1] |= eh
    M[1:] |= ev
    M[:-1] |= ev
    return M


def _scene(esc, name):
    """-> (product scene, eye, look, render keywords)"""
    if name == "cornell":
        return (ol.scene_to_product(ol.load_dump("CornellBox-Original")), CORNELL_EYE, CORNELL_LOOK,
                dict(face_mode=esc.ESC_FACE_HASH, seed=11))
    if name == "two":
        return ol.scene_to_product(ol.scene_two()), (0, 1, 3), (0, 1, 0), {}
    if name == "water":
        return ol.scene_to_product(ol.load_dump("CornellBox-Water")), CORNELL_EYE, CORNELL_LOOK, {}
    eye, look = esc.synthetic_view()
    return esc.Scene.synthetic(name), eye, look, dict(shadows=False)  # c2: primary rays only


_CACHE = {}


def composed(esc, r, name, w, h, spp):
    """uploads the scene; -> (camera, keywords, B, S), B and S rendered once and never written to"""
    sc, eye, look, kw = _scene(esc, name)
    r.upload(sc)
    cam = esc.Camera.for_image(eye, look, w, h)
    if (name, w, h) not in _CACHE:
        B = r.render(cam, w, h, **kw)
        B.setflags(write=False)
        _CACHE[(name, w, h)] = B
    if (name, w, h, spp) not in _CACHE:
        S = r.render_supersampled(cam, w, h, spp, **kw)
        S.setflags(write=False)
        _CACHE[(name, w, h, spp)] = S
    return cam, kw, _CACHE[(name, w, h)], _CACHE[(name, w, h, spp)]


def check_composition(esc, r, name, w, h, spp, threshold, vacuous_ok=False, **extra):
    cam, kw, B, S = composed(esc, r, name, w, h, spp)
    M = mask_of(B, threshold)
    n = int(M.sum())
    print(f"{name} {w}x{h} spp {spp} threshold {threshold}: {n} of {w * h} pixels masked")
    if not vacuous_ok:
        assert 0 < n < w * h, n
        assert (S.view(np.uint32)[M] != B.view(np.uint32)[M]).any(), "S == B on every masked pixel"
    want = np.where(M[..., None], S, B)
    img, u8, mask = r.render_adaptive(cam, w, h, spp, threshold, want_u8=True, want_mask=True, **kw, **extra)
    st = r.adaptive_stats()
    assert np.array_equal(mask, M.astype(np.uint8)), f"mask: {int((mask != M).sum())} pixels differ"
    assert_same(img, want, f"{name} spp {spp} threshold {threshold}")
    assert np.array_equal(u8, ol.oracle_quantise(want))
    assert st["pixels"] == w * h and st["refined_pixels"] == n and st["samples"] == spp * n, st
    return img, u8, mask, st


# ---- 1. composition ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.0, 0.05])
@pytest.mark.parametrize("spp", [4, 9, 16])
@pytest.mark.parametrize("name", ["cornell", "two", "water"])
def test_composition(esc, r, name, spp, threshold):
    _, _, _, st = check_composition(esc, r, name, W, H, spp, threshold)
    # every refined pixel sends spp primary rays; the shadow rays are those of the hits (x lights)
    assert 0 < st["hit_rays"] <= st["samples"], st
    assert st["shadow_rays"] % st["hit_rays"] == 0, st


# ---- 2. degenerate settings ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_degenerate_settings(esc, r):
    cam, kw, B, _ = composed(esc, r, "cornell", W, H, 4)
    # a threshold nothing exceeds: the frame itself
    img, u8, mask = r.render_adaptive(cam, W, H, 4, 1e30, want_u8=True, want_mask=True, **kw)
    st = r.adaptive_stats()
    assert mask_of(B, 1e30).sum() == 0 and mask.sum() == 0
    assert_same(img, B, "threshold 1e30")
    assert np.array_equal(u8, ol.oracle_quantise(B))
    assert st["refined_pixels"] == 0 and st["samples"] == 0 and st["hit_rays"] == 0, st
    # spp == 1: the frame itself, though the masked pixels are still refined
    img = r.render_adaptive(cam, W, H, 1, 0.05, **kw)
    st = r.adaptive_stats()
    n = int(mask_of(B, 0.05).sum())
    assert_same(img, B, "spp 1")
    assert n > 0 and st["refined_pixels"] == n and st["samples"] == n, st
    # two calls with the same arguments give identical bytes
    a = r.render_adaptive(cam, W, H, 9, 0.05, want_u8=True, want_mask=True, **kw)
    b = r.render_adaptive(cam, W, H, 9, 0.05, want_u8=True, want_mask=True, **kw)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # the smallest frame: no pixel masked (the box's four corner rays miss), and all four (`two`)
    assert check_composition(esc, r, "cornell", 2, 2, 4, 0.0, vacuous_ok=True)[3]["refined_pixels"] == 0
    assert check_composition(esc, r, "two", 2, 2, 4, 0.05, vacuous_ok=True)[3]["refined_pixels"] == 4


# ---- 3. bands -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bands_do_not_change_the_image(esc, r):
    # 61 rows are no multiple of 5: band boundaries fall inside edge regions, the last band is short
    whole = check_composition(esc, r, "cornell", W, H, 4, 0.05)
    for band_rows in (5, 61, 1, 1000):
        got = check_composition(esc, r, "cornell", W, H, 4, 0.05, band_rows=band_rows)
        for x, y in zip(whole[:3], got[:3]):
            assert x.tobytes() == y.tobytes(), band_rows
        # (exact_tests is left out: the sweeps open groups per wavefront, so it follows the list's order)
        for k in ("pixels", "refined_pixels", "samples", "hit_rays", "shadow_rays"):
            assert got[3][k] == whole[3][k], (band_rows, k)


# ---- 4. the sphere path -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sphere_scene(esc, r):
    st = check_composition(esc, r, "c2", 160, 90, 4, 0.05)[3]
    assert st["hit_rays"] > 0 and st["shadow_rays"] == 0, st


# ---- 5. bad arguments ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments(esc, r):
    import torch
    from esctp1raytracer_amd import _capi
    cam, kw, _, _ = composed(esc, r, "cornell", W, H, 4)
    with pytest.raises(esc.EscError, match="esc_render_adaptive"):
        r.render_adaptive(cam, W, H, 3, 0.05)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(esc.EscError, match="esc_render_adaptive.*threshold"):
            r.render_adaptive(cam, W, H, 4, bad)
    with pytest.raises(esc.EscError, match="esc_render_adaptive.*band_rows"):
        r.render_adaptive(cam, W, H, 4, 0.05, band_rows=-1)
    dev = torch.device("cuda", r.device)
    img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    o = _capi.esc_render_options()
    o.shadows = 1
    a = _capi.esc_adaptive_options(4, 0.05, 0, 1)
    with pytest.raises(esc.EscError, match="esc_render_adaptive.*reserved"):
        _capi.check(r._lib.esc_render_adaptive(r._h, C.byref(cam.c), W, H, C.byref(o), C.byref(a),
                                               C.c_void_p(img.data_ptr()), None, None))
    a.reserved = 0
    _capi.check(r._lib.esc_render_adaptive(r._h, C.byref(cam.c), W, H, C.byref(o), C.byref(a),
                                           C.c_void_p(img.data_ptr()), None, None))
    r.synchronize()


# ---- 6. no interference -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adaptive_leaves_the_other_calls_alone(esc):
    r = esc.Renderer(0)
    sc, eye, look, kw = _scene(esc, "cornell")
    r.upload(sc)
    cam = esc.Camera.for_image(eye, look, W, H)
    f1, f81 = r.render(cam, W, H, want_u8=True, **kw)
    s1 = r.render_supersampled(cam, W, H, 4, **kw)
    st1 = r.shade_stats()
    cam2 = esc.Camera.for_image(eye, (0.3, 0.8, 0), 64, 33)
    r.render_adaptive(cam2, 64, 33, 9, 0.02, **kw)
    assert r.adaptive_stats()["refined_pixels"] > 0
    assert r.shade_stats() == st1
    f2, f82 = r.render(cam, W, H, want_u8=True, **kw)
    s2 = r.render_supersampled(cam, W, H, 4, **kw)
    assert f1.tobytes() == f2.tobytes() and f81.tobytes() == f82.tobytes()
    assert s1.tobytes() == s2.tobytes()
    assert r.shade_stats() == st1
    r.close()


@pytest.mark.gpu
def test_adaptive_on_a_torch_stream(esc):
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=s)
    sc, eye, look, kw = _scene(esc, "cornell")
    r.upload(sc)
    cam = esc.Camera.for_image(eye, look, W, H)
    B = r.render(cam, W, H, **kw)
    S = r.render_supersampled(cam, W, H, 4, **kw)
    M = mask_of(B, 0.05)
    with torch.cuda.stream(s):
        got, mask = r.render_adaptive(cam, W, H, 4, 0.05, want_mask=True, **kw)
    assert np.array_equal(mask, M.astype(np.uint8))
    assert_same(got, np.where(M[..., None], S, B), "torch stream")
    r.close()


# ---- 7. the viewer ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_viewer_adaptive(esc, r, tmp_path):
    viewer = os.path.join(ROOT, "bin", "ESCViewer2021")
    obj_dir = tmp_path / "models"
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as tf:
        tf.extractall(obj_dir)
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(obj_dir) for f in fs if f == "CornellBox-Original.obj"]
    assert objs
    w, h = 64, 48
    ppm = tmp_path / "adaptive.ppm"
    p = subprocess.run([viewer, "-m", objs[0], "-v", "0,1,3.5", "-l", "0,1,0", "-w", f"{w},{h}", "--spp", "4",
                        "--adaptive", "0.05", "-o", str(ppm)], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(objs[0]))
    assert p.returncode == 0, p.stderr
    r.upload(esc.Scene.load_obj(objs[0]))
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, w, h)
    img = r.render_adaptive(cam, w, h, 4, 0.05, face_mode=esc.ESC_FACE_HASH, seed=0)
    assert 0 < r.adaptive_stats()["refined_pixels"] < w * h
    mine = tmp_path / "mine.ppm"
    esc.write_ppm(mine, img)
    assert ppm.read_bytes() == mine.read_bytes()
    # and it is neither the plain frame nor the fully supersampled one
    plain = tmp_path / "plain.ppm"
    esc.write_ppm(plain, r.render(cam, w, h, face_mode=esc.ESC_FACE_HASH, seed=0))
    assert ppm.read_bytes() != plain.read_bytes()
