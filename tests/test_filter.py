"""The edge-stopping a-trous filter on the GPU (Renderer.filter_guided / filter_stats) against the numpy
restatement of tests/filter_lib.py: images bit for bit, the four stats exactly.  There is no tolerance in this
file.  The cases are those of tests/filter_cases.py, whose conditions are asserted on the CPU
(test_filter_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
import filter_cases as fc
import filter_lib as fl
import oracle_lib as ol
from ray_oracle import F32, FLT_MAX, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("pixels", "hit_pixels", "taps_tested", "taps_accepted")
SKY = ((0.2, 0.4, 1.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1))


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)  # the filter needs no scene
    yield rr
    rr.close()


def assert_filtered(r, got, want, what):
    out, st = want
    assert got.shape == out.shape and got.dtype == np.float32
    assert_same(got, out, what)
    gs = r.filter_stats()
    assert gs == {k: st[k] for k in STATS}, (what, gs, st)


# ---- every case --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,k", fc.TRACED, ids=fc.TRACED_IDS)
def test_traced_case_matches_the_restatement(r, name, k):
    g = fc.traced_guides(name)
    for ch in (1, 3):
        for same in (True, False):
            got = r.filter_guided(fc.traced_image(name, k, ch), g, iterations=fc.ITER_A, normal_cos=fc.NORMAL_COS,
                                  plane_dist=fc.traced_plane(name), same_object=same)
            assert_filtered(r, got, fc.traced_want(name, k, ch, same), f"{name} setting {k} channels {ch} same {same}")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,L", fc.SYNTHETIC, ids=fc.SYNTHETIC_IDS)
def test_synthetic_case_matches_the_restatement(r, W, H, L):
    g = fc.synthetic(W, H)
    for ch in (1, 3):
        for same in (True, False):
            got = r.filter_guided(g[f"image{ch}"], g, iterations=L, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE,
                                  same_object=same)
            assert_filtered(r, got, fc.synthetic_want(W, H, L, ch, same), f"{W}x{H} L {L} channels {ch} same {same}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", range(1, 9))
def test_every_iteration_count(r, L):
    """both parities of the alternation between the output and the scratch image"""
    W, H = 33, 19
    g = fc.synthetic(W, H)
    for ch in (1, 3):
        got = r.filter_guided(g[f"image{ch}"], g, iterations=L, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
        assert_filtered(r, got, fc.synthetic_want(W, H, L, ch), f"L {L} channels {ch}")


# ---- invariants on the device ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ones_misses_and_stops_off(r):
    W, H, L = 65, 9, 5
    g = fc.synthetic(W, H)
    for ch in (1, 3):
        ones = np.ones((H, W) if ch == 1 else (H, W, 3), F32)
        got = r.filter_guided(ones, g, iterations=L, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
        assert got.tobytes() == ones.tobytes()
        img = g[f"image{ch}"]
        miss = dict(g, geom=np.full((H, W), -1, np.int32), prim=np.full((H, W), -1, np.int32))
        got = r.filter_guided(img, miss, iterations=L, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
        assert got.tobytes() == img.tobytes()
        st = r.filter_stats()
        assert st == {"pixels": W * H, "hit_pixels": 0, "taps_tested": 0, "taps_accepted": 0}, st
    flat = {"normal": np.tile(np.array([0, 0, 1], F32), (H, W, 1)), "position": np.nan_to_num(g["position"]),
            "geom": np.zeros((H, W), np.int32), "prim": np.arange(H * W, dtype=np.int32).reshape(H, W)}
    for pd in (float(FLT_MAX), float("inf")):
        got = r.filter_guided(g["image1"], flat, iterations=L, normal_cos=float("-inf"), plane_dist=pd, same_object=False)
        want = fl.atrous(g["image1"], flat, L, -np.inf, pd, same_object=False)
        assert_filtered(r, got, want, f"stops off, plane {pd}")
        st = r.filter_stats()
        assert st["taps_accepted"] == st["taps_tested"] > 0 and st["hit_pixels"] == W * H, st
    # NaN and infinite image values spread to whatever accepts them, as the restatement says
    img = g["image1"].copy()
    img[4, 30], img[2, 50] = np.nan, np.inf
    got = r.filter_guided(img, g, iterations=3, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
    want = fl.atrous(img, g, 3, fc.NORMAL_COS, fc.SYN_PLANE)
    assert np.isnan(want[0]).sum() > 1
    assert_filtered(r, got, want, "NaN and inf in the image")


@pytest.mark.gpu
def test_device_tensors_and_out(esc, r):
    import torch
    W, H, L = 33, 19, 2
    g = fc.synthetic(W, H)
    dev = torch.device("cuda", r.device)
    guides = {k: torch.from_numpy(np.array(g[k])).to(dev) for k in ("normal", "position", "geom", "prim")}
    img = torch.from_numpy(np.array(g["image3"])).to(dev)
    out = torch.empty_like(img)
    torch.cuda.current_stream(dev).synchronize()
    res = r.filter_guided(img, guides, iterations=L, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE, out=out)
    r.synchronize()
    assert res is out
    assert_filtered(r, out.cpu().numpy(), fc.synthetic_want(W, H, L, 3), "device tensors")
    assert img.cpu().numpy().tobytes() == g["image3"].tobytes()  # the input is left alone


# ---- GPU guides --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.SCENES)
def test_render_gbuffer_guides_the_filter(esc, name):
    r = esc.Renderer(0)
    r.upload(ol.scene_to_product(ac.scene(name)[0]))
    g = r.render_gbuffer(ac.frame_camera(name), ac.FRAME_W, ac.FRAME_H)
    for ch in (1, 3):
        got = r.filter_guided(fc.traced_image(name, 1, ch), g, iterations=fc.ITER_A, normal_cos=fc.NORMAL_COS,
                              plane_dist=fc.traced_plane(name))
        assert_filtered(r, got, fc.traced_want(name, 1, ch), f"{name} GPU guides channels {ch}")
    r.close()


# ---- bad arguments -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments(esc, r):
    import torch
    from esctp1raytracer_amd import _capi
    W, H = 33, 19
    g = fc.synthetic(W, H)
    img = g["image1"]
    good = dict(iterations=3, normal_cos=0.9, plane_dist=0.05)
    for key, bad, word in (("iterations", 0, "iterations"), ("iterations", 9, "iterations"), ("iterations", -1, "iterations"),
                           ("normal_cos", float("nan"), "normal_cos"), ("plane_dist", float("nan"), "plane_dist"),
                           ("plane_dist", -0.5, "plane_dist")):
        with pytest.raises(esc.EscError, match="esc_filter_guided.*" + word):
            r.filter_guided(img, g, **dict(good, **{key: bad}))
    dev = torch.device("cuda", r.device)
    t = {k: torch.from_numpy(np.array(g[k])).to(dev) for k in ("normal", "position", "geom", "prim", "image1")}
    out = torch.empty_like(t["image1"])
    torch.cuda.current_stream(dev).synchronize()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def call(W_=W, H_=H, ch=1, src=p(t["image1"]), dst=p(out), opts=_capi.esc_filter_options(3, 0.9, 0.05, 1), normal=p(t["normal"])):
        return r._lib.esc_filter_guided(r._h, W_, H_, ch, src, normal, p(t["position"]), p(t["geom"]), p(t["prim"]),
                                        None if opts is None else C.byref(opts), dst)
    assert call() == _capi.ESC_OK
    r.synchronize()
    for kw, word in ((dict(dst=p(t["image1"])), "d_out must not be d_in"), (dict(ch=2), "channels"), (dict(ch=4), "channels"),
                     (dict(W_=0), "W,H"), (dict(H_=0), "W,H"), (dict(src=None), "required"), (dict(dst=None), "required"),
                     (dict(normal=None), "required"), (dict(opts=None), "opts"),
                     (dict(opts=_capi.esc_filter_options(3, 0.9, 0.05, 1, (C.c_int32 * 2)(0, 1))), "reserved"),
                     (dict(opts=_capi.esc_filter_options(3, 0.9, 0.05, 2)), "same_object")):
        with pytest.raises(esc.EscError, match="esc_filter_guided.*" + word):
            _capi.check(call(**kw))
    # the renderer still works
    got = r.filter_guided(img, g, iterations=3, normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
    assert_filtered(r, got, fc.synthetic_want(W, H, 3, 1), "after the errors")


# ---- scratch -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scratch_growth_and_release(esc):
    b0 = esc.live_device_allocations()
    r1 = esc.Renderer(0)
    small, big = fc.synthetic(33, 19), fc.synthetic(130, 70)
    kw = dict(normal_cos=fc.NORMAL_COS, plane_dist=fc.SYN_PLANE)
    a = r1.filter_guided(small["image3"], small, iterations=3, **kw)
    m1 = esc.live_device_allocations()
    b = r1.filter_guided(big["image3"], big, iterations=6, **kw)  # the scratch grows
    m2 = esc.live_device_allocations()
    c = r1.filter_guided(small["image1"], small, iterations=3, **kw)  # and is kept
    assert esc.live_device_allocations() == m2 and m2 != m1
    r2 = esc.Renderer(0)
    assert b.tobytes() == r2.filter_guided(big["image3"], big, iterations=6, **kw).tobytes()
    assert_same(a, fc.synthetic_want(33, 19, 3, 3)[0], "small before")
    assert_same(b, fc.synthetic_want(130, 70, 6, 3)[0], "big after small")
    assert_same(c, fc.synthetic_want(33, 19, 3, 1)[0], "small after big")
    r1.close()
    r2.close()
    assert esc.live_device_allocations() == b0


# ---- the viewer --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_viewer_denoise(esc, tmp_path):
    viewer = os.path.join(ROOT, "bin", "ESCViewer2021")
    obj = os.path.join(ROOT, "tests", "golden", "scenes", "one.obj")
    w, h = 32, 24
    sky = "/".join(",".join(repr(c) for c in col) for col in SKY)
    base = [viewer, "-m", obj, "-w", f"{w},{h}", "--sky", sky, "--ao", "8", "--ao-radius", "0.5", "--skylight"]
    out = {}
    for what, extra in (("denoise", ["--denoise", "3"]), ("plain", [])):
        ppm = tmp_path / (what + ".ppm")
        p = subprocess.run(base + extra + ["-o", str(ppm)], capture_output=True, text=True, timeout=300,
                           cwd=os.path.dirname(obj))
        assert p.returncode == 0, p.stderr
        out[what] = ppm.read_bytes()
    # the Python composition with the viewer's defaults (test_skylight.py), normal 0.9 and plane radius / 4
    r = esc.Renderer(0)
    r.upload(esc.Scene.load_obj(obj))
    r.set_ambient_table(esc.ambient_table(16, 8, 0))
    r.set_environment(esc.environment_sky(64, *SKY))
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), w, h)
    img = r.render_traced(cam, w, h, max_depth=0, bias=1e-4, face_mode=esc.ESC_FACE_HASH, seed=0)
    f = r.render_skylight(cam, w, h, radius=0.5, bias=1e-4, seed=0)
    g = r.render_gbuffer(cam, w, h)
    light = r.filter_guided(f["light"], g, iterations=3, normal_cos=0.9, plane_dist=0.5 / 4)
    st = r.filter_stats()
    assert 0 < st["taps_accepted"] < st["taps_tested"] and light.tobytes() != f["light"].tobytes(), st
    mine = tmp_path / "mine.ppm"
    esc.write_ppm(mine, r.add_light(img, light))
    assert out["denoise"] == mine.read_bytes()
    assert out["denoise"] != out["plain"]
    r.close()
