"""Thin-lens camera on the GPU (Renderer.lens_rays / render_lens / set_lens_table) against the numpy
restatement of tests/lens_lib.py, bit for bit.  There is no tolerance in this file.  Cameras, frames and lens
settings are those of tests/lens_cases.py, whose condition is asserted on the CPU (test_lens_cpu.py) and again
here before a case is compared.  The frames are pinned by composition: the restatement's rays go through
Renderer.trace, which tests/test_trace_rays.py and tests/test_transmission.py hold to the oracle."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
import lens_cases as lc
import lens_lib as ll
import oracle_lib as ol
from ray_cases import product
from ray_oracle import F32, assert_same

pytestmark = pytest.mark.gpu

PAIRS = [(c, W, H) for c in lc.CAMERAS for W, H in lc.FRAMES]
IDS = [f"{c}-{W}x{H}" for c, W, H in PAIRS]
FW, FH = ac.FRAME_W, ac.FRAME_H  # 16 x 12
SEED = 77


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    rr.uploaded = None
    yield rr
    rr.close()


def use(r, name):
    if r.uploaded != name:
        r.upload(ol.scene_to_product(ac.scene(name)[0]))
        r.uploaded = name


def on_device(a):
    """a numpy array as a device tensor, ready for the renderer's stream"""
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda:0")  # a copy: the cases' arrays are read-only
    torch.cuda.current_stream(t.device).synchronize()
    return t


def host(r, *tensors):
    r.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def last_error(r):
    return r._lib.esc_last_error().decode("utf-8", "replace")


# ---- 1. rays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", PAIRS, ids=IDS)
def test_lens_rays_match_the_restatement(r, name, W, H):
    cam = lc.camera(name, W, H)[0]
    shape = None
    for c in lc.cases(name, W, H):
        lc.check_condition(c)
        if shape != (c["S"], c["K"]):
            shape = (c["S"], c["K"])
            r.set_lens_table(lc.table(*shape))
            assert r.lens_table_shape == shape
        offs = lc.case_offsets(c)
        o, d = host(r, *r.lens_rays(cam, W, H, aperture=c["aperture"], focus_dist=c["focus_dist"], sample=c["k"],
                                    seed=lc.LENS_SEED, rows=c["rows"], offsets=None if offs is None else on_device(offs)))
        wo, wd = lc.want(c)
        assert_same(o, wo, f"{lc.key(c)} origins")
        assert_same(d, wd, f"{lc.key(c)} dirs")


def test_degenerate_tables(r):
    """a table whose only point is the lens centre: the pinhole origin, and the restatement's directions
    (p*focus_dist normalised is not always normalize(p) in bits); a point on the rim; a point outside the disk
    is taken as given"""
    W, H = 33, 9
    cam, ext, dist = lc.camera("c2_200", W, H)
    pix = lc.pixels(W, H, None)
    ap = float(F32(0.1 * ext))
    for tab in (np.zeros((1, 1, 2), F32), np.array([[[1.0, 0.0]], [[0.0, -1.0]]], F32),
                np.array([[[3.0, -2.0], [0.5, 0.5]]], F32)):
        r.set_lens_table(tab)
        k = tab.shape[1] - 1
        o, d = host(r, *r.lens_rays(cam, W, H, aperture=ap, focus_dist=dist, sample=k, seed=9))
        wo, wd = ll.lens_rays(cam.vectors(), W, H, pix, ap, dist, tab, k, 9)
        assert np.isfinite(wo).all() and np.isfinite(wd).all()
        assert_same(o, wo, "origins")
        assert_same(d, wd, "dirs")
        if not tab.any():
            assert_same(o, np.tile(cam.vectors()["origin"], (W * H, 1)), "the centre of the lens is the pinhole")


# ---- 2. aperture 0 is the pinhole camera -------------------------------------------------------------------
def test_aperture_zero_rays_are_camera_rays(esc):
    rr = esc.Renderer(0)  # no table: a pinhole needs none
    try:
        assert rr.lens_table_shape == (0, 0)
        for name, W, H in PAIRS:
            cam = lc.camera(name, W, H)[0]
            for rows in lc.ROWS:
                n = len(lc.pixels(W, H, rows))
                for offs in (None, on_device(lc.offsets(n))):
                    got = host(rr, *rr.lens_rays(cam, W, H, aperture=0.0, focus_dist=0.5, sample=3, rows=rows, offsets=offs))
                    ref = host(rr, *rr.camera_rays(cam, W, H, rows=rows, offsets=offs))
                    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), (name, W, H, rows)
    finally:
        rr.close()


def sphere_scene():
    d = dict(ol.load_dump("CornellBox-Sphere"))
    d["transmission"] = {g: np.array([0.8, 0.9, 0.7, 1.5], F32) for g in range(1, len(d["geometry"]), 2)}
    d["sphere_transmission"] = {}
    return product(d)


@pytest.mark.parametrize("transmission", ["off", "refract"])
@pytest.mark.parametrize("max_depth", [0, 2])
@pytest.mark.parametrize("spp", [1, 4])
def test_aperture_zero_frames_are_render_traced(esc, spp, max_depth, transmission):
    rr = esc.Renderer(0)  # no table
    try:
        rr.upload(sphere_scene())
        cam = ac.frame_camera("CornellBox-Sphere")
        kw = dict(spp=spp, max_depth=max_depth, bias=1e-3, transmission=transmission, seed=SEED, want_u8=True)
        want, want8 = rr.render_traced(cam, FW, FH, **kw)
        st, tr = rr.trace_stats(), rr.transmit_stats()
        got, got8 = rr.render_lens(cam, FW, FH, aperture=0.0, focus_dist=1.0, lens_seed=3, **kw)
        assert got.tobytes() == want.tobytes() and got8.tobytes() == want8.tobytes()
        assert rr.trace_stats() == st and rr.transmit_stats() == tr
        assert st["depth_rays"][0] == spp * FW * FH
        if transmission == "refract" and max_depth:
            assert tr["refracted"] > 0, "no ray was refracted: the mode was not exercised"
        if max_depth == 0 and transmission == "off":
            ss = rr.render_supersampled(cam, FW, FH, spp, seed=SEED)
            assert got.tobytes() == ss.tobytes()
    finally:
        rr.close()


# ---- 3. frames by composition ------------------------------------------------------------------------------
def lens_setting(name):
    """-> (aperture, focus_dist): 5 % of the extent, focused on the look-at point"""
    _, ext, dist = lc.camera(name, FW, FH)
    return float(F32(0.05 * ext)), dist


def composed(r, name, spp, n, table, face_mode, max_depth, bias):
    """sum over k of Renderer.trace on the restatement's rays of sample k, in order, then / float(spp)"""
    cam = lc.camera(name, FW, FH)[0]
    ap, fd = lens_setting(name)
    pix = lc.pixels(FW, FH, None)
    acc = None
    for k in range(spp):
        o, d = ll.lens_rays(cam.vectors(), FW, FH, pix, ap, fd, table, k, lc.LENS_SEED, ll.grid_offset(k, n))
        assert np.isfinite(o).all() and np.isfinite(d).all()
        rgb = r.trace(o.copy(), d.copy(), max_depth=max_depth, bias=bias, pixel_base=0, seed=SEED + k,
                      face_mode=face_mode)["rgb"]
        acc = (np.zeros_like(rgb) + rgb).astype(F32) if acc is None else (acc + rgb).astype(F32)
    return (acc / F32(spp)).astype(F32).reshape(FH, FW, 3)


@pytest.mark.parametrize("face", ["fixed", "hash"])
@pytest.mark.parametrize("max_depth", [0, 1])
@pytest.mark.parametrize("name", ["CornellBox-Original", "c2_200"])
def test_frames_equal_the_composition(esc, r, name, max_depth, face):
    use(r, name)
    tab = lc.table(3, 16)
    r.set_lens_table(tab)
    face_mode = esc.ESC_FACE_FIXED if face == "fixed" else esc.ESC_FACE_HASH
    cam = lc.camera(name, FW, FH)[0]
    ap, fd = lens_setting(name)
    want = composed(r, name, 4, 2, tab, face_mode, max_depth, 1e-3)
    got, got8 = r.render_lens(cam, FW, FH, spp=4, aperture=ap, focus_dist=fd, lens_seed=lc.LENS_SEED, max_depth=max_depth,
                              bias=1e-3, seed=SEED, face_mode=face_mode, want_u8=True)
    st = r.trace_stats()
    assert_same(got, want, f"{name} depth {max_depth} {face}")
    assert np.array_equal(got8, esc.quantise(want).reshape(FH, FW, 3))
    assert st["depth_rays"][0] == 4 * FW * FH, st
    assert float((want.max(axis=-1) > 0).mean()) > 0.25, "a mostly black frame pins little"


# ---- 4. the lens does something, and the same thing twice --------------------------------------------------
@pytest.mark.parametrize("name", ["CornellBox-Original", "c2_200"])
def test_a_lens_blurs_and_is_deterministic(r, name):
    use(r, name)
    r.set_lens_table(lc.table(3, 16))
    cam = lc.camera(name, FW, FH)[0]
    ap, fd = lens_setting(name)
    kw = dict(spp=4, focus_dist=fd * 0.25, lens_seed=lc.LENS_SEED, max_depth=1, bias=1e-3, seed=SEED)
    pin = r.render_lens(cam, FW, FH, aperture=0.0, **kw)
    a = r.render_lens(cam, FW, FH, aperture=ap, **kw)
    b = r.render_lens(cam, FW, FH, aperture=ap, **kw)
    assert a.tobytes() == b.tobytes(), "two calls with the same arguments differ"
    assert a.tobytes() != pin.tobytes(), "the aperture changed nothing"
    c = r.render_lens(cam, FW, FH, aperture=ap, **dict(kw, lens_seed=lc.LENS_SEED + 1))
    assert c.tobytes() != a.tobytes(), "the lens seed changed nothing"


# ---- 5. validation -----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written(esc, r):
    import torch
    from esctp1raytracer_amd import _capi
    use(r, "c2_200")
    r.set_lens_table(lc.table(1, 4))
    W, H = 17, 13
    cam = lc.camera("c2_200", W, H)[0]
    lib, h, cc = r._lib, r._h, C.byref(cam.c)
    o = torch.full((W * H, 3), 7.0, dtype=torch.float32, device="cuda:0")
    d = torch.full((W * H, 3), 7.0, dtype=torch.float32, device="cuda:0")
    img = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda:0")
    u8 = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    po, pd, pi, pu = (C.c_void_p(t.data_ptr()) for t in (o, d, img, u8))
    opts = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO)
    nan, inf = float("nan"), float("inf")

    def lens(ap=0.5, fd=2.0, res=(0, 0)):
        return _capi.esc_lens_options(ap, fd, 0, (C.c_int32 * 2)(*res))

    def topt(depth=1, bias=1e-3, mode=0, res=0):
        return _capi.esc_trace_options(depth, bias, mode, res)

    def rays(lo=None, sample=0, po=po, pd=pd, poff=None, cam=cc, rows=(0, H), W=W):
        return lib.esc_lens_rays(h, cam, W, H, rows[0], rows[1], poff, C.byref(lo) if lo else None, sample, po, pd)

    def frame(lo=None, spp=4, to=None, pi=pi, pu=pu, o_=opts, cam=cc, W=W):
        return lib.esc_render_lens(h, cam, W, H, spp, C.byref(o_) if o_ else None, C.byref(to) if to else None,
                                   C.byref(lo) if lo else None, pi, pu)

    bad_lens = [("aperture", lens(ap=-0.5)), ("aperture", lens(ap=nan)), ("aperture", lens(ap=inf)),
                ("focus_dist", lens(fd=0.0)), ("focus_dist", lens(fd=-1.0)), ("focus_dist", lens(fd=nan)),
                ("focus_dist", lens(fd=inf)), ("reserved", lens(res=(1, 0))), ("reserved", lens(res=(0, -1)))]
    calls = []
    for word, lo in bad_lens:
        calls.append((f"lens_rays {word}", "esc_lens_rays", word, lambda lo=lo: rays(lo)))
        calls.append((f"render_lens {word}", "esc_render_lens", word, lambda lo=lo: frame(lo, to=topt())))
    # a pinhole's other fields are checked too
    calls.append(("lens_rays pinhole focus", "esc_lens_rays", "focus_dist", lambda: rays(lens(ap=0.0, fd=0.0))))
    calls.append(("render_lens pinhole reserved", "esc_render_lens", "reserved", lambda: frame(lens(ap=0.0, res=(0, 2)), to=topt())))
    calls += [
        ("sample beyond the table", "esc_lens_rays", "sample", lambda: rays(lens(), sample=4)),
        ("negative sample", "esc_lens_rays", "sample", lambda: rays(lens(), sample=-1)),
        ("spp beyond the table", "esc_render_lens", "spp", lambda: frame(lens(), spp=9, to=topt())),
        ("null lens options (rays)", "esc_lens_rays", "lens", lambda: rays(None)),
        ("null lens options (frame)", "esc_render_lens", "lens", lambda: frame(None, to=topt())),
        ("null origins", "esc_lens_rays", "required", lambda: rays(lens(), po=None)),
        ("null dirs", "esc_lens_rays", "required", lambda: rays(lens(), pd=None)),
        ("misaligned origins", "esc_lens_rays", "align", lambda: rays(lens(), po=C.c_void_p(o.data_ptr() + 2))),
        ("misaligned dirs", "esc_lens_rays", "align", lambda: rays(lens(), pd=C.c_void_p(d.data_ptr() + 1))),
        ("misaligned offsets", "esc_lens_rays", "align", lambda: rays(lens(), poff=C.c_void_p(d.data_ptr() + 2))),
        ("null camera", "esc_lens_rays", "cam", lambda: rays(lens(), cam=None)),
        ("rows", "esc_lens_rays", "row_begin", lambda: rays(lens(), rows=(5, 4))),
        ("rows past the frame", "esc_lens_rays", "row_begin", lambda: rays(lens(), rows=(0, H + 1))),
        ("W = 1", "esc_lens_rays", "W,H", lambda: rays(lens(), W=1)),
        # esc_render_traced_ex's argument errors
        ("null trace options", "esc_render_lens", "trace options", lambda: frame(lens(), to=None)),
        ("spp 3", "esc_render_lens", "spp", lambda: frame(lens(), spp=3, to=topt())),
        ("spp 0", "esc_render_lens", "spp", lambda: frame(lens(), spp=0, to=topt())),
        ("max_depth 17", "esc_render_lens", "max_depth", lambda: frame(lens(), to=topt(depth=17))),
        ("bias", "esc_render_lens", "bias", lambda: frame(lens(), to=topt(bias=-1.0))),
        ("transmission 7", "esc_render_lens", "transmission", lambda: frame(lens(), to=topt(mode=7))),
        ("trace reserved", "esc_render_lens", "reserved", lambda: frame(lens(), to=topt(res=1))),
        ("null image", "esc_render_lens", "", lambda: frame(lens(), to=topt(), pi=None)),
        ("misaligned image", "esc_render_lens", "align", lambda: frame(lens(), to=topt(), pi=C.c_void_p(img.data_ptr() + 2))),
        ("null options", "esc_render_lens", "", lambda: frame(lens(), to=topt(), o_=None)),
        ("null camera (frame)", "esc_render_lens", "", lambda: frame(lens(), to=topt(), cam=None)),
        ("W = 1 (frame)", "esc_render_lens", "W,H", lambda: frame(lens(), to=topt(), W=1)),
    ]
    for what, fn, word, call in calls:
        rc = call()
        assert rc == _capi.ESC_ERR_INVALID, f"{what}: rc {rc}"
        msg = last_error(r)
        assert fn in msg and word in msg, f"{what}: {msg!r}"
    # no table while aperture > 0; a pinhole still renders
    r.set_lens_table(None)
    assert r.lens_table_shape == (0, 0)
    for what, fn, call in (("rays", "esc_lens_rays", lambda: rays(lens())),
                           ("frame", "esc_render_lens", lambda: frame(lens(), to=topt()))):
        assert call() == _capi.ESC_ERR_INVALID, what
        assert fn in last_error(r) and "no lens table" in last_error(r)
    # a scene is needed by the frame, not by the rays
    fresh = esc.Renderer(0)
    try:
        fresh.set_lens_table(lc.table(1, 4))
        assert lib.esc_render_lens(fresh._h, cc, W, H, 4, C.byref(opts), C.byref(topt()), C.byref(lens()), pi, pu) == -1
        assert "esc_render_lens" in last_error(r) and "no scene" in last_error(r)
        fresh.synchronize()
    finally:
        fresh.close()
    r.synchronize()
    for t in (o, d, img):
        assert bool((t == 7.0).all()), "a refused call wrote into an output"
    assert bool((u8 == 7).all())
    # and the same buffers take a good call
    r.set_lens_table(lc.table(1, 4))
    assert rays(lens(), sample=3) == 0 and frame(lens(), to=topt()) == 0, last_error(r)
    r.synchronize()
    assert not bool((o == 7.0).all()) and not bool((img == 7.0).all())


def test_set_lens_table_refuses_bad_shapes(esc, r):
    from esctp1raytracer_amd import _capi
    r.set_lens_table(lc.table(3, 16))
    t = np.zeros(2 * 65 * 65, np.float32)
    for S, K, p in ((0, 4, t), (4, 4, None), (65, 4, t), (4, 65, t), (-1, 4, t), (4, 0, t)):
        rc = r._lib.esc_set_lens_table(r._h, S, K, None if p is None else esc._fp(p))
        assert rc == _capi.ESC_ERR_INVALID and "esc_set_lens_table" in last_error(r), (S, K)
        assert r.lens_table_shape == (3, 16), "a refused call replaced the table"
    with pytest.raises(ValueError):
        r.set_lens_table(np.zeros((3, 4, 3), F32))


# ---- 6. ownership ------------------------------------------------------------------------------------------
def test_the_table_survives_uploads_and_is_freed_with_the_context(esc):
    base = esc.live_device_allocations()
    rr = esc.Renderer(0)
    W, H = 33, 9
    cam, ext, dist = lc.camera("c2_200", W, H)
    ap = float(F32(0.1 * ext))
    tab = lc.table(3, 16)
    created = esc.live_device_allocations()
    rr.set_lens_table(tab)
    with_table = esc.live_device_allocations()
    assert with_table[0] == created[0] + 1 and with_table[1] == created[1] + tab.nbytes
    want = ll.lens_rays(cam.vectors(), W, H, lc.pixels(W, H, None), ap, dist, tab, 15, 4)
    for name in ("c2_200", "CornellBox-Original"):
        rr.upload(ol.scene_to_product(ac.scene(name)[0]))
        assert rr.lens_table_shape == (3, 16)
        o, d = host(rr, *rr.lens_rays(cam, W, H, aperture=ap, focus_dist=dist, sample=15, seed=4))
        assert_same(o, want[0], "origins after an upload")
        assert_same(d, want[1], "dirs after an upload")
    # a new table replaces the old one: one buffer, not two
    held = esc.live_device_allocations()
    rr.set_lens_table(lc.table(1, 4))
    assert rr.lens_table_shape == (1, 4)
    now = esc.live_device_allocations()
    assert now[0] == held[0] and now[1] == held[1] - tab.nbytes + 1 * 4 * 2 * 4
    rr.set_lens_table(None)
    assert rr.lens_table_shape == (0, 0)
    assert esc.live_device_allocations() == (held[0] - 1, held[1] - tab.nbytes)
    rr.set_lens_table(lc.table(2, 9))  # a context that dies with a table frees it
    rr.close()
    assert esc.live_device_allocations() == base
