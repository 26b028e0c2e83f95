"""The G-buffer on the GPU (Renderer.gbuffer / gbuffer_rays / render_gbuffer / gbuffer_stats) against the numpy
restatement filter_lib.gbuffer: floats bit for bit, ids exactly, t / geom / prim byte for byte with ambient's and
intersect's.  There is no tolerance in this file.  Scenes and rays are those of tests/ambient_cases.py."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
import filter_cases as fc
import filter_lib as fl
import oracle_lib as ol
from ray_oracle import F32, FLT_MAX, assert_same

KEYS = ("normal", "position", "albedo", "t", "geom", "prim")
_WANT = {}


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    rr.set_ambient_table(ac.table())
    rr.uploaded = None
    yield rr
    rr.close()


def use(r, name):
    d = ac.scene(name)[0]
    if r.uploaded != name:
        r.upload(ol.scene_to_product(d))
        r.uploaded = name
    return d


def want(name, ray_set):
    if ray_set == "frame":
        return fc.traced_guides(name)
    if (name, ray_set) not in _WANT:
        _WANT[(name, ray_set)] = fc.frozen(fl.gbuffer(ac.scene(name)[0], *ac.rays(name, ray_set)))
    return _WANT[(name, ray_set)]


def assert_gbuffer(got, w, what, sel=slice(None)):
    for key in ("normal", "position", "albedo", "t"):
        assert_same(got[key], w[key][sel], f"{what} {key}")
    assert np.array_equal(got["geom"], w["geom"][sel]) and np.array_equal(got["prim"], w["prim"][sel]), what


SETS = [(s, rs_) for s in ac.SCENES for rs_ in ac.RAY_SETS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ray_set", SETS, ids=[f"{s}-{rs_}" for s, rs_ in SETS])
def test_rays_match_the_restatement(r, name, ray_set):
    use(r, name)
    o, dirs = ac.rays(name, ray_set)
    w = want(name, ray_set)
    got = r.gbuffer(o, dirs)
    st = r.gbuffer_stats()
    what = f"{name} {ray_set}"
    assert_gbuffer(got, w, what)
    nh = int(w["has"].sum())
    assert nh > 0 and st["rays"] == len(o) and st["hit_rays"] == nh, st
    # t / geom / prim: byte for byte what intersect and ambient write
    hit = r.intersect(o, dirs)
    q = r.query_stats()
    radius, bias = ac.setting(name, 1)
    amb = r.ambient(o, dirs, radius=radius, bias=bias, seed=ac.SEED)
    for key in ("t", "geom", "prim"):
        assert got[key].tobytes() == hit[key].tobytes() == amb[key].tobytes(), (what, key)
    print(what, st, "intersect:", q)
    assert st["exact_rays"] == q["exact_rays"] and st["exact_tests"] == q["exact_tests"], (st, q)
    # every ray through the reference loop: the same outputs
    ex = r.gbuffer(o, dirs, exact=True)
    st = r.gbuffer_stats()
    assert_gbuffer(ex, w, what + " exact")
    assert st["rays"] == len(o) and st["hit_rays"] == nh and st["exact_rays"] == len(o) and st["exact_tests"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(r, n):
    name = "CornellBox-Sphere"
    use(r, name)
    o, dirs = (np.concatenate([a, b])[:n] for a, b in zip(ac.rays(name, "frame"), ac.rays(name, "surface")))
    wf, ws = want(name, "frame"), want(name, "surface")
    w = {k: np.concatenate([wf[k], ws[k]]) for k in KEYS + ("has",)}
    assert len(w["t"]) >= 257
    got = r.gbuffer(o, dirs)
    assert_gbuffer(got, w, f"n {n}", slice(0, n))
    st = r.gbuffer_stats()
    assert st["rays"] == n and st["hit_rays"] == int(w["has"][:n].sum()), st


@pytest.mark.gpu
def test_each_output_alone_and_none(esc, r):
    import torch
    name = "CornellBox-Sphere"
    use(r, name)
    o, dirs = ac.rays(name, "surface")
    w = want(name, "surface")
    n = len(o)
    dev = torch.device("cuda", r.device)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(dirs).to(dev)
    for key in KEYS:
        shape = (n, 3) if key in KEYS[:3] else (n,)
        buf = torch.empty(shape, dtype=torch.int32 if key in ("geom", "prim") else torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        r.gbuffer_rays(to, td, **{key: buf})
        r.synchronize()
        got = buf.cpu().numpy()
        if got.dtype == np.int32:
            assert np.array_equal(got, w[key]), key
        else:
            assert_same(got, w[key], key + " alone")
    with pytest.raises(esc.EscError, match="esc_gbuffer_rays.*one of"):
        r.gbuffer_rays(to, td)
    cam = ac.frame_camera(name)
    from esctp1raytracer_amd import _capi
    with pytest.raises(esc.EscError, match="esc_render_gbuffer.*one of"):
        _capi.check(r._lib.esc_render_gbuffer(r._h, C.byref(cam.c), 16, 12, 0, None, None, None, None, None, None))
    buf = torch.empty(n, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with pytest.raises(esc.EscError, match="esc_gbuffer_rays.*flags"):
        _capi.check(r._lib.esc_gbuffer_rays(r._h, n, p(to), p(td), 2, None, None, None, p(buf), None, None))
    with pytest.raises(esc.EscError, match="esc_gbuffer_rays.*n < 0"):
        _capi.check(r._lib.esc_gbuffer_rays(r._h, -1, p(to), p(td), 0, None, None, None, p(buf), None, None))
    with pytest.raises(esc.EscError, match="esc_gbuffer_rays.*d_origins"):
        _capi.check(r._lib.esc_gbuffer_rays(r._h, n, None, p(td), 0, None, None, None, p(buf), None, None))
    with pytest.raises(esc.EscError, match="esc_render_gbuffer.*W,H"):
        r.render_gbuffer(cam, 1, 12)
    r2 = esc.Renderer(0)
    with pytest.raises(esc.EscError, match="esc_gbuffer_rays.*scene"):
        r2.gbuffer(o, dirs)
    r2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_200", "CornellBox-Sphere"])
def test_odd_rays_among_ordinary_ones(r, name):
    d = use(r, name)
    o, dirs = (v.copy() for v in ac.rays(name, "surface"))
    plain = r.gbuffer(o, dirs)
    nan = F32(np.nan)
    dirs[3] = nan
    dirs[20] = 0
    o[41, 0] = nan
    dirs[64, 1] = nan
    dirs[65] = 0
    if len(d["spheres"]):
        o[65] = d["spheres"][0][:3] + F32(0.25) * d["spheres"][0][3] * np.array([1, 0, 0], F32)  # inside sphere 0
    o[90, 0] = nan
    dirs[90] = nan
    odd = [3, 20, 41, 64, 65, 90]
    w = fl.gbuffer(d, o, dirs)
    got = r.gbuffer(o, dirs)
    st = r.gbuffer_stats()
    print(name, {i: bool(w["has"][i]) for i in odd})
    assert_gbuffer(got, w, name + " odd rays")
    assert st["exact_rays"] >= len(odd) and st["hit_rays"] == int(w["has"].sum()), st
    keep = np.ones(len(o), bool)
    keep[odd] = False
    for key in KEYS:
        assert got[key][keep].tobytes() == plain[key][keep].tobytes(), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.SCENES)
def test_render_gbuffer(r, name):
    import torch
    use(r, name)
    # 16 x 12: the restatement
    g = r.render_gbuffer(ac.frame_camera(name), ac.FRAME_W, ac.FRAME_H)
    st = r.gbuffer_stats()
    w = want(name, "frame")
    got = {k: v.cpu().numpy().reshape((-1, 3) if k in KEYS[:3] else (-1,)) for k, v in g.items()}
    assert g["normal"].shape == (ac.FRAME_H, ac.FRAME_W, 3) and g["geom"].shape == (ac.FRAME_H, ac.FRAME_W)
    assert_gbuffer(got, w, name + " frame")
    assert st["rays"] == ac.FRAME_W * ac.FRAME_H and st["hit_rays"] == int(w["has"].sum()), st
    # 33 x 19 (odd, more than one workgroup): gbuffer_rays on camera_rays' rays, byte for byte
    W, H = 33, 19
    cam = ac.frame_camera(name, W, H)
    g = r.render_gbuffer(cam, W, H)
    st1 = r.gbuffer_stats()
    to, td = r.camera_rays(cam, W, H)
    out = r._gbuffer_tensors((W * H,))
    torch.cuda.current_stream(to.device).synchronize()
    r.gbuffer_rays(to, td, **out)
    st2 = r.gbuffer_stats()
    for k in KEYS:
        assert g[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), (name, k)
    assert st1 == st2 and st1["rays"] == W * H and st1["hit_rays"] > 0, (st1, st2)
    ex = r.render_gbuffer(cam, W, H, exact=True)
    for k in KEYS:
        assert g[k].cpu().numpy().tobytes() == ex[k].cpu().numpy().tobytes(), (name, k, "exact")


@pytest.mark.gpu
def test_ambient_is_unchanged_by_a_gbuffer_call(r):
    name = "rand5"
    use(r, name)
    o, dirs = ac.rays(name, "surface")
    radius, bias = ac.setting(name, 1)
    kw = dict(radius=radius, bias=bias, seed=ac.SEED, pixel_base=ac.PIXEL_BASE)
    before = r.ambient(o, dirs, **kw)
    s0 = r.ambient_stats()
    r.gbuffer(o, dirs)
    r.render_gbuffer(ac.frame_camera(name), ac.FRAME_W, ac.FRAME_H)
    after = r.ambient(o, dirs, **kw)
    assert s0 == r.ambient_stats()
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key
    assert np.array_equal(after["count"], ac.want(name, "surface", 1)["count"])
    assert (after["t"][~ac.want(name, "surface", 1)["has"]] == FLT_MAX).all()
