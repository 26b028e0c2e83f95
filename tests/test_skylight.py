"""Sky lighting on the GPU (Renderer.skylight / skylight_rays / render_skylight / add_light) against the numpy
restatement of tests/skylight_lib.py: sky, light, vis and t bit for bit, count / geom / prim exactly.  There is
no tolerance in this file.  Scenes, rays and settings are those of tests/ambient_cases.py, the cubes and the
conditions those of tests/skylight_cases.py, asserted on the CPU (test_skylight_cpu.py) and again here before
a case is compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
import ambient_lib as al
import oracle_lib as ol
import skylight_cases as sc
import skylight_lib as sl
from environment_lib import random_cube
from ray_cases import surface_points
from ray_oracle import F32, FLT_MAX, assert_same, normalize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, S = ac.TABLE_SAMPLES, ac.TABLE_SETS
FLOATS, INTS = ("sky", "light", "vis", "t"), ("count", "geom", "prim")
SKY = ((0.2, 0.4, 1.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1))


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    rr.set_ambient_table(ac.table())
    rr.set_environment(sc.cube())
    rr.uploaded = None
    yield rr
    rr.close()


def use(r, name):
    """the scene of a case on the device (uploaded when it is not the one already there) -> scene dict"""
    d = ac.scene(name)[0]
    if r.uploaded != name:
        r.upload(ol.scene_to_product(d))
        r.uploaded = name
    return d


def joined(a, w, n=None):
    """the restatement's seven outputs: ambient's dict and skylight's, the first n rays"""
    out = {key: a[key] for key in ("vis", "t", "count", "geom", "prim")}
    out.update(sky=w["sky"], light=w["light"])
    return {key: v[:n] for key, v in out.items()}


def assert_skylight(got, want, what):
    for key in INTS:
        assert np.array_equal(got[key], want[key]), \
            f"{what}: {key} differs at {np.argwhere(got[key] != want[key])[:6].ravel().tolist()}"
    for key in FLOATS:
        assert got[key].shape == want[key].shape, (what, key)
        assert_same(got[key], want[key], f"{what} {key}")


# ---- 1. every case: outputs and stats; 2. the old kernel holds the new one ---------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,ray_set,k", sc.CASES, ids=[f"{s}-{rs_}-{k}" for s, rs_, k in sc.CASES])
def test_case_matches_the_restatement(r, name, ray_set, k):
    sc.check_condition(name, ray_set, k)
    use(r, name)
    o, dirs = ac.rays(name, ray_set)
    radius, bias = ac.setting(name, k)
    a = ac.want(name, ray_set, k)
    want = joined(a, sc.want(name, ray_set, k))
    kw = dict(radius=radius, bias=bias, seed=ac.SEED, pixel_base=ac.PIXEL_BASE if ray_set == "surface" else 0)
    what = f"{name} {ray_set} radius {radius} bias {bias}"
    before = r.ambient(o, dirs, **kw)
    st0 = r.ambient_stats()
    got = r.skylight(o, dirs, **kw)
    st = r.ambient_stats()
    assert_skylight(got, want, what)
    assert (got["light"] != 0).any() and (got["sky"] != 0).any(), what
    # the stats are those of the visibility answer, and of the ambient call
    nh = int(a["has"].sum())
    assert st["rays"] == len(o) and st["hit_rays"] == nh and st["samples"] == K * nh, st
    assert st["occluded_samples"] == int((K - a["count"][a["has"]]).sum()), st
    assert st == st0, (st, st0)
    # the old kernel holds the new one, and is what it was after it
    after = r.ambient(o, dirs, **kw)
    for key in ("vis", "count", "t", "geom", "prim"):
        assert got[key].tobytes() == before[key].tobytes(), (what, key)
        assert after[key].tobytes() == before[key].tobytes(), (what, key)
    # every ray through the reference loop: the same outputs
    ex = r.skylight(o, dirs, exact=True, **kw)
    st = r.ambient_stats()
    assert_skylight(ex, want, what + " exact")
    assert st["exact_rays"] == len(o) + K * nh, st


# ---- 3. the all-ones cube ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["CornellBox-Sphere", "c2_200"])
def test_all_ones_cube_gives_the_visibility(esc, name):
    r = esc.Renderer(0)
    r.set_ambient_table(ac.table())
    r.set_environment(sc.cube("ones"))
    d = ac.scene(name)[0]
    r.upload(ol.scene_to_product(d))
    o, dirs = ac.rays(name, "frame")
    radius, bias = ac.setting(name, 1)
    a = ac.want(name, "frame", 1)
    got = r.skylight(o, dirs, radius=radius, bias=bias, seed=ac.SEED)
    has = a["has"]
    assert has.any() and (name != "c2_200" or not has.all()), "hits, and in c2_200's frame misses too"
    for c in range(3):
        assert got["sky"][has, c].tobytes() == got["vis"][has].tobytes(), (name, c)
    kd = sl.material_kd(d, got["geom"], got["prim"])
    assert_same(got["light"][has], (kd[has] * got["vis"][has, None]).astype(F32), name + " light == kd * vis")
    assert not got["sky"][~has].view(np.uint32).any() and not got["light"][~has].view(np.uint32).any()
    assert (got["vis"][~has] == 1).all() and (got["count"][~has] == K).all()
    assert_skylight(got, joined(a, sc.want(name, "frame", 1, "ones")), name + " ones")
    r.close()


# ---- 4. shapes -------------------------------------------------------------------------------------------------
SHAPE_SCENE = "CornellBox-Original"
_SHAPE = {}


def shape_rays():
    """257 rays from the eye to surface points (rng seed 2)"""
    if "rays" not in _SHAPE:
        d, eye, _, _ = ac.scene(SHAPE_SCENE)
        pts = surface_points(d, 257, np.random.default_rng(2))
        o = np.tile(np.array(eye, F32), (257, 1))
        _SHAPE["rays"] = (o, normalize((pts - o).astype(F32)))
    return _SHAPE["rays"]


def shape_cube(res):
    return random_cube(res, 3 + res)


def shape_want(k_, s_, res, n=257):
    """the restatement for the first n shape rays with the (s_, k_) table of seed 9 and the cube of res"""
    key = (k_, s_, n)
    if key not in _SHAPE:
        o, dirs = shape_rays()
        _SHAPE[key] = al.ambient(ac.scene(SHAPE_SCENE)[0], o[:n], dirs[:n], ac.table(s_, k_, 9),
                                 ac.setting(SHAPE_SCENE, 1)[0], 1e-3, 5, 0)
    a = _SHAPE[key]
    return a, sl.skylight(ac.scene(SHAPE_SCENE)[0], a, shape_cube(res), k_)


@pytest.mark.gpu
@pytest.mark.parametrize("k_,s_", [(8, 4), (1, 1), (64, 64), (64, 1), (1, 64)])
def test_shapes(esc, k_, s_):
    r = esc.Renderer(0)
    r.upload(ol.scene_to_product(ac.scene(SHAPE_SCENE)[0]))
    r.set_ambient_table(ac.table(s_, k_, 9))
    o, dirs = shape_rays()
    radius = ac.setting(SHAPE_SCENE, 1)[0]
    many = (k_, s_) == (8, 4)
    for res in (1, 8):
        r.set_environment(shape_cube(res))
        a, w = shape_want(k_, s_, res, 257 if many else 65)
        assert a["has"].all()
        for n in ((0, 1, 63, 64, 65, 257) if many else (65,)):
            got = r.skylight(o[:n], dirs[:n], radius=radius, bias=1e-3, seed=5)
            assert_skylight(got, joined(a, w, n), f"n {n} K {k_} S {s_} R {res}")
            st = r.ambient_stats()
            assert st["rays"] == n and st["hit_rays"] == n and st["samples"] == k_ * n, st
    r.close()


@pytest.mark.gpu
def test_table_prefix_and_a_lone_hit(esc):
    r = esc.Renderer(0)
    d = ac.scene(SHAPE_SCENE)[0]
    r.upload(ol.scene_to_product(d))
    r.set_environment(sc.cube())
    o, dirs = shape_rays()
    radius = ac.setting(SHAPE_SCENE, 1)[0]
    # the first 8 samples of the first 4 sets of a 64 x 64 table are the 4 x 8 table they form
    big = ac.table(64, 64, 9)
    r.set_ambient_table(big)
    a = al.ambient(d, o[:65], dirs[:65], big[:4, :8], radius, 1e-3, 5, 0)
    got = r.skylight(o[:65], dirs[:65], radius=radius, bias=1e-3, seed=5, samples=8, sets=4)
    assert_skylight(got, joined(a, sl.skylight(d, a, sc.cube(), 8)), "prefix")
    # a wave with exactly one hitting lane, next to a wave of misses
    r.set_ambient_table(ac.table())
    dd = np.tile(np.array([0, 0, 1], F32), (128, 1))  # out of the box's open front
    dd[17] = dirs[17]
    oo = np.tile(o[:1], (128, 1))
    a = al.ambient(d, oo, dd, ac.table(), radius, 1e-3, 5, 0)
    assert a["has"].sum() == 1 and a["has"][17]
    got = r.skylight(oo, dd, radius=radius, bias=1e-3, seed=5)
    assert_skylight(got, joined(a, sl.skylight(d, a, sc.cube(), K)), "one hitting lane")
    assert not got["sky"][~a["has"]].view(np.uint32).any() and not got["light"][~a["has"]].view(np.uint32).any()
    st = r.ambient_stats()
    assert st["hit_rays"] == 1 and st["samples"] == K and st["occluded_samples"] == K - int(a["count"][17]), st
    r.close()


# ---- 5. odd rays -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_200", "CornellBox-Sphere"])
def test_odd_rays_among_ordinary_ones(r, name):
    d = use(r, name)
    o, dirs = (v.copy() for v in ac.rays(name, "surface"))
    radius, bias = ac.setting(name, 1)
    plain = r.skylight(o, dirs, radius=radius, bias=bias, seed=ac.SEED)
    nan = F32(np.nan)
    odd = {3: "nan_dir", 20: "zero_dir", 41: "nan_origin", 64: "nan_dir_one", 65: "zero_dir_inside", 90: "nan_both"}
    for i, kind in odd.items():
        if kind in ("nan_dir", "nan_both"):
            dirs[i] = nan
        if kind == "nan_dir_one":
            dirs[i, 1] = nan
        if kind in ("zero_dir", "zero_dir_inside"):
            dirs[i] = 0
        if kind in ("nan_origin", "nan_both"):
            o[i, 0] = nan
        if kind == "zero_dir_inside" and len(d["spheres"]):
            o[i] = d["spheres"][0][:3] + F32(0.25) * d["spheres"][0][3] * np.array([1, 0, 0], F32)  # inside sphere 0
    a = al.ambient(d, o, dirs, ac.table(), radius, bias, ac.SEED, 0)
    want = joined(a, sl.skylight(d, a, sc.cube(), K))
    got = r.skylight(o, dirs, radius=radius, bias=bias, seed=ac.SEED)
    print(name, {kind: (int(a["count"][i]), bool(a["has"][i]), want["sky"][i].tolist()) for i, kind in odd.items()})
    assert_skylight(got, want, name + " odd rays")
    keep = np.ones(len(o), bool)
    keep[list(odd)] = False
    for key in FLOATS + INTS:  # the ordinary rays' results are unchanged
        assert got[key][keep].tobytes() == plain[key][keep].tobytes(), key


# ---- 6. frames -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.SCENES)
def test_render_skylight(esc, r, name):
    import torch
    use(r, name)
    radius, bias = ac.setting(name, 1)
    # 16 x 12: the restatement
    a, w = ac.want(name, "frame", 1), sc.want(name, "frame", 1)
    f = r.render_skylight(ac.frame_camera(name), ac.FRAME_W, ac.FRAME_H, radius=radius, bias=bias, seed=ac.SEED,
                          want_count=True)
    assert f["sky"].shape == (ac.FRAME_H, ac.FRAME_W, 3) and f["vis"].shape == (ac.FRAME_H, ac.FRAME_W)
    assert f["count"].dtype == np.int32 and np.array_equal(f["count"].ravel(), a["count"]), name
    assert_same(f["vis"].ravel(), a["vis"], name + " frame vis")
    assert_same(f["sky"].reshape(-1, 3), w["sky"], name + " frame sky")
    assert_same(f["light"].reshape(-1, 3), w["light"], name + " frame light")
    only = r.render_skylight(ac.frame_camera(name), ac.FRAME_W, ac.FRAME_H, radius=radius, bias=bias, seed=ac.SEED,
                             want_light=False)
    assert sorted(only) == ["sky", "vis"] and only["sky"].tobytes() == f["sky"].tobytes()
    # 33 x 19 (odd, more than one workgroup): skylight_rays on camera_rays' rays, byte for byte
    W, H = 33, 19
    cam = ac.frame_camera(name, W, H)
    f = r.render_skylight(cam, W, H, radius=radius, bias=bias, seed=ac.SEED, want_count=True)
    st1 = r.ambient_stats()
    to, td = r.camera_rays(cam, W, H)
    dev = to.device
    ts, tl = (torch.empty((W * H, 3), dtype=torch.float32, device=dev) for _ in range(2))
    tv = torch.empty(W * H, dtype=torch.float32, device=dev)
    tc = torch.empty(W * H, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    r.skylight_rays(to, td, sky=ts, light=tl, vis=tv, count=tc, radius=radius, bias=bias, seed=ac.SEED)
    st2 = r.ambient_stats()
    for key, t in (("sky", ts), ("light", tl), ("vis", tv), ("count", tc)):
        assert f[key].tobytes() == t.cpu().numpy().tobytes(), (name, key)
    assert st1 == st2 and st1["rays"] == W * H and 0 < st1["occluded_samples"] < st1["samples"], (st1, st2)


# ---- 7. the environment and the table are the context's --------------------------------------------------------
@pytest.mark.gpu
def test_environment_and_table_survive_uploads(esc):
    r = esc.Renderer(0)
    r.set_ambient_table(ac.table())
    r.set_environment(sc.cube())
    r.uploaded = None
    for name in ("CornellBox-Original", "rand3", "CornellBox-Original"):  # nothing is set again in between
        use(r, name)
        o, dirs = ac.rays(name, "surface")
        radius, bias = ac.setting(name, 1)
        kw = dict(radius=radius, bias=bias, seed=ac.SEED, pixel_base=ac.PIXEL_BASE)
        got = r.skylight(o, dirs, **kw)
        assert_skylight(got, joined(ac.want(name, "surface", 1), sc.want(name, "surface", 1)), name + " after an upload")
    # a new cube replaces the old one
    r.set_environment(sc.cube("faces"))
    want = joined(ac.want(name, "surface", 1), sc.want(name, "surface", 1, "faces"))
    assert not np.array_equal(want["sky"], sc.want(name, "surface", 1)["sky"])
    assert_skylight(r.skylight(o, dirs, **kw), want, "new cube")
    # no environment: the calls say so, and ambient occlusion goes on
    r.set_environment(None)
    cam = ac.frame_camera(name)
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*environment"):
        r.skylight(o, dirs, **kw)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*environment"):
        r.render_skylight(cam, 16, 12, radius=radius)
    assert r.ambient(o, dirs, **kw)["vis"].tobytes() == ac.want(name, "surface", 1)["vis"].tobytes()
    # a renderer without a table
    r2 = esc.Renderer(0)
    r2.upload(ol.scene_to_product(ac.scene(name)[0]))
    r2.set_environment(sc.cube())
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*table"):
        r2.skylight(o, dirs, radius=1.0, samples=8, sets=4)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*table"):
        r2.render_skylight(cam, 16, 12, radius=1.0, samples=8, sets=4)
    r2.close()
    # afterwards the renderer still works
    r.set_environment(sc.cube())
    assert_skylight(r.skylight(o, dirs, **kw), joined(ac.want(name, "surface", 1), sc.want(name, "surface", 1)),
                    "after the errors")
    r.close()


# ---- 8. add_light ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_add_light(r):
    import torch
    rng = np.random.default_rng(4)
    img = rng.uniform(-0.5, 2.0, (19, 33, 3)).astype(F32)
    img[0, 0] = (0, 1, 1.5)
    light = rng.uniform(-0.25, 1.0, (19, 33, 3)).astype(F32)
    want = (img + light).astype(F32)
    out, u8 = r.add_light(img, light, want_u8=True)
    assert_same(out, want, "add_light")
    assert np.array_equal(u8, ol.oracle_quantise(want))
    assert r.add_light(img, light).tobytes() == out.tobytes()
    assert r.add_light(img[:0], light[:0]).shape == (0, 33, 3)  # nothing to do is not an error
    # in place: d_out is d_rgb
    dev = torch.device("cuda", r.device)
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(light).to(dev)
    t8 = torch.empty(img.shape, dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert r._lib.esc_add_light(r._h, 19 * 33, p(ti), p(tl), p(ti), p(t8)) == 0
    r.synchronize()
    assert ti.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(t8.cpu().numpy(), u8)
    assert r._lib.esc_add_light(r._h, 0, None, None, None, None) == 0


# ---- 9. bad arguments ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments(esc, r):
    import torch
    from esctp1raytracer_amd import _capi
    use(r, SHAPE_SCENE)
    o, dirs = shape_rays()
    o, dirs = o[:8], dirs[:8]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(esc.EscError, match="esc_skylight_rays.*radius"):
            r.skylight(o, dirs, radius=bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(esc.EscError, match="esc_skylight_rays.*bias"):
            r.skylight(o, dirs, radius=1.0, bias=bad)
    for bad in (0, -1, K + 1, 65):
        with pytest.raises(esc.EscError, match="esc_skylight_rays.*samples"):
            r.skylight(o, dirs, radius=1.0, samples=bad)
    for bad in (0, -1, S + 1, 65):
        with pytest.raises(esc.EscError, match="esc_skylight_rays.*sets"):
            r.skylight(o, dirs, radius=1.0, sets=bad)
    cam = ac.frame_camera(SHAPE_SCENE)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*radius"):
        r.render_skylight(cam, 16, 12, radius=-1.0)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*bias"):
        r.render_skylight(cam, 16, 12, radius=1.0, bias=-1.0)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*W,H"):
        r.render_skylight(cam, 1, 12, radius=1.0)
    with pytest.raises(esc.EscError, match="esc_render_skylight.*W,H"):
        r.render_skylight(cam, 16, 1, radius=1.0)
    # the raw calls: both outputs NULL, flags, n < 0, missing pointers
    dev = torch.device("cuda", r.device)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(dirs).to(dev)
    sky = torch.empty((8, 3), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = _capi.esc_ambient_options(K, S, 1.0, 1e-4, 0, 0, 0)
    call = lambda n, opts, s, l: r._lib.esc_skylight_rays(r._h, n, p(to), p(td), C.byref(opts), s, l, None, None, None,  # noqa: E731
                                                          None, None)
    assert call(8, good, p(sky), None) == _capi.ESC_OK  # one of the two outputs, and none of the optional ones
    assert call(8, good, None, p(sky)) == _capi.ESC_OK
    r.synchronize()
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*d_sky, d_light"):
        _capi.check(call(8, good, None, None))
    for flags in (2, 4, 3):
        bad = _capi.esc_ambient_options(K, S, 1.0, 1e-4, 0, 0, flags)
        with pytest.raises(esc.EscError, match="esc_skylight_rays.*flags"):
            _capi.check(call(8, bad, p(sky), None))
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*n < 0"):
        _capi.check(call(-1, good, p(sky), None))
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*opts"):
        _capi.check(r._lib.esc_skylight_rays(r._h, 8, p(to), p(td), None, p(sky), None, None, None, None, None, None))
    with pytest.raises(esc.EscError, match="esc_render_skylight.*d_sky, d_light"):
        _capi.check(r._lib.esc_render_skylight(r._h, C.byref(cam.c), 16, 12, C.byref(good), None, None, None, None))
    with pytest.raises(esc.EscError, match="esc_add_light.*d_out"):
        _capi.check(r._lib.esc_add_light(r._h, 8, p(sky), p(sky), None, None))
    with pytest.raises(esc.EscError, match="esc_add_light.*n < 0"):
        _capi.check(r._lib.esc_add_light(r._h, -1, p(sky), p(sky), p(sky), None))
    # a renderer without a scene
    r3 = esc.Renderer(0)
    r3.set_ambient_table(ac.table())
    r3.set_environment(sc.cube())
    with pytest.raises(esc.EscError, match="esc_skylight_rays.*scene"):
        r3.skylight(o, dirs, radius=1.0)
    r3.close()
    # the renderer still works
    name = "CornellBox-Original"
    radius, bias = ac.setting(name, 1)
    got = r.skylight(*ac.rays(name, "surface"), radius=radius, bias=bias, seed=ac.SEED, pixel_base=ac.PIXEL_BASE)
    assert_skylight(got, joined(ac.want(name, "surface", 1), sc.want(name, "surface", 1)), "after the errors")


# ---- 10. the viewer --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_viewer_skylight(esc, tmp_path):
    viewer = os.path.join(ROOT, "bin", "ESCViewer2021")
    obj = os.path.join(ROOT, "tests", "golden", "scenes", "one.obj")
    w, h = 32, 24
    sky = "/".join(",".join(repr(c) for c in col) for col in SKY)
    base = [viewer, "-m", obj, "-w", f"{w},{h}", "--sky", sky]
    ao = ["--ao", "8", "--ao-radius", "0.5"]
    out = {}
    for what, extra in (("skylight", ao + ["--skylight"]), ("ao", ao), ("sky", [])):
        ppm = tmp_path / (what + ".ppm")
        p = subprocess.run(base + extra + ["-o", str(ppm)], capture_output=True, text=True, timeout=300,
                           cwd=os.path.dirname(obj))
        assert p.returncode == 0, p.stderr
        out[what] = ppm.read_bytes()
    # the Python composition: the viewer's defaults are eye (0, 1, 3), look (0, 1, 0), hashed faces with seed 0,
    # a 64-texel sky, depth 0, 16 sets, bias 1e-4, table and draw seed 0
    r = esc.Renderer(0)
    r.upload(esc.Scene.load_obj(obj))
    r.set_ambient_table(esc.ambient_table(16, 8, 0))
    r.set_environment(esc.environment_sky(64, *SKY))
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), w, h)
    img = r.render_traced(cam, w, h, max_depth=0, bias=1e-4, face_mode=esc.ESC_FACE_HASH, seed=0)
    f = r.render_skylight(cam, w, h, radius=0.5, bias=1e-4, seed=0, want_count=True)
    assert (f["light"] != 0).any() and 0 < (f["count"] < 8).sum(), "the composition shows no light or no occlusion"
    mine = tmp_path / "mine.ppm"
    esc.write_ppm(mine, r.add_light(img, f["light"]))
    assert out["skylight"] == mine.read_bytes()
    assert out["skylight"] != out["ao"] and out["skylight"] != out["sky"]
    r.close()
