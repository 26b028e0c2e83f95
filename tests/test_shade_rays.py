"""Shading of caller-supplied rays (Renderer.camera_rays / shade_rays / shade / render_supersampled)
against the frame kernels and the reference-pinned oracle.

Three yardsticks:
  - camera rays: orc_camera_get_ray (camera.h:31-34) at s = (w + dx) / (W - 1), t = (h + dy) / (H - 1);
  - camera rays shaded: the frame itself (esc_render_rows), bit for bit, fp32 and u8;
  - arbitrary rays: ray_oracle.ray_colours, orc_render of pixel (0, 0) of a 2x2 frame whose camera is
    built by hand with origin o and lower_left_corner a, so that its ray is
    (o, orc_camera_get_ray(cam, 0, 0)) and its colour is scan_row's (main.cpp:698-791) for that ray.
NaN results compare as NaN (payloads are not portable between processors).
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import random_scenes as rs
from ray_cases import CORNELL_EYE, CORNELL_LOOK, box, ray_sets
from ray_oracle import F32, assert_same, normalize, ray_colours

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def _cpu(t):
    return t.cpu().numpy()


def shade_camera(esc, r, cam, W, H, rows=None, offsets=None, **kw):
    """shade_rays(camera_rays(cam)) for rows (r0, r1): (rgb, rgb8) numpy, band-local"""
    import torch
    r0, r1 = (0, H) if rows is None else rows
    o, d = r.camera_rays(cam, W, H, rows=(r0, r1), offsets=offsets)
    n = o.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=o.device)
    rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=o.device)
    r.shade_rays(o, d, rgb, rgb8=rgb8, pixel_base=r0 * W, **kw)
    r.synchronize()
    return _cpu(rgb).reshape(r1 - r0, W, 3), _cpu(rgb8).reshape(r1 - r0, W, 3)


def render_band(esc, r, cam, W, H, r0, r1, **kw):
    import torch
    dev = torch.device("cuda", r.device)
    f = torch.empty((r1 - r0) * W * 3, dtype=torch.float32, device=dev)
    u = torch.empty((r1 - r0) * W * 3, dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    r.render_rows(cam, W, H, r0, r1, f, u, **kw)
    r.synchronize()
    return _cpu(f).reshape(r1 - r0, W, 3), _cpu(u).reshape(r1 - r0, W, 3)


# ---- 1. camera rays pinned to orc_camera_get_ray ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H,rows,with_offsets", [(37, 23, None, False), (37, 23, None, True),
                                                   (64, 41, (7, 19), True), (5, 2, (1, 2), False)])
def test_camera_rays_pinned(esc, r, W, H, rows, with_offsets):
    import torch
    lib = ol.oracle()
    r.upload(ol.scene_to_product(ol.scene_one()))
    eye, look = (0.3, 1.1, 3.2), (0.1, 0.9, -0.2)
    cam = esc.Camera.for_image(eye, look, W, H)
    ocam = ol.oracle_camera(eye, look, W, H)
    r0, r1 = (0, H) if rows is None else rows
    n = (r1 - r0) * W
    off = None
    if with_offsets:
        off = np.random.default_rng(W * H).uniform(-0.5, 0.5, (n, 2)).astype(F32)
        off[::11] = 0.0
    toff = None if off is None else torch.from_numpy(off).to(torch.device("cuda", r.device))
    torch.cuda.synchronize()
    o, d = r.camera_rays(cam, W, H, rows=rows, offsets=toff)
    r.synchronize()
    o, d = _cpu(o), _cpu(d)
    want = np.zeros((n, 3), F32)
    out = np.zeros(3, F32)
    for i in range(n):
        h, w = r0 + i // W, i % W
        dx, dy = (F32(0), F32(0)) if off is None else (off[i, 0], off[i, 1])
        s = (F32(w) + dx) / F32(W - 1)
        t = (F32(h) + dy) / F32(H - 1)
        lib.orc_camera_get_ray(C.byref(ocam), C.c_float(s), C.c_float(t), ol.fp(out))
        want[i] = out
    assert_same(d, want, "directions")
    assert_same(o, np.broadcast_to(np.array(ocam.origin, F32), (n, 3)), "origins")


# ---- 2. camera rays shaded == the frame ------------------------------------------------------------
def _scene(esc, name):
    if name in ("one", "two"):
        return ol.load_dump(name), ol.scene_to_product(ol.load_dump(name)), (0, 1, 3), (0, 1, 0)
    if name in ("cornell", "water"):
        d = ol.load_dump("CornellBox-Original" if name == "cornell" else "CornellBox-Water")
        return d, ol.scene_to_product(d), CORNELL_EYE, CORNELL_LOOK
    sc = esc.Scene.synthetic(name)
    eye, look = esc.synthetic_view()
    return None, sc, eye, look


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two", "cornell", "water", "c2", "c3"])
def test_camera_rays_shaded_equal_the_frame(esc, r, name, tmp_path):
    _, sc, eye, look = _scene(esc, name)
    r.upload(sc)
    W, H = (1024, 768) if name in ("one", "two") else (320, 181)
    cam = esc.Camera.for_image(eye, look, W, H)
    rgb, rgb8 = shade_camera(esc, r, cam, W, H)
    img, u8 = r.render(cam, W, H, want_u8=True)
    assert_same(rgb, img, name)
    assert np.array_equal(rgb8, u8)
    if name in ("one", "two"):
        md5 = {"one": "b10e1cb14f839129bd111670002cfb0b", "two": "c8137a8d70d8de0ad6a001d41be4e0e1"}[name]
        p = tmp_path / "x.ppm"
        esc.write_ppm(p, rgb8)
        assert hashlib.md5(p.read_bytes()).hexdigest() == md5


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,band", [("c4", 3840, 2160, 720), ("c5", 7680, 4320, 540)])
def test_large_frames_in_bands(esc, r, name, W, H, band):
    _, sc, eye, look = _scene(esc, name)
    r.upload(sc)
    cam = esc.Camera.for_image(eye, look, W, H)
    for r0 in range(0, H, band):
        r1 = min(H, r0 + band)
        rgb, rgb8 = shade_camera(esc, r, cam, W, H, rows=(r0, r1))
        f, u = render_band(esc, r, cam, W, H, r0, r1)
        assert_same(rgb, f, f"{name} rows {r0}..{r1}")
        assert np.array_equal(rgb8, u)
        st = r.shade_stats()
        assert st["rays"] == (r1 - r0) * W and st["exact_rays"] == 0, st


@pytest.mark.gpu
def test_face_modes_shadows_and_row_bands(esc, r):
    d = ol.load_dump("CornellBox-Original")
    r.upload(ol.scene_to_product(d))
    W, H = 200, 150
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    assert min(g["face_index"].shape[0] for i, g in enumerate(d["geometry"]) if i in d["light_sources"]) >= 2
    cases = [dict(face_mode=esc.ESC_FACE_FIXED, fixed_face=0), dict(face_mode=esc.ESC_FACE_FIXED, fixed_face=1),
             dict(face_mode=esc.ESC_FACE_HASH, seed=1), dict(face_mode=esc.ESC_FACE_HASH, seed=0xDEADBEEF12),
             dict(shadows=False)]
    for kw in cases:
        rgb, rgb8 = shade_camera(esc, r, cam, W, H, **kw)
        img, u8 = r.render(cam, W, H, want_u8=True, **kw)
        assert_same(rgb, img, str(kw))
        assert np.array_equal(rgb8, u8)
        # a row band with pixel_base = r0 * W
        rgb, _ = shade_camera(esc, r, cam, W, H, rows=(37, 101), **kw)
        assert_same(rgb, img[37:101], f"band {kw}")
    # a second scene: two lights, smooth normals
    two = ol.load_dump("two")
    r.upload(ol.scene_to_product(two))
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), W, H)
    for seed in (3, 4):
        rgb, _ = shade_camera(esc, r, cam, W, H, face_mode=esc.ESC_FACE_HASH, seed=seed)
        assert_same(rgb, r.render(cam, W, H, face_mode=esc.ESC_FACE_HASH, seed=seed), f"two seed {seed}")


# ---- 3. arbitrary rays against the reference-pinned oracle ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", ["cornell", 9, 18, 27, 3, 5, 14, 22])
def test_arbitrary_rays_against_the_oracle(esc, r, seed):
    if seed == "cornell":
        d = ol.load_dump("CornellBox-Original")
    else:
        d = rs.random_scene(seed)[0]
    r.upload(ol.scene_to_product(d))
    rng = np.random.default_rng(7 if seed == "cornell" else seed)
    n = 96
    for name, (o, a) in ray_sets(d, rng, n).items():
        dirs, want = ray_colours(d, o, a)
        got = r.shade(o, dirs, face_mode=esc.ESC_FACE_FIXED)
        assert_same(got["rgb"], want, f"{seed} {name}")
        ex = r.shade(o, dirs, face_mode=esc.ESC_FACE_FIXED, exact=True)
        assert_same(ex["rgb"], want, f"{seed} {name} exact")


# ---- 4. quirk S3: the first occluder in index order moves the next light's hit point --------------
def _s3_scene(n_filler):
    floor = {"vertex": np.array([(-5, 0, 5), (5, 0, 5), (5, 0, -5), (-5, 0, 5), (5, 0, -5), (-5, 0, -5)], F32),
             "face_index": np.arange(6).reshape(-1, 3), "material": ol.WHITE}
    light0 = {"vertex": np.array([(0, 2, 0), (0.2, 2, 0), (0, 2, 0.2)], F32),
              "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_A}
    light1 = {"vertex": np.array([(-2, 3, 2), (-1.8, 3, 2), (-2, 3, 2.2)], F32),
              "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_B}
    # three occluders between the floor and light 0, listed far-to-near (index order = far first)
    occ = [(0, 1.7, 0, 0.1), (0, 1.1, 0, 0.1), (0, 0.5, 0, 0.1)]
    rng = np.random.default_rng(3)
    filler = [(40 + x, y, z, 0.05) for x, y, z in rng.uniform(0, 4, (n_filler, 3))]
    sph = np.array(occ + filler, F32)
    mats = np.array([ol.RED] * len(sph), F32)
    return ol.scene_dict([floor, light0, light1], sph, mats)


@pytest.mark.gpu
@pytest.mark.parametrize("n_filler", [0, 600])  # 600: the sphere groups are swept, not in index order
def test_quirk_s3_first_occluder(esc, r, n_filler):
    d = _s3_scene(n_filler)
    r.upload(ol.scene_to_product(d))
    zs = np.linspace(0.004, 0.034, 7, dtype=F32)  # off the floor quad's diagonal (x = -z)
    o = np.stack([np.full(7, 3, F32), np.ones(7, F32), zs], 1).astype(F32)
    a = np.stack([np.zeros(7, F32), np.zeros(7, F32), zs], 1).astype(F32)
    dirs, want = ray_colours(d, o, a)
    got = r.shade(o, dirs)
    assert_same(got["rgb"], want, "first occluder")
    assert (got["geom"] == 0).all()  # every ray hit the floor
    # light 0 is occluded (it adds nothing); light 1 lights the point that the occluder's t2 moved
    # along the primary ray, and its diffuse term depends on where that point is
    amb = (np.array(ol.WHITE[:3], F32) * F32(0.5) + np.array(ol.WHITE[9:12], F32)) / F32(2)
    assert (want.sum(1) > amb.sum()).all(), want
    st = r.shade_stats()
    assert st["shadow_rays"] == 2 * 7 and st["hit_rays"] == 7, st


# ---- 5. filtered == exact on the large scenes ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["water", "c4", "c5"])
def test_filtered_equals_exact(esc, r, name):
    import torch
    d, sc, eye, look = _scene(esc, name)
    r.upload(sc)
    W, H = (256, 144) if name != "c5" else (128, 72)
    cam = esc.Camera.for_image(eye, look, W, H)
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()
    o, dd = _cpu(o), _cpu(dd)
    if d is None:
        d = ol.scene_from_product(sc)
    lo, hi = box(d)
    rng = np.random.default_rng(13)
    m = 8192 if name != "c5" else 2048
    oi = (lo + rng.uniform(0, 1, (m, 3)) * (hi - lo)).astype(F32)
    di = normalize(rng.standard_normal((m, 3)))
    for what, (oo, ddd) in (("camera", (o, dd)), ("incoherent", (oi, di))):
        a = r.shade(oo, ddd)
        st = r.shade_stats()
        b = r.shade(oo, ddd, exact=True)
        stx = r.shade_stats()
        for k in ("rgb", "t"):
            assert_same(a[k], b[k], f"{name} {what} {k}")
        for k in ("rgb8", "geom", "prim"):
            assert np.array_equal(a[k], b[k]), f"{name} {what} {k}"
        q = r.intersect(oo, ddd)
        assert_same(a["t"], q["t"], f"{name} {what} t vs intersect")
        assert np.array_equal(a["geom"], q["geom"]) and np.array_equal(a["prim"], q["prim"])
        n = oo.shape[0]
        assert st["rays"] == n and stx["rays"] == n
        assert stx["exact_rays"] == n + stx["shadow_rays"], stx
        if what == "camera":
            # the camera's rays and their shadow rays all meet the filters' preconditions
            assert st["exact_rays"] == 0, st
            assert st["hit_rays"] == int((a["prim"] >= 0).sum()), st
        if name == "c4" and what == "camera":
            assert st["exact_tests"] * 5 < stx["exact_tests"], (st, stx)


# ---- 6. odd inputs ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_odd_inputs_match_exact(esc, r):
    d = ol.load_dump("CornellBox-Original")
    r.upload(ol.scene_to_product(d))
    rng = np.random.default_rng(5)
    n = 4096
    lo, hi = box(d)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F32)
    dirs = normalize(rng.standard_normal((n, 3)))
    dirs[::7] *= F32(2.0)
    dirs[1::7] *= F32(1e-3)
    dirs[2::97] = 0.0
    dirs[3::97, 1] = np.nan
    dirs[4::97, 2] = np.inf
    o[5::101] = F32(2.0 ** 61)
    o[6::101, 0] = -F32(2.0 ** 61)
    dirs[7::101] = normalize(-o[7::101] * F32(2.0 ** 61) + F32(1))
    o[7::101] *= F32(2.0 ** 40)
    a = r.shade(o, dirs)
    st = r.shade_stats()
    b = r.shade(o, dirs, exact=True)
    for k in ("rgb", "t"):
        assert_same(a[k], b[k], k)
    for k in ("geom", "prim"):
        assert np.array_equal(a[k], b[k]), k
    assert 0 < st["exact_rays"] < n + st["shadow_rays"]
    # n == 0, and 2^20 + 17 rays
    z = r.shade(np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    assert z["rgb"].shape == (0, 3)
    assert r.shade_stats()["rays"] == 0
    m = (1 << 20) + 17
    o = (lo + rng.uniform(0, 1, (m, 3)) * (hi - lo)).astype(F32)
    dirs = normalize(rng.standard_normal((m, 3)))
    a = r.shade(o, dirs)
    assert r.shade_stats()["rays"] == m
    b = r.shade(o, dirs, exact=True)
    assert_same(a["rgb"], b["rgb"], "2^20 + 17 rays")


# ---- 7. supersampling ------------------------------------------------------------------------------
def _offsets(k, nn):
    i, j = k % nn, k // nn
    return (F32(i) + F32(0.5)) / F32(nn) - F32(0.5), (F32(j) + F32(0.5)) / F32(nn) - F32(0.5)


@pytest.mark.gpu
def test_supersampling(esc, r, tmp_path):
    import torch
    dev = torch.device("cuda", r.device)
    # spp == 1 is the frame
    for name, W, H in (("c4", 640, 360), ("cornell", 200, 150)):
        _, sc, eye, look = _scene(esc, name)
        r.upload(sc)
        cam = esc.Camera.for_image(eye, look, W, H)
        img, u8 = r.render_supersampled(cam, W, H, 1, want_u8=True)
        ref, ref8 = r.render(cam, W, H, want_u8=True)
        assert_same(img, ref, f"{name} spp 1")
        assert np.array_equal(u8, ref8)
    # spp 4 and 9 == the documented sum and divide over separately shaded samples (hashed faces)
    d = ol.load_dump("CornellBox-Original")
    r.upload(ol.scene_to_product(d))
    W, H = 96, 72
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    for spp in (4, 9):
        nn = int(round(spp ** 0.5))
        acc = np.zeros((H, W, 3), F32)
        for k in range(spp):
            dx, dy = _offsets(k, nn)
            off = torch.from_numpy(np.tile(np.array([dx, dy], F32), (W * H, 1))).to(dev)
            torch.cuda.synchronize()
            rgb, _ = shade_camera(esc, r, cam, W, H, offsets=off, face_mode=esc.ESC_FACE_HASH, seed=11 + k)
            acc = (acc + rgb).astype(F32)
        want = (acc / F32(spp)).astype(F32)
        img, u8 = r.render_supersampled(cam, W, H, spp, want_u8=True, face_mode=esc.ESC_FACE_HASH, seed=11)
        assert_same(img, want, f"spp {spp}")
        assert np.array_equal(u8, ol.oracle_quantise(want))
        img2, u82 = r.render_supersampled(cam, W, H, spp, want_u8=True, face_mode=esc.ESC_FACE_HASH, seed=11)
        assert img2.tobytes() == img.tobytes() and u82.tobytes() == u8.tobytes()
        assert not np.array_equal(img, r.render(cam, W, H, face_mode=esc.ESC_FACE_HASH, seed=11))
    with pytest.raises(esc.EscError):
        r.render_supersampled(cam, W, H, 3)
    with pytest.raises(esc.EscError):
        r.render_supersampled(cam, W, H, 81)
    # the viewer's --spp 4 PPM == the Python result quantised (hashed faces, seed 0: its defaults)
    viewer = os.path.join(ROOT, "bin", "ESCViewer2021")
    obj_dir = tmp_path / "models"
    import tarfile
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as tf:
        tf.extractall(obj_dir)
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(obj_dir) for f in fs if f == "CornellBox-Original.obj"]
    assert objs
    W, H = 64, 48
    ppm = tmp_path / "ss.ppm"
    p = subprocess.run([viewer, "-m", objs[0], "-v", "0,1,3.5", "-l", "0,1,0", "-w", f"{W},{H}", "--spp", "4",
                        "-o", str(ppm)], capture_output=True, text=True, timeout=300, cwd=os.path.dirname(objs[0]))
    assert p.returncode == 0, p.stderr
    sc = esc.Scene.load_obj(objs[0])
    r.upload(sc)
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    img = r.render_supersampled(cam, W, H, 4, face_mode=esc.ESC_FACE_HASH, seed=0)
    mine = tmp_path / "mine.ppm"
    esc.write_ppm(mine, img)
    assert ppm.read_bytes() == mine.read_bytes()


# ---- 8. no interference ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_shading_leaves_rendering_alone(esc):
    import torch
    r = esc.Renderer(0)
    sc = esc.Scene.synthetic("c4", 2000)
    r.upload(sc)
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, 320, 180)
    r.reset_counters()
    f1 = r.render(cam, 320, 180)
    c1 = r.counters()
    cam2 = esc.Camera.for_image(eye, (0.5, 2, -8), 97, 61)
    shade_camera(esc, r, cam2, 97, 61)
    r.render_supersampled(cam2, 97, 61, 4)
    assert r.counters() == c1
    r.reset_counters()
    f2 = r.render(cam, 320, 180)
    assert r.counters() == c1
    assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32))
    dev = torch.device("cuda", 0)
    out = torch.empty(320 * 180 * 3, dtype=torch.float32, device=dev)
    fr = r.record_strips(cam, 320, 180, 0, 1, out)
    shade_camera(esc, r, cam2, 97, 61)
    r.render_supersampled(cam2, 97, 61, 9)
    out.zero_()
    r.synchronize()
    fr.launch()
    r.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(180, 320, 3).view(np.uint32), f1.view(np.uint32))
    fr.close()
    r.close()


@pytest.mark.gpu
def test_shade_rays_on_a_torch_stream(esc):
    import torch
    d = ol.load_dump("CornellBox-Original")
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=s)
    r.upload(ol.scene_to_product(d))
    W, H = 128, 96
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    ref = r.render(cam, W, H)
    with torch.cuda.stream(s):
        o, dd = r.camera_rays(cam, W, H)
        rgb = torch.full((W * H, 3), -1.0, device=dev)
        r.shade_rays(o, dd, rgb)
        got = rgb.cpu().numpy().reshape(H, W, 3)
    assert_same(got, ref, "torch stream")
    r.close()
