"""GPU: k_frame's SURE instantiation -- no workgroup vote, no fallback sweep -- and the launch conditions
that guard it (csrc/rt_kernels.hip k_frame / esc_launch_render, csrc/rt_capi.cpp, DESIGN.md 3.9 "Frames that
need no fallback").

 1. same image: c3 (300 spheres) and a c4 cut (600) at 64x8 (one full workgroup tile), 80x12 (a partial tile
    to the right and one below) and 200x40 as the two ranks of a stride-2 strip partition; fp32 and bytes,
    rendered three ways -- default (SURE), ESC_RENDER_VOTE, ESC_RENDER_INDEX_ORDER -- identical bit for bit and
    byte for byte; the instantiation query names SURE for the first and only for it; the tripwire reads 0;
 2. the launch refuses when it must, and the frame equals the index-order frame: (a) a direction cell over
    kLightListCap (spheres strung along one ray from the sample point; the list read-back shows the cell),
    (b) a camera beyond the bound of 3.9, and a non-finite camera (which the renderer refuses outright),
    (c) ESC_RENDER_VOTE, (d) a two-face light with per-pixel face draws (shadow_lists_cover rejects it);
 3. tripwire: twenty seeded random scenes (random_scenes.py) at 96x24, a camera inside and one just outside
    the scene box each: wherever SURE ran, the tripwire is 0 and the frame is the ESC_RENDER_VOTE frame's.
"""
import numpy as np
import pytest

import oracle_lib as ol
import random_scenes

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as esc
    return esc


@pytest.fixture(scope="module")
def renderer(esc):
    r = esc.Renderer(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def frame(esc, renderer, cam, w, h, flags=0, **kw):
    """-> (fp32, bytes, last_frame_kernel, tripwire)"""
    img, u8 = renderer.render(cam, w, h, want_u8=True, flags=flags, **kw)
    return img, u8, renderer.last_frame_kernel(), renderer.frame_tripwire()


def strips(esc, renderer, cam, w, h, flags=0):
    """both ranks of a stride-2 strip partition -> (fp32 rows, byte rows, kernels, tripwire)"""
    import torch
    f, b, kern = [], [], []
    for rank in range(2):
        n = esc.strip_local_rows(h, 8, rank, 2) * w * 3
        of = torch.zeros(n, dtype=torch.float32, device="cuda:0")
        ob = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        renderer.render_strips(cam, w, h, rank, 2, out_f32=of, out_u8=ob, flags=flags)
        kern.append(renderer.last_frame_kernel())
        renderer.synchronize()
        f.append(of.cpu().numpy())
        b.append(ob.cpu().numpy())
    return np.concatenate(f), np.concatenate(b), kern, renderer.frame_tripwire()


SCENES = {"c3": ("c3", 300), "c4 cut": ("c4", 600)}


@pytest.mark.parametrize("name", list(SCENES))
def test_same_image_three_ways(esc, renderer, name):
    sc = esc.Scene.synthetic(*SCENES[name])
    renderer.upload(sc)
    eye, look = esc.synthetic_view()
    assert sc.shadow_origins_inside(eye)
    for w, h in ((64, 8), (80, 12)):
        cam = esc.Camera.for_image(eye, look, w, h)
        img, u8, kern, trip = frame(esc, renderer, cam, w, h)
        assert kern["fused"] and kern["sure"] and not kern["idl"] and not kern["tgrp"], f"{name} {w}x{h}: {kern}"
        assert trip == 0
        assert np.any(img)
        for what, fl in (("vote", esc.ESC_RENDER_VOTE), ("index order", esc.ESC_RENDER_INDEX_ORDER)):
            img2, u82, kern2, trip2 = frame(esc, renderer, cam, w, h, flags=fl)
            assert kern2["fused"] and not kern2["sure"], f"{name} {w}x{h} {what}: {kern2}"
            assert trip2 == 0
            assert np.array_equal(bits(img), bits(img2)), f"{name} {w}x{h}: SURE and {what} differ in fp32"
            assert np.array_equal(u8, u82), f"{name} {w}x{h}: SURE and {what} differ in bytes"
    w, h = 200, 40
    cam = esc.Camera.for_image(eye, look, w, h)
    f, b, kern, trip = strips(esc, renderer, cam, w, h)
    assert all(k["sure"] for k in kern) and trip == 0, f"{name} strips: {kern}, tripwire {trip}"
    assert np.any(f)
    for what, fl in (("vote", esc.ESC_RENDER_VOTE), ("index order", esc.ESC_RENDER_INDEX_ORDER)):
        f2, b2, kern2, trip2 = strips(esc, renderer, cam, w, h, flags=fl)
        assert not any(k["sure"] for k in kern2) and trip2 == 0
        assert np.array_equal(bits(f), bits(f2)), f"{name} strips: SURE and {what} differ in fp32"
        assert np.array_equal(b, b2), f"{name} strips: SURE and {what} differ in bytes"


def refused(esc, renderer, cam, w, h, what, flags=0, **kw):
    """the frame (default options plus `flags`) runs today's kernel and equals the index-order frame"""
    img, u8, kern, trip = frame(esc, renderer, cam, w, h, flags=flags, **kw)
    assert kern["fused"] and not kern["sure"], f"{what}: {kern}"
    assert trip == 0
    ref, ref8, _, _ = frame(esc, renderer, cam, w, h, flags=esc.ESC_RENDER_INDEX_ORDER, **kw)
    assert np.array_equal(bits(img), bits(ref)), f"{what}: differs from the index-order frame"
    assert np.array_equal(u8, ref8), f"{what}: bytes differ from the index-order frame"
    return img


FLOOR = {"vertex": np.array([(-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6)], F32),
         "face_index": np.array([[0, 1, 2], [0, 2, 3]]), "material": ol.WHITE}
LIGHT = {"vertex": np.array([(-0.5, 8, 0), (0.5, 8, 0), (0, 8, -0.5)], F32), "face_index": np.array([[0, 1, 2]]),
         "material": ol.LIGHT_A}


def grey(n):
    return np.stack([ol.material13(ka=(0.4, 0.4, 0.4), kd=(0.6, 0.6, 0.6))] * n)


def test_refused_cell_over_cap(esc, renderer):
    # the sample point the product takes for the light, then 400 small spheres along one ray from it
    P = ol.scene_to_product(ol.scene_dict([dict(FLOOR), dict(LIGHT)])).table("light_points").view(F32)[:3]
    u = np.array([0.21, -1.0, 0.13])
    u /= np.linalg.norm(u)
    s = np.linspace(2.0, 7.0, 400)
    sph = np.concatenate([P.astype(np.float64) + s[:, None] * u, np.full((400, 1), 0.004)], axis=1).astype(F32)
    sc = ol.scene_to_product(ol.scene_dict([dict(FLOOR), dict(LIGHT)], sph, grey(400)))
    renderer.upload(sc)
    eye, look = (0.0, 3.0, 9.0), (0.0, 2.0, 0.0)
    assert sc.shadow_origins_inside(eye)  # the camera is not the reason
    cam = esc.Camera.for_image(eye, look, 80, 12)
    refused(esc, renderer, cam, 80, 12, "cell over its cap")
    ll = renderer.light_lists(2)
    assert ll is not None and int(ll["counts"].max()) > ll["cap"], "no cell is over kLightListCap"


def test_refused_camera(esc, renderer):
    sc = esc.Scene.synthetic("c3", 300)
    renderer.upload(sc)
    eye, look = esc.synthetic_view()
    hdr = sc.table("header").view(F32)
    lo, hi = hdr[4:7].astype(np.float64), hdr[7:10].astype(np.float64)
    dist = 12.0 * float((hi - lo).sum())  # (the bound is near 10 times the extents' sum)
    far = tuple(float(x) for x in (0.5 * (lo + hi) + dist * np.array([0.1, 0.5, 0.87])).astype(F32))
    assert sc.shadow_origins_inside(eye) and not sc.shadow_origins_inside(far)
    cam = esc.Camera.for_image(far, (0.0, 1.0, -10.0), 80, 12, vfov=0.4)  # (the oracle lights 207 pixels)
    img = refused(esc, renderer, cam, 80, 12, "camera beyond the bound")
    assert int((img.sum(axis=2) > 0).sum()) > 100
    # the same context takes SURE again for the near camera (the predicate is asked per camera origin)
    near = esc.Camera.for_image(eye, look, 80, 12)
    assert frame(esc, renderer, near, 80, 12)[2]["sure"]
    inf = (float(eye[0]), float("inf"), float(eye[2]))
    assert not sc.shadow_origins_inside(inf)
    with pytest.raises(esc.EscError):  # a camera that is not finite is refused before any launch
        renderer.render(esc.Camera.for_image(inf, look, 80, 12), 80, 12)


def test_refused_by_flag(esc, renderer):
    renderer.upload(esc.Scene.synthetic("c3", 300))
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, 80, 12)
    assert frame(esc, renderer, cam, 80, 12)[2]["sure"]
    refused(esc, renderer, cam, 80, 12, "ESC_RENDER_VOTE", flags=esc.ESC_RENDER_VOTE)


def test_refused_light_with_face_draws(esc, renderer):
    two_faces = {"vertex": np.array([(-0.5, 8, 0), (0.5, 8, 0), (0.5, 8, -1), (-0.5, 8, -1)], F32),
                 "face_index": np.array([[0, 1, 2], [0, 2, 3]]), "material": ol.LIGHT_A}
    rng = np.random.default_rng(5)
    sph = np.concatenate([rng.uniform(-4, 4, (300, 1)), rng.uniform(0.3, 4, (300, 1)), rng.uniform(-4, 4, (300, 1)),
                          rng.uniform(0.1, 0.3, (300, 1))], axis=1).astype(F32)
    sc = ol.scene_to_product(ol.scene_dict([dict(FLOOR), two_faces], sph, grey(300)))
    renderer.upload(sc)
    eye, look = (0.0, 3.0, 9.0), (0.0, 2.0, 0.0)
    assert sc.shadow_origins_inside(eye)
    cam = esc.Camera.for_image(eye, look, 80, 12)
    refused(esc, renderer, cam, 80, 12, "per-pixel face draws", face_mode=esc.ESC_FACE_HASH, seed=7)
    # the same light with its face fixed offers one sample point: SURE again
    assert frame(esc, renderer, cam, 80, 12, fixed_face=1)[2]["sure"]


def test_tripwire_on_random_scenes(esc, renderer):
    w, h = 96, 24
    n_sure = n_frames = 0
    for seed in range(4, 84, 4):  # twenty scenes; multiples of 4 are sphere clouds under a one-face light
        d, _, look, _, _, vfov = random_scenes.random_scene(seed)
        sc = ol.scene_to_product(d)
        renderer.upload(sc)
        hdr = sc.table("header").view(F32)
        lo, hi = hdr[4:7].astype(np.float64), hdr[7:10].astype(np.float64)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        inside = mid + half * np.array([0.31, 0.22, -0.43])
        outside = mid + half * np.array([0.2, 1.04, 0.3])
        for eye in (inside, outside):
            eye = tuple(float(x) for x in eye.astype(F32))
            cam = esc.Camera.for_image(eye, look, w, h, vfov=vfov)
            img, u8, kern, trip = frame(esc, renderer, cam, w, h)
            n_frames += 1
            assert trip == 0, f"seed {seed}, camera {eye}: the tripwire is set"
            if not kern["sure"]:
                continue
            n_sure += 1
            assert sc.shadow_origins_inside(eye)
            img2, u82, kern2, _ = frame(esc, renderer, cam, w, h, flags=esc.ESC_RENDER_VOTE)
            assert not kern2["sure"]
            assert np.array_equal(bits(img), bits(img2)) and np.array_equal(u8, u82), \
                f"seed {seed}, camera {eye}: SURE and vote frames differ"
    print(f"SURE ran for {n_sure} of {n_frames} frames")
    assert n_sure >= 4, "the hunt never met the instantiation it is about"
