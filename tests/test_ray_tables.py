"""GPU: k_frame takes the column and row terms of its primary rays from two per-context tables (csrc/rt_device.h
RayTables, csrc/rt_kernels.hip k_prepare_ray_tables, csrc/rt_capi.cpp; DESIGN.md 4 "Ray tables") instead of
dividing per pixel.  The tables are filled by primary_dir's own statements, so nothing may change:

 1. same image: frames of the default path equal, as uint32 bits on every pixel, the same frame under
    ESC_RENDER_TWO_KERNELS (k_primary + k_shade: still the divides), esc_camera_rays + esc_shade_rays on the same
    pixels, and the CPU oracle -- at 67x13, 130x9, 64x8, 33x5 and 129x17 (partial tiles to the right and below,
    one full tile, less than a wave's width, more than one tile each way), on a 300-sphere cut of c4 and on the
    committed OBJ fixture `two`; as the whole frame and as ranks 1 and 2 of 3 with 8-row strips (h_tile, a short
    last strip; a rank without rows is not rendered); fp32 and bytes.  The API refuses W < 2 and H < 2, so W - 1
    = 0 cannot be asked for;
 2. table lifetime: camera A, camera B, camera A again, then A at another size in ONE context, each frame equal to
    the same frame from a fresh context; a frame recorded before a camera change reports invalid after it -- also
    when only the view direction changes and no tile lists are asked for, so that nothing but the ray tables'
    key ends it;
 3. the context's allocations are gone after it is destroyed.
"""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = ((67, 13), (130, 9), (64, 8), (33, 5), (129, 17))


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as esc
    return esc


@pytest.fixture(scope="module")
def renderer(esc):
    r = esc.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes(esc):
    """name -> (product scene, oracle scene, eye, look)"""
    sc = esc.Scene.synthetic("c4", 300)
    eye, look = esc.synthetic_view()
    d = ol.load_dump("two")
    return {"spheres": (sc, ol.OracleScene(ol.scene_from_product(sc)), eye, look),
            "two": (ol.scene_to_product(d), ol.OracleScene(d), (0.0, 1.0, 3.0), (0.0, 1.0, 0.0))}


_ORACLE = {}


def oracle_frame(scenes, name, w, h):
    """computed once per (scene, size), never written to"""
    key = (name, w, h)
    if key not in _ORACLE:
        _, osc, eye, look = scenes[name]
        img = ol.oracle_render(osc, eye, look, w, h, threads=4)
        img.setflags(write=False)
        _ORACLE[key] = img
    return _ORACLE[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def strip_rows_of(h, rank, stride, strip=8):
    return [r for k in range(rank, (h + strip - 1) // strip, stride) for r in range(k * strip, min(k * strip + strip, h))]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["spheres", "two"])
def test_same_image(esc, renderer, scenes, name, size):
    import torch
    w, h = size
    sc, _, eye, look = scenes[name]
    renderer.upload(sc)
    cam = esc.Camera.for_image(eye, look, w, h)
    ref = oracle_frame(scenes, name, w, h)
    ref8 = ol.oracle_quantise(ref)
    assert np.any(ref)
    # the whole frame: k_frame
    img, u8 = renderer.render(cam, w, h, want_u8=True)
    assert renderer.last_frame_kernel()["fused"], "the default path did not take k_frame"
    assert np.array_equal(bits(img), bits(ref)), f"{name} {w}x{h}: k_frame differs from the oracle"
    assert np.array_equal(u8, ref8), f"{name} {w}x{h}: k_frame's bytes differ from the oracle's"
    # k_primary + k_shade: primary_dir's divides
    img2, u82 = renderer.render(cam, w, h, want_u8=True, flags=esc.ESC_RENDER_TWO_KERNELS)
    assert not renderer.last_frame_kernel()["fused"]
    assert np.array_equal(bits(img), bits(img2)), f"{name} {w}x{h}: k_frame differs from the two-kernel frame"
    assert np.array_equal(u8, u82)
    # esc_camera_rays + esc_shade_rays: rt_camera_ray.h's divides
    o, d = renderer.camera_rays(cam, w, h)
    rgb = torch.empty((w * h, 3), dtype=torch.float32, device=o.device)
    rgb8 = torch.empty((w * h, 3), dtype=torch.uint8, device=o.device)
    renderer.shade_rays(o, d, rgb, rgb8=rgb8)
    renderer.synchronize()
    assert np.array_equal(bits(img).reshape(-1, 3), bits(rgb.cpu().numpy())), \
        f"{name} {w}x{h}: k_frame differs from shaded camera rays"
    assert np.array_equal(u8.reshape(-1, 3), rgb8.cpu().numpy())
    # ranks 1 and 2 of 3, 8-row strips
    for rank in (1, 2):
        rows = strip_rows_of(h, rank, 3)
        assert esc.strip_local_rows(h, 8, rank, 3) == len(rows)
        if not rows:
            continue
        of = torch.zeros(len(rows) * w * 3, dtype=torch.float32, device="cuda:0")
        ob = torch.zeros(len(rows) * w * 3, dtype=torch.uint8, device="cuda:0")
        renderer.render_strips(cam, w, h, rank, 3, out_f32=of, out_u8=ob)
        assert renderer.last_frame_kernel()["fused"]
        renderer.synchronize()
        assert np.array_equal(bits(of.cpu().numpy()).reshape(len(rows), w, 3), bits(ref[rows])), \
            f"{name} {w}x{h}: rank {rank} of 3 differs from the oracle's rows {rows[0]}..{rows[-1]}"
        assert np.array_equal(ob.cpu().numpy().reshape(len(rows), w, 3), ref8[rows])


def fresh_frame(esc, sc, cam, w, h):
    r = esc.Renderer(0)
    try:
        r.upload(sc)
        return r.render(cam, w, h, want_u8=True)
    finally:
        r.close()


def test_table_lifetime(esc, scenes):
    sc, _, eye, look = scenes["spheres"]
    look_b = (look[0] + 1.5, look[1] + 0.5, look[2])
    eye_c = (eye[0] + 0.75, eye[1] + 0.25, eye[2] - 0.5)
    cams = [("A", eye, look, 67, 13), ("B: another direction", eye, look_b, 67, 13), ("A again", eye, look, 67, 13),
            ("C: another origin", eye_c, look, 67, 13), ("A at 130x9", eye, look, 130, 9),
            ("A at 33x21", eye, look, 33, 21), ("A once more", eye, look, 67, 13)]
    r = esc.Renderer(0)
    try:
        r.upload(sc)
        for what, e, l, w, h in cams:
            cam = esc.Camera.for_image(e, l, w, h)
            img, u8 = r.render(cam, w, h, want_u8=True)
            assert r.last_frame_kernel()["fused"]
            ref, ref8 = fresh_frame(esc, sc, cam, w, h)
            assert np.any(ref)
            assert np.array_equal(bits(img), bits(ref)), f"camera {what}: differs from a fresh context's frame"
            assert np.array_equal(u8, ref8)
    finally:
        r.close()


@pytest.mark.parametrize("flags", ["default", "no tile lists"])
def test_recorded_frame_ends_with_the_tables(esc, renderer, scenes, flags):
    import torch
    fl = esc.ESC_RENDER_NO_TILE_LISTS if flags == "no tile lists" else 0
    sc, _, eye, look = scenes["spheres"]
    renderer.upload(sc)
    w, h = 67, 13
    cam = esc.Camera.for_image(eye, look, w, h)
    buf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda:0")
    ref = renderer.render(cam, w, h, flags=fl)
    f = renderer.record_strips(cam, w, h, 0, 1, out_f32=buf, flags=fl)
    try:
        assert f.valid()
        f.launch()
        renderer.synchronize()
        assert np.array_equal(bits(buf.cpu().numpy()), bits(ref).reshape(-1))
        # the same call again (camera, size and strips: the host-frame path above renders one tall band, which
        # is another tile-list key): the tables stand
        renderer.render_strips(cam, w, h, 0, 1, out_f32=buf, flags=fl)
        assert f.valid()
        # the same origin, another direction: llc / horizontal / vertical change, nothing per-origin does
        turned = esc.Camera.for_image(eye, (look[0] + 1.5, look[1] + 0.5, look[2]), w, h)
        renderer.render_strips(turned, w, h, 0, 1, out_f32=buf, flags=fl)
        assert not f.valid(), "a recorded frame outlived the ray tables it reads"
        with pytest.raises(esc.EscError):
            f.launch()
    finally:
        f.close()


def test_allocations_return(esc, renderer, scenes):
    sc, _, eye, look = scenes["spheres"]
    before = esc.live_device_allocations()
    r = esc.Renderer(0)
    try:
        r.upload(sc)
        for w, h in ((67, 13), (130, 9)):
            r.render(esc.Camera.for_image(eye, look, w, h), w, h)
        during = esc.live_device_allocations()
        assert during[0] > before[0]
    finally:
        r.close()
    assert esc.live_device_allocations() == before
