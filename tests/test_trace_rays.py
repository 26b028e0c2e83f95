"""Mirror reflections on the GPU (esc_trace_rays / esc_render_traced, rt_trace.hip), bit for bit:
depth 0 is esc_shade_rays; bounces against the CPU restatement of tests/ray_oracle.py (oracle_trace with
transmission off: the index-order closest hit pinned to orc_intersect_*, orc_cross / orc_normalize for the
normal, the reflection in numpy fp32 as include/esctp1_rt.h writes it, each level's colour by orc_render
through a hand-built camera); large scenes composed from the public shade / intersect calls; odd inputs
against exact mode; no interference with frames, queries and shading.

The cases and their rays come from tests/ray_cases.py: trace_case_rays() keeps only rays for which the
hand-built camera reproduces every bounce direction at every level of the deepest setting (chosen by the
oracle alone, before anything runs on the GPU), and every case asserts that all of its rays are compared.

powf: the device's and the host libm's differ in the last bit (ray_cases.py's docstring).  With Ns = 0
on the edited materials every bit is compared; for the `_ns` cases the tolerance of
test_big_mesh_smooth_normals applies (rtol = atol = 1e-5, at least 90 % of the values bit-equal, u8 within
1), and depth_rays must still equal the oracle's counts exactly."""
import numpy as np
import pytest

import oracle_lib as ol
from ray_cases import CORNELL_EYE, CORNELL_LOOK, TRACE_CASES, trace_case_rays, with_ks
from ray_oracle import F32, assert_same, cross, normalize, oracle_trace, reflect, same_bits


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


# ---- 2. bounces against the CPU restatement ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,max_depth,bias,shadows", TRACE_CASES)
def test_bounces_against_the_oracle(esc, r, name, max_depth, bias, shadows):
    d, o, a = trace_case_rays(name)
    bias = float(F32(bias))
    res = oracle_trace(d, o, a, max_depth, bias, shadows=shadows)
    dirs, want, usable, counts, hits0 = (res[k] for k in ("dirs", "rgb", "usable", "depth_rays", "hit_rays0"))
    # the oracle alone must bounce, or the comparison below shows nothing
    assert hits0 > 0 and counts[1] * 10 >= hits0, (counts, hits0)
    if max_depth >= 2:
        assert counts[2] >= 1, counts
    assert usable.all(), np.flatnonzero(~usable).tolist()  # every ray is compared (see trace_case_rays)
    r.upload(ol.scene_to_product(d))
    one_face = all(len(d["geometry"][g]["face_index"]) == 1 for g in d["light_sources"])
    for mode in (esc.ESC_FACE_FIXED, esc.ESC_FACE_HASH):
        for exact in (False, True):
            got = r.trace(o, dirs, max_depth=max_depth, bias=bias, shadows=shadows, face_mode=mode, seed=77,
                          pixel_base=1234, exact=exact)
            st = r.trace_stats()
            assert st["depth_rays"] == counts, (st["depth_rays"], counts)
            assert st["rays"] == sum(counts)
            if (mode == esc.ESC_FACE_FIXED or one_face) and not name.endswith("_ns"):
                assert_same(got["rgb"], want, f"{name} mode {mode} exact {exact}")
                assert np.array_equal(got["rgb8"], ol.oracle_quantise(want))
            elif mode == esc.ESC_FACE_FIXED or one_face:  # Ns != 0: powf's last bit (module docstring)
                fin = np.isfinite(want)
                assert np.array_equal(fin, np.isfinite(got["rgb"]))
                assert np.allclose(got["rgb"][fin], want[fin], rtol=1e-5, atol=1e-5)
                assert same_bits(got["rgb"], want).mean() > 0.9
                assert np.abs(got["rgb8"].astype(int) - ol.oracle_quantise(want).astype(int)).max() <= 1
            if exact:
                assert_same(got["rgb"], filtered["rgb"], f"{name} mode {mode}: filtered vs exact")
            filtered = got


# ---- 1. depth 0 is the old behaviour ----------------------------------------------------------------
def _scene(esc, name):
    if name in ("one", "two"):
        return ol.scene_to_product(ol.load_dump(name)), (0, 1, 3), (0, 1, 0)
    if name in ("cornell", "water"):
        d = ol.load_dump("CornellBox-Original" if name == "cornell" else "CornellBox-Water")
        return ol.scene_to_product(d), CORNELL_EYE, CORNELL_LOOK
    return esc.Scene.synthetic(name), *esc.synthetic_view()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two", "cornell", "water", "c2", "c3"])
def test_depth_zero_is_shade(esc, r, name):
    sc, eye, look = _scene(esc, name)
    r.upload(sc)
    W, H = 97, 61
    cam = esc.Camera.for_image(eye, look, W, H)
    o, d = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    o, d = o.cpu().numpy(), d.cpu().numpy()
    rng = np.random.default_rng(3)
    o2 = (o[0] + rng.standard_normal((4096, 3))).astype(F32)
    d2 = normalize(rng.standard_normal((4096, 3)))
    for oo, dd, what in ((o, d, "camera"), (o2, d2, "arbitrary")):
        for mode in (esc.ESC_FACE_FIXED, esc.ESC_FACE_HASH):
            want = r.shade(oo, dd, face_mode=mode, seed=9, pixel_base=5)
            got = r.trace(oo, dd, max_depth=0, bias=0.25, face_mode=mode, seed=9, pixel_base=5)
            assert_same(got["rgb"], want["rgb"], f"{name} {what}")
            assert np.array_equal(got["rgb8"], want["rgb8"])
            st = r.trace_stats()
            assert st["depth_rays"][0] == len(oo) and sum(st["depth_rays"][1:]) == 0
    # every ks of these scenes' diffuse materials ends a path: a deeper trace changes nothing where
    # no material has ks > 0
    img = r.render_traced(cam, W, H, max_depth=0, bias=0.0)
    assert_same(img, r.render(cam, W, H), f"{name} frame")
    assert_same(r.render_traced(cam, W, H, spp=4, max_depth=0, bias=0.0), r.render_supersampled(cam, W, H, 4),
                f"{name} spp 4")


@pytest.mark.gpu
def test_a_scene_without_ks_never_bounces(esc, r):
    sc = esc.Scene.synthetic("c4", 2000)  # Lambertian spheres: every ks is 0
    _, mats = sc.spheres()
    assert not np.any(mats[:, 6:9])
    r.upload(sc)
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, 320, 180)
    want = r.render(cam, 320, 180)
    for depth in (1, 16):
        assert_same(r.render_traced(cam, 320, 180, max_depth=depth, bias=1e-3), want, f"depth {depth}")
        st = r.trace_stats()
        assert st["depth_rays"][0] == 320 * 180 and st["depth_rays"][1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two"])
def test_depth_zero_frames_give_the_reference_md5(esc, r, name, tmp_path):
    import hashlib
    sc, eye, look = _scene(esc, name)
    r.upload(sc)
    cam = esc.Camera.for_image(eye, look, 1024, 768)
    img, u8 = r.render_traced(cam, 1024, 768, spp=1, max_depth=0, bias=0.0, want_u8=True)
    want, want8 = r.render(cam, 1024, 768, want_u8=True)
    assert_same(img, want, name)
    assert np.array_equal(u8, want8)
    md5 = {"one": "b10e1cb14f839129bd111670002cfb0b", "two": "c8137a8d70d8de0ad6a001d41be4e0e1"}[name]
    p = tmp_path / "x.ppm"
    esc.write_ppm(p, u8)
    assert hashlib.md5(p.read_bytes()).hexdigest() == md5


@pytest.mark.gpu
def test_depth_zero_c4_at_4k_is_render(esc, r):
    r.upload(esc.Scene.synthetic("c4"))
    W, H = 3840, 2160
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    img, u8 = r.render_traced(cam, W, H, spp=1, max_depth=0, bias=0.0, want_u8=True)
    want, want8 = r.render(cam, W, H, want_u8=True)
    assert_same(img, want, "c4 4K")
    assert np.array_equal(u8, want8)
    assert r.trace_stats()["depth_rays"][0] == W * H


# ---- 3. large scenes, composed from the public GPU calls -------------------------------------------
def _mirror_c4(esc, n=10000):
    sc = esc.Scene.synthetic("c4", n)
    sp, mats = sc.spheres()
    rng = np.random.default_rng(4)
    sel = rng.uniform(size=len(mats)) < 1 / 3
    mats = mats.copy()
    mats[sel, 6:9] = rng.uniform(0.2, 0.9, (int(sel.sum()), 3))
    geoms = [sc.geometry(i) for i in range(sc.info()["n_geometry"])]
    return ol.scene_dict(geoms, sp, mats)


@pytest.mark.gpu
def test_c4_4k_composed_from_shade_and_intersect(esc, r):
    d = _mirror_c4(esc)
    r.upload(ol.scene_to_product(d))
    eye, look = esc.synthetic_view()
    W, H, bias = 3840, 2160, float(F32(1e-3))
    cam = esc.Camera.for_image(eye, look, W, H)
    got = r.render_traced(cam, W, H, max_depth=2, bias=bias, seed=5).reshape(-1, 3)
    st = r.trace_stats()
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    o, dd = o.cpu().numpy(), dd.cpu().numpy()
    n = W * H
    Cc = np.zeros((n, 3), F32)
    idx = np.arange(n)
    w = np.ones((n, 3), F32)
    counts = [n, 0, 0]
    with np.errstate(all="ignore"):
        for k in range(3):
            sh = r.shade(o, dd, seed=5 + 64 * k)  # fixed face: the pixel id does not matter
            Cc[idx] = sh["rgb"] if k == 0 else (Cc[idx] + (w * sh["rgb"]).astype(F32)).astype(F32)
            if k == 2:
                break
            hit = sh["prim"] >= 0  # c4's primitives that get hit are spheres and the light's triangles
            sph = (sh["geom"] < 0) & hit
            ks = np.zeros((len(idx), 3), F32)
            ks[sph] = d["sphere_materials"][sh["prim"][sph]][:, 6:9]
            N = np.zeros((len(idx), 3), F32)
            pt = ((o + (dd * sh["t"][:, None]).astype(F32)).astype(F32)[sph] - d["spheres"][sh["prim"][sph], :3])
            N[sph] = normalize(pt.astype(F32))
            w = (w * ks).astype(F32)
            go = sph & ((w[:, 0] > 0) | (w[:, 1] > 0) | (w[:, 2] > 0))
            o2, _, d2 = reflect(o, dd, sh["t"], N, bias)
            if k == 0:
                hits0 = int(hit.sum())
            idx, o, dd, w = idx[go], o2[go], d2[go], w[go]
            counts[k + 1] = len(idx)
    assert counts[1] * 10 >= hits0 and counts[2] >= 1, (counts, hits0)
    assert st["depth_rays"][:3] == counts, (st["depth_rays"], counts)
    assert_same(got, Cc, "c4 4K depth 2")
    # filtered == exact on a seeded sample of 2^16 of the level-0 rays
    o0, d0 = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    pick = np.random.default_rng(8).choice(n, 1 << 16, replace=False)
    o0, d0 = o0.cpu().numpy()[pick], d0.cpu().numpy()[pick]
    a = r.trace(o0, d0, max_depth=2, bias=bias)
    b = r.trace(o0, d0, max_depth=2, bias=bias, exact=True)
    assert_same(a["rgb"], b["rgb"], "c4 filtered vs exact")
    assert_same(a["rgb"], got[pick], "c4 rays vs frame")


def _tri_normals(G, prim, v):
    """main.cpp:728-738 (quirk S1: u == 0) for hits on geometry G, vectorised in fp32"""
    f = G["face_index"][prim]
    V = G["vertex"]
    N = normalize(cross((V[f[:, 1]] - V[f[:, 0]]).astype(F32), (V[f[:, 2]] - V[f[:, 0]]).astype(F32)))
    if len(G["normals"]):
        n = G["normals"]
        a = ((n[f[:, 1]] * F32(0)).astype(F32) + (n[f[:, 2]] * v[:, None]).astype(F32)).astype(F32)
        N = normalize((a + (n[f[:, 0]] * ((F32(1) - F32(0)) - v)[:, None]).astype(F32)).astype(F32))
    return N


@pytest.mark.gpu
def test_c5_8k_in_bands_composed_from_shade_and_intersect(esc, r):
    sc = esc.Scene.synthetic("c5")
    d = ol.scene_from_product(sc)
    mesh = max(range(len(d["geometry"])), key=lambda g: len(d["geometry"][g]["face_index"]))
    d["geometry"][mesh]["material"][6:9] = 0.5
    G = d["geometry"][mesh]
    r.upload(ol.scene_to_product(d))
    W, H, band, bias = 7680, 4320, 540, float(F32(1e-3))
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    got = r.render_traced(cam, W, H, max_depth=2, bias=bias)  # 116 B a ray: some 15 bands of 256 MB
    st = r.trace_stats()
    counts, hits0 = [0, 0, 0], 0
    rng = np.random.default_rng(8)
    sample = []
    with np.errstate(all="ignore"):
        for r0 in range(0, H, band):
            o, dd = r.camera_rays(cam, W, H, rows=(r0, r0 + band))
            r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
            o, dd = o.cpu().numpy(), dd.cpu().numpy()
            n = len(o)
            if len(sample) < 8:
                pick = rng.choice(n, 1 << 13, replace=False)
                sample.append((r0 * W + pick, o[pick], dd[pick]))
            Cc = np.zeros((n, 3), F32)
            idx, w = np.arange(n), np.ones((n, 3), F32)
            for k in range(3):
                counts[k] += len(idx)
                sh = r.shade(o, dd)
                Cc[idx] = sh["rgb"] if k == 0 else (Cc[idx] + (w * sh["rgb"]).astype(F32)).astype(F32)
                if k == 2 or len(idx) == 0:
                    break
                on = sh["geom"] == mesh
                if k == 0:
                    hits0 += int((sh["prim"] >= 0).sum())
                v = r.intersect(o[on], dd[on])["uv"][:, 1]
                N = _tri_normals(G, sh["prim"][on], v)
                o2, _, d2 = reflect(o[on], dd[on], sh["t"][on], N, bias)
                w = (w[on] * G["material"][6:9]).astype(F32)
                idx, o, dd = idx[on], o2, d2
            assert_same(got[r0:r0 + band].reshape(-1, 3), Cc, f"c5 rows {r0}..")
    assert counts[1] * 10 >= hits0 and counts[2] >= 1, (counts, hits0)
    assert st["depth_rays"][:3] == counts, (st["depth_rays"], counts)
    # filtered == exact on a seeded sample of 2^16 of the frame's rays
    pix = np.concatenate([p for p, _, _ in sample])
    o0, d0 = np.concatenate([x for _, x, _ in sample]), np.concatenate([x for _, _, x in sample])
    a = r.trace(o0, d0, max_depth=2, bias=bias)
    b = r.trace(o0, d0, max_depth=2, bias=bias, exact=True)
    assert_same(a["rgb"], b["rgb"], "c5 filtered vs exact")
    assert_same(a["rgb"], got.reshape(-1, 3)[pix], "c5 rays vs frame")


# ---- 4. odd inputs equal exact mode -------------------------------------------------------------------
@pytest.mark.gpu
def test_odd_inputs_match_exact(esc, r):
    d = with_ks(ol.load_dump("CornellBox-Original"), 5, share=1.0)
    r.upload(ol.scene_to_product(d))
    rng = np.random.default_rng(2)
    n = 4096
    o = (np.array([0, 1, 0.5], F32) + rng.uniform(-0.4, 0.4, (n, 3))).astype(F32)
    dd = normalize(rng.standard_normal((n, 3)))
    odd = [np.zeros(3), np.array([3.0, 0, 0]), np.array([1e30, 0, 0]), np.array([np.nan, 0, 1]),
           np.array([np.inf, 0, 0]), np.array([0, -1e-30, 0])]
    for j, v in enumerate(odd):
        dd[j::64][: n // 128] = v.astype(F32)
        o[j + 8::64][: n // 128] = (v * 1e3).astype(F32)
    dd[20::64] = np.array([1, 0, 0], F32)  # along the floor and the walls: s is +-0 on axis-aligned faces
    o[20::64, 1] = 0.0
    for bias in (0.0, 1e-4, 1e22):
        a = r.trace(o, dd, max_depth=4, bias=bias)
        sa = r.trace_stats()
        b = r.trace(o, dd, max_depth=4, bias=bias, exact=True)
        sb = r.trace_stats()
        assert_same(a["rgb"], b["rgb"], f"bias {bias}")
        assert np.array_equal(a["rgb8"], b["rgb8"])
        assert sa["depth_rays"] == sb["depth_rays"] and sa["depth_rays"][1] > 0
        assert sa["exact_rays"] > 0  # the odd rays (and, with the huge bias, the bounces) fail the gate
        if bias > 1:
            assert sa["exact_rays"] >= sa["depth_rays"][1]


# ---- 5. no interference --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tracing_leaves_everything_else_alone(esc):
    import torch
    r = esc.Renderer(0)
    d = with_ks(ol.load_dump("CornellBox-Original"), 5, share=1.0)
    r.upload(ol.scene_to_product(d))
    W, H = 160, 90
    cam = esc.Camera.for_image(CORNELL_EYE, CORNELL_LOOK, W, H)
    o, dd = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    on, dn = o.cpu().numpy(), dd.cpu().numpy()
    frame = r.render(cam, W, H)
    query = r.intersect(on, dn)
    shade = r.shade(on, dn)
    dev = torch.device("cuda", 0)
    out = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
    rec = r.record_strips(cam, W, H, 0, 1, out)
    r.reset_counters()
    r.render(cam, W, H)
    c1 = r.counters()
    big = r.trace(on, dn, max_depth=3, bias=1e-4)
    small = r.trace(on[:1000], dn[:1000], max_depth=3, bias=1e-4)
    assert_same(small["rgb"], big["rgb"][:1000], "n = 1000 after n = 14400")
    again = r.trace(np.concatenate([on, on]), np.concatenate([dn, dn]), max_depth=3, bias=1e-4)  # regrowth
    assert_same(again["rgb"][: W * H], big["rgb"], "after the scratch grew")
    assert_same(again["rgb"][W * H:], big["rgb"], "second half: pixel ids do not matter with a fixed face")
    assert r.trace(on[:0], dn[:0], max_depth=3, bias=0.0)["rgb"].shape == (0, 3)
    assert_same(r.render(cam, W, H), frame, "frame after tracing")
    q2 = r.intersect(on, dn)
    for k in ("t", "geom", "prim"):
        assert np.array_equal(q2[k], query[k]), k
    assert_same(r.shade(on, dn)["rgb"], shade["rgb"], "shade after tracing")
    r.render_traced(esc.Camera.for_image(CORNELL_EYE, (0.3, 1, 0), 97, 61), 97, 61, spp=4, max_depth=2, bias=1e-4)
    r.reset_counters()
    r.render(cam, W, H)
    assert r.counters() == c1
    out.zero_()
    r.synchronize()
    rec.launch()
    r.synchronize()
    assert_same(out.cpu().numpy().reshape(H, W, 3), frame, "recorded frame after tracing")
    rec.close()
    r.close()
    # a caller's torch stream
    s = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=s)
    r.upload(ol.scene_to_product(d))
    with torch.cuda.stream(s):
        o, dd = r.camera_rays(cam, W, H)
        rgb = torch.full((W * H, 3), -1.0, device=dev)
        r.trace_rays(o, dd, rgb, max_depth=3, bias=1e-4)
        got = rgb.cpu().numpy()
    assert_same(got, big["rgb"], "torch stream")
    # argument checks
    for kw in ({"max_depth": -1, "bias": 0.0}, {"max_depth": 17, "bias": 0.0}, {"max_depth": 1, "bias": -1.0},
               {"max_depth": 1, "bias": float("nan")}, {"max_depth": 1, "bias": float("inf")}):
        with pytest.raises(esc.EscError) as e:
            r.trace(on[:4], dn[:4], **kw)
        assert e.value.code == -1 and ("max_depth" in str(e.value) or "bias" in str(e.value))
    r.close()
