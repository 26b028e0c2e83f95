"""Batched ray queries (Renderer.intersect / occluded / intersect_rays / occluded_rays) against the
reference arithmetic.

The reference is the closest-hit / occlusion loop of main.cpp:176-192, 314-329 with the sphere
extension (oracle closest_hit / occlusion order: triangles geometry by geometry and face by face,
then spheres) of tests/ray_oracle.py, over its numpy restatement of orc_intersect_triangle /
orc_intersect_sphere.  test_numpy_restatement_pinned pins that restatement, pair by pair and bit
for bit, against the oracle's own C functions (it needs no GPU).  t, u and v are compared bit for
bit; NaN results (NaN or infinite inputs) compare as NaN, because NaN payloads are not portable
between processors.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import random_scenes as rs
from ray_cases import box, surface_points
from ray_oracle import EPS, F32, FLT_MAX, dot, normalize, ref_queries, same_bits, sph_test, tri_test


def check_equal(got, occ, ref, ref_occ, what=""):
    for k in ("t", "uv"):
        bad = ~same_bits(got[k], ref[k])
        assert not bad.any(), f"{what}: {k} differs at {np.argwhere(bad)[:5].tolist()}"
    for k in ("geom", "prim"):
        bad = got[k] != ref[k]
        assert not bad.any(), f"{what}: {k} differs at {np.argwhere(bad)[:5].tolist()}"
    if occ is not None:
        bad = occ != ref_occ
        assert not bad.any(), f"{what}: occlusion differs at {np.argwhere(bad)[:5].tolist()}"
        hit = (got["geom"] >= 0) | (got["prim"] >= 0)
        assert np.array_equal(hit.astype(np.uint8), occ), f"{what}: occlusion != closest hit found"


# ---- ray sets -------------------------------------------------------------------------------
def camera_rays(eye, look, W, H, vfov=60.0):
    """camera.h:31-34 get_ray over the pixel centres of a W x H image, in fp32 numpy"""
    import esctp1raytracer_amd as esc
    c = esc.Camera.for_image(eye, look, W, H, vfov=vfov).vectors()
    s = ((np.arange(W, dtype=F32) + F32(0.5)) / F32(W))[None, :].repeat(H, 0).reshape(-1)
    t = ((np.arange(H, dtype=F32) + F32(0.5)) / F32(H))[:, None].repeat(W, 1).reshape(-1)
    p = (c["lower_left_corner"] + c["horizontal"] * s[:, None]) + c["vertical"] * t[:, None]
    dirs = normalize(p - c["origin"])
    return np.broadcast_to(c["origin"], dirs.shape).astype(F32).copy(), dirs


def random_rays(d, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = box(d)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F32)
    return o, normalize(rng.standard_normal((n, 3)))


def n_prims(d):
    return sum(g["face_index"].shape[0] for g in d["geometry"]) + len(d["spheres"])


def rays_for_budget(d, cap=4096):
    return int(max(64, min(cap, 2_000_000 // max(1, n_prims(d)))))


# ---- oracle pin (no GPU) -------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_numpy_restatement_pinned():
    lib = ol.oracle()
    rng = np.random.default_rng(7)
    n = 4000
    o = rng.standard_normal((n, 3)).astype(F32)
    dirs = normalize(rng.standard_normal((n, 3)))
    dirs[::7] *= F32(2.0)
    dirs[1::7] *= F32(1e-3)
    dirs[2::97] = 0.0
    dirs[3::97, 1] = np.nan
    dirs[4::97, 2] = np.inf
    tri = rng.standard_normal((3, 3)).astype(F32) * F32(0.8)
    o[5::3] = (tri[0] + 0.3 * (tri[1] - tri[0]) + 0.3 * (tri[2] - tri[0]) + rng.standard_normal(3) * 2).astype(F32)
    dirs[5::3] = normalize(tri[0] + 0.3 * (tri[1] - tri[0]) + 0.3 * (tri[2] - tri[0]) - o[5::3])
    sph = np.array([0.1, -0.2, 0.3, 0.9], F32)
    tin = np.where(rng.uniform(size=n) < 0.5, FLT_MAX, rng.uniform(0, 4, n)).astype(F32)
    ok, t2, u2, v2 = tri_test(o, dirs, tri[0], tri[1], tri[2])
    sok, st2 = sph_test(o, dirs, sph)
    n_acc = 0
    for i in range(n):
        oi = np.ascontiguousarray(o[i])
        di = np.ascontiguousarray(dirs[i])
        t = C.c_float(tin[i])
        u = C.c_float(0)
        v = C.c_float(0)
        a = lib.orc_intersect_triangle(_fp(oi), _fp(di), _fp(tri[0]), _fp(tri[1]), _fp(tri[2]),
                                       C.byref(t), C.byref(u), C.byref(v))
        mine = bool(ok[i] and not (t2[i] >= tin[i]))
        assert a == mine, i
        if a:
            n_acc += 1
            assert same_bits(np.array([t.value, u.value, v.value], F32),
                             np.array([t2[i], u2[i], v2[i]], F32)).all(), i
        t = C.c_float(tin[i])
        a = lib.orc_intersect_sphere(_fp(oi), _fp(di), _fp(sph), C.byref(t))
        assert a == bool(sok[i] and not (st2[i] >= tin[i])), i
        if a:
            n_acc += 1
            assert same_bits(np.array([t.value], F32), st2[i:i + 1]).all(), i
    assert n_acc > 500


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r():
    import esctp1raytracer_amd as esc
    rr = esc.Renderer(0)
    yield rr
    rr.close()


def run_both(r, d, o, dirs, tmax=None, what="", exact_too=True):
    import esctp1raytracer_amd as esc
    r.upload(ol.scene_to_product(d))
    ref, ref_occ = ref_queries(d, o, dirs, tmax)
    for exact in ((False, True) if exact_too else (False,)):
        got = r.intersect(o, dirs, tmax, exact=exact)
        occ = r.occluded(o, dirs, tmax, exact=exact)
        check_equal(got, occ, ref, ref_occ, f"{what} exact={exact}")
    assert isinstance(esc.Renderer.query_stats(r), dict)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two", "CornellBox-Original"])
def test_camera_rays_pinned_scenes(r, name):
    d = {"one": ol.scene_one, "two": ol.scene_two}[name]() if name in ("one", "two") else ol.load_dump(name)
    eye, look = ((0, 1, 3), (0, 1, 0)) if name in ("one", "two") else ((0, 1, 3.5), (0, 1, 0))
    o, dirs = camera_rays(eye, look, 64, 48)
    ref = run_both(r, d, o, dirs, what=name)
    assert (ref["geom"] >= 0).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [9, 18, 27, 3, 5, 36])
def test_random_scenes_light_and_grazing_rays(r, seed):
    d, eye, look, W, H, vfov = rs.random_scene(seed)
    rng = np.random.default_rng(seed)
    n = rays_for_budget(d, 3000)
    lo, hi = box(d)
    size = float(np.max(hi - lo))
    # surface points towards the lights (the light's first vertex, quirk S2), t bounded by the distance
    p = surface_points(d, n, rng)
    lp = np.stack([d["geometry"][li]["vertex"][0] for li in d["light_sources"]])
    target = lp[rng.integers(0, len(lp), len(p))]
    dirs = normalize(target - p)
    tmax = np.sqrt(dot((target - p).astype(F32), (target - p).astype(F32))).astype(F32)
    run_both(r, d, p, dirs, tmax, what=f"seed {seed} lights")
    # grazing: in the plane of a flat patch (or of y = const through the box), origins 1e-7 .. 1e-3
    # of the scene's size off it, directions nearly in it
    y0 = float(d["geometry"][0]["vertex"][:, 1].mean()) if d["geometry"] else float(lo[1])
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F32)
    o[:, 1] = y0 + size * 10.0 ** rng.uniform(-7, -3, n) * rng.choice([-1.0, 1.0], n)
    g = rng.standard_normal((n, 3))
    g[:, 1] = g[:, 1] * 10.0 ** rng.uniform(-7, -2, n)
    run_both(r, d, o, normalize(g), what=f"seed {seed} grazing")


@pytest.mark.gpu
def test_inside_spheres_and_far_origins(r):
    d, *_ = rs.random_scene(8)  # spheres, a few large ones
    rng = np.random.default_rng(1)
    n = rays_for_budget(d, 2000)
    s = d["spheres"][rng.integers(0, len(d["spheres"]), n)]
    o = (s[:, :3] + rng.uniform(-0.5, 0.5, (n, 3)) * s[:, 3:]).astype(F32)
    run_both(r, d, o, normalize(rng.standard_normal((n, 3))), what="inside spheres")
    lo, hi = box(d)
    c = (lo + hi) / 2
    far = (c + normalize(rng.standard_normal((n, 3))) * F32(20 * np.max(hi - lo))).astype(F32)
    dirs = normalize(c + rng.uniform(-0.3, 0.3, (n, 3)) * (hi - lo) - far)
    run_both(r, d, far, dirs, what="far origins", exact_too=False)
    st = r.query_stats()
    assert st["rays"] == n and st["exact_rays"] == n


@pytest.mark.gpu
def test_non_unit_zero_nan_inf_directions(r):
    d, *_ = rs.random_scene(3)
    rng = np.random.default_rng(2)
    n = rays_for_budget(d, 2000)
    o, dirs = random_rays(d, n, 3)
    dirs = dirs.copy()
    dirs[0::6] *= F32(2.0)
    dirs[1::6] *= F32(1e-3)
    dirs[2::6] = 0.0
    dirs[3::12, 0] = np.nan
    dirs[4::12, 1] = np.inf
    dirs[9::12, 2] = -np.inf
    o[10::24, 0] = np.nan
    run_both(r, d, o, dirs, what="odd directions")
    assert r.query_stats()["exact_rays"] >= (n * 4) // 6


@pytest.mark.gpu
def test_per_ray_tmax(r):
    d = ol.load_dump("CornellBox-Original")
    o, dirs = camera_rays((0, 1, 3.5), (0, 1, 0), 48, 40)
    n = o.shape[0]
    rng = np.random.default_rng(4)
    run_both(r, d, o, dirs, np.where(rng.uniform(size=n) < 0.5, EPS, F32(0.5) * EPS).astype(F32),
             what="tmax <= eps")
    first = ref_queries(d, o, dirs)[0]
    hit = first["geom"] >= 0
    tmax = np.where(hit, first["t"], FLT_MAX).astype(F32)  # strict: that very hit is rejected
    ref = run_both(r, d, o, dirs, tmax, what="tmax = hit t")
    # the hit at t == tmax is rejected: a nearer one, or a miss that returns the bound
    assert np.all((ref["t"][hit] < first["t"][hit]) |
                  ((ref["prim"][hit] < 0) & same_bits(ref["t"][hit], tmax[hit])))


def _tie_scene(n_extra_spheres):
    plane = np.array([(-1, -1, 0), (1, -1, 0), (0, 1.5, 0)], F32)
    geoms = [{"vertex": plane, "face_index": [[0, 1, 2]], "material": ol.WHITE},
             {"vertex": plane.copy(), "face_index": [[0, 1, 2]], "material": ol.RED},  # duplicate
             {"vertex": np.array([(-9, 5, 9), (9, 5, 9), (0, 5, -9)], F32), "face_index": [[0, 1, 2]],
              "material": ol.LIGHT_A}]
    rng = np.random.default_rng(5)
    extra = np.concatenate([rng.uniform(-6, 6, (n_extra_spheres, 3)) + [0, 0, -20],
                            rng.uniform(0.05, 0.3, (n_extra_spheres, 1))], 1)
    sph = np.concatenate([[[0, 0, -1, 1], [0, 0, -1, 1]], extra]).astype(F32)  # duplicate, tangent at z = 0
    mats = np.stack([ol.WHITE] * len(sph))
    return ol.scene_dict(geoms, sph, mats)


@pytest.mark.gpu
@pytest.mark.parametrize("n_extra", [0, 600])  # 600: the sphere groups are swept
def test_ties(r, n_extra):
    d = _tie_scene(n_extra)
    rng = np.random.default_rng(6)
    n = 1500
    o = np.zeros((n, 3), F32)
    o[:, :2] = rng.uniform(-0.02, 0.02, (n, 2))
    o[:, 2] = 5.0
    o[:8, :2] = 0.0
    dirs = np.zeros((n, 3), F32)
    dirs[:, 2] = -1.0
    ref = run_both(r, d, o, dirs, what=f"ties {n_extra}")
    assert ref["geom"][0] == 0 and ref["prim"][0] == 0 and ref["t"][0] == F32(5.0)
    # triangles removed: the two equal spheres tie, sphere 0 wins
    d2 = ol.scene_dict([d["geometry"][2]], d["spheres"], d["sphere_materials"])
    ref = run_both(r, d2, o, dirs, what=f"sphere ties {n_extra}")
    assert ref["geom"][0] == -1 and ref["prim"][0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "spheres_only", "triangles_only", "mixed"])
def test_scene_kinds(r, kind):
    if kind == "small":
        d = ol.scene_one()  # 4 triangles: no groups
    else:
        d, *_ = rs.random_scene({"spheres_only": 4, "triangles_only": 18, "mixed": 15}[kind])
        if kind == "spheres_only":
            d = ol.scene_dict([], d["spheres"], d["sphere_materials"])
    n = rays_for_budget(d, 3000)
    o, dirs = random_rays(d, n, 11)
    run_both(r, d, o, dirs, what=kind)


@pytest.mark.gpu
def test_flat_upload_ids_refer_to_the_array(r):
    import esctp1raytracer_amd as esc
    d = ol.load_dump("CornellBox-Original")
    flat = esc.FlatScene(ol.scene_to_product(d), sort_by_centroid_x=True)
    nt = flat.num_triangles
    verts = np.array([[list(flat.triangles[i].vertices[k]) for k in range(3)] for i in range(nt)], F32)
    gids = np.array([flat.triangles[i].geom_id for i in range(nt)], np.int32)
    one_each = ol.scene_dict([{"vertex": verts[i], "face_index": [[0, 1, 2]], "material": ol.WHITE}
                              for i in range(nt)])
    o, dirs = camera_rays((0, 1, 3.5), (0, 1, 0), 64, 48)
    ref, ref_occ = ref_queries(one_each, o, dirs)
    hit = ref["geom"] >= 0
    ref["prim"] = np.where(hit, ref["geom"], -1).astype(np.int32)
    ref["geom"] = np.where(hit, gids[np.maximum(ref["geom"], 0)], -1).astype(np.int32)
    r.upload(flat)
    check_equal(r.intersect(o, dirs), r.occluded(o, dirs), ref, ref_occ, "flat")
    assert hit.sum() > 100


@pytest.mark.gpu
def test_n_zero_and_a_million_rays_against_exact(r):
    import esctp1raytracer_amd as esc
    import torch
    sc = esc.Scene.synthetic("c4", 500)
    r.upload(sc)
    dev = torch.device("cuda", 0)
    e = torch.empty((0, 3), dtype=torch.float32, device=dev)
    t = torch.empty(0, dtype=torch.float32, device=dev)
    i32 = torch.empty(0, dtype=torch.int32, device=dev)
    r.intersect_rays(e, e, t, i32, i32.clone())
    r.occluded_rays(e, e, torch.empty(0, dtype=torch.uint8, device=dev))
    assert r.query_stats() == {"rays": 0, "exact_rays": 0, "exact_tests": 0}
    d = ol.scene_from_product(sc)
    n = 2 ** 20 + 17
    o, dirs = random_rays(d, n, 12)
    a = r.intersect(o, dirs)
    assert r.query_stats()["rays"] == n
    b = r.intersect(o, dirs, exact=True)
    assert r.query_stats()["exact_rays"] == n
    check_equal(a, None, b, None, "2^20 + 17")
    assert np.array_equal(r.occluded(o, dirs), r.occluded(o, dirs, exact=True))


@pytest.mark.gpu
def test_wrapper_argument_checks(r):
    import torch
    r.upload(ol.scene_to_product(ol.scene_one()))
    dev = torch.device("cuda", 0)
    o = torch.zeros((8, 3), dtype=torch.float32, device=dev)
    t = torch.empty(8, dtype=torch.float32, device=dev)
    g = torch.empty(8, dtype=torch.int32, device=dev)
    p = torch.empty(8, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        r.intersect_rays(o.double(), o, t, g, p)
    with pytest.raises(ValueError):
        r.intersect_rays(o, o[:4], t, g, p)
    with pytest.raises(ValueError):
        r.intersect_rays(o.cpu(), o, t, g, p)
    with pytest.raises(ValueError):
        r.intersect_rays(torch.zeros((3, 8), device=dev).t(), o, t, g, p)
    with pytest.raises(TypeError):
        r.occluded_rays(o, o, torch.empty(8, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        r.intersect_rays(o, o, t, g, p, uv=torch.empty((8, 3), device=dev))


# ---- large scenes: filtered == exact ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4", "water", "c5"])
def test_large_scenes_filtered_equals_exact(r, name):
    import esctp1raytracer_amd as esc
    if name == "water":
        sc = ol.scene_to_product(ol.load_dump("CornellBox-Water"))
        eye, look = (0, 1, 3.5), (0, 1, 0)
    else:
        sc = esc.Scene.synthetic(name)
        eye, look = esc.synthetic_view()
    r.upload(sc)
    info = sc.info()
    P = info["n_triangles"] + info["n_spheres"]
    W, H = (256, 144) if name != "c5" else (128, 72)
    o, dirs = camera_rays(eye, look, W, H)
    n = o.shape[0]
    a = r.intersect(o, dirs)
    st = r.query_stats()
    ao = r.occluded(o, dirs)
    b = r.intersect(o, dirs, exact=True)
    check_equal(a, None, b, None, f"{name} coherent")
    assert np.array_equal(ao, r.occluded(o, dirs, exact=True))
    assert st["exact_rays"] == 0
    if name == "c4":
        assert st["exact_tests"] < 0.01 * n * P, st
    lo, hi = box(ol.scene_from_product(sc))
    rng = np.random.default_rng(13)
    m = 8192 if name != "c5" else 4096
    o = (lo + rng.uniform(0, 1, (m, 3)) * (hi - lo)).astype(F32)
    dirs = normalize(rng.standard_normal((m, 3)))
    check_equal(r.intersect(o, dirs), None, r.intersect(o, dirs, exact=True), None, f"{name} incoherent")
    assert np.array_equal(r.occluded(o, dirs), r.occluded(o, dirs, exact=True))


# ---- no interference with rendering ---------------------------------------------------------------
@pytest.mark.gpu
def test_queries_leave_rendering_alone():
    import esctp1raytracer_amd as esc
    import torch
    r = esc.Renderer(0)
    sc = esc.Scene.synthetic("c4", 2000)
    r.upload(sc)
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, 320, 180)
    r.reset_counters()
    f1 = r.render(cam, 320, 180)
    c1 = r.counters()
    o, dirs = camera_rays(eye, look, 97, 61)
    r.intersect(o, dirs)
    r.occluded(o, dirs)
    assert r.counters() == c1
    f2 = r.render(cam, 320, 180)
    assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32))
    # a recorded frame launched after queries
    dev = torch.device("cuda", 0)
    out = torch.empty(320 * 180 * 3, dtype=torch.float32, device=dev)
    fr = r.record_strips(cam, 320, 180, 0, 1, out)
    r.intersect(o, dirs)
    out.zero_()
    r.synchronize()
    fr.launch()
    r.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(180, 320, 3).view(np.uint32), f1.view(np.uint32))
    fr.close()
    r.close()


@pytest.mark.gpu
def test_queries_on_a_torch_stream():
    import esctp1raytracer_amd as esc
    import torch
    d = ol.load_dump("CornellBox-Original")
    o, dirs = camera_rays((0, 1, 3.5), (0, 1, 0), 128, 96)
    ref, ref_occ = ref_queries(d, o, dirs)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=s)
    r.upload(ol.scene_to_product(d))
    n = o.shape[0]
    with torch.cuda.stream(s):
        to = torch.from_numpy(o).to(dev, non_blocking=False)
        td = torch.from_numpy(dirs).to(dev)
        t = torch.full((n,), -1.0, device=dev)
        g = torch.full((n,), -7, dtype=torch.int32, device=dev)
        p = torch.full((n,), -7, dtype=torch.int32, device=dev)
        uv = torch.full((n, 2), -1.0, device=dev)
        oc = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        r.intersect_rays(to, td, t, g, p, uv=uv)
        r.occluded_rays(to, td, oc)
        res = {"t": t.cpu().numpy(), "geom": g.cpu().numpy(), "prim": p.cpu().numpy(),
               "uv": uv.cpu().numpy()}
        occ = oc.cpu().numpy()
    check_equal(res, occ, ref, ref_occ, "torch stream")
    r.close()
