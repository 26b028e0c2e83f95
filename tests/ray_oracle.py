"""The CPU restatement that the ray tests compare the GPU with (queries, shading of caller rays, mirror
bounces, refraction): numpy fp32 with one rounding per operation, made of oracle pieces.  No scenes and no
pytest here; tests/ray_cases.py chooses scenes and rays with it.

  - the closest hit / occlusion loop of main.cpp:176-192, 314-329 with the sphere extension (triangles
    geometry by geometry and face by face, then spheres) over tri_test / sph_test, which
    test_ray_queries.py::test_numpy_restatement_pinned pins pair by pair to orc_intersect_*;
  - the colour of one arbitrary ray (ray_colours): orc_render of pixel (0, 0) of a 2x2 frame whose camera
    is built by hand with origin o and lower_left_corner a, so that its ray is
    (o, orc_camera_get_ray(cam, 0, 0)) and its colour is scan_row's (main.cpp:698-791) for that ray;
  - the bounce rule of include/esctp1_rt.h (at esc_trace_options) in `bounce`, and the loop around it in
    oracle_trace.  A new bounce rule is added to `bounce` and nowhere else.

How a level's colour comes out of orc_render for a bounce ray (o', d'): the hand-built camera's get_ray
gives normalize(lower_left_corner - origin), and d' = normalize(x).  With lower_left_corner = x * 2^40 the
subtraction returns x * 2^40 exactly whenever every component of o' lies under half an ulp of the matching
component of x * 2^40, and a power-of-two scale goes through normalize unchanged.  oracle_trace checks the
direction orc_camera_get_ray returns against d' for every ray and level ("usable").

NaN results compare as NaN (payloads are not portable between processors)."""
import ctypes as C

import numpy as np

import oracle_lib as ol

F32 = np.float32
U64 = np.uint64
EPS = F32(np.finfo(np.float32).eps)
FLT_MAX = F32(np.finfo(np.float32).max)
OFF, REFRACT, FRESNEL = 0, 1, 2
MODE_NAME = {OFF: "off", REFRACT: "refract", FRESNEL: "fresnel"}


def same_bits(a, b):
    a = np.ascontiguousarray(a, F32)
    b = np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(a, b, what):
    bad = ~same_bits(a, b)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[:4].tolist()}"


def dot(a, b):  # vec.h:95-101 / orc_dot: sum = 0; sum += a[i] * b[i]
    s = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, F32)
    for k in range(3):
        s = (s + a[..., k] * b[..., k]).astype(F32)
    return s


def cross(a, b):  # vec.h:103-109
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F32)


def normalize(v):  # vec.h:135 in fp32
    v = np.ascontiguousarray(v, F32)
    return (v / np.sqrt(dot(v, v))[..., None]).astype(F32)


# ---- closest hit and occlusion ------------------------------------------------------------------------
def tri_test(o, d, v0, v1, v2):
    """ray_triangle.h:7-46 for rays (o, d) against one triangle, every reject but `t2 >= t`:
    -> (ok, t2, u2, v2)"""
    with np.errstate(all="ignore"):
        e1 = (v1 - v0).astype(F32)
        e2 = (v2 - v0).astype(F32)
        pv = cross(d, np.broadcast_to(e2, d.shape))
        det = dot(np.broadcast_to(e1, d.shape), pv).astype(np.float64)
        ok = ~((det > -EPS) & (det < EPS))
        inv = 1.0 / det
        tv = o - v0
        u2 = (dot(tv, pv).astype(np.float64) * inv).astype(F32)
        ok &= ~((u2 < EPS) | (u2 > F32(1)))
        qv = cross(tv, np.broadcast_to(e1, d.shape))
        v2 = (dot(d, qv).astype(np.float64) * inv).astype(F32)
        ok &= ~((v2 < EPS) | ((u2 + v2) > F32(1)))
        t2 = (dot(np.broadcast_to(e2, d.shape), qv).astype(np.float64) * inv).astype(F32)
        ok &= ~(t2 < EPS)
    return ok, t2, u2, v2


def sph_test(o, d, sph):
    """orc_intersect_sphere (oracle/rt_oracle.c) without `t2 >= t`: -> (ok, t2)"""
    with np.errstate(all="ignore"):
        oc = o - sph[:3]
        b = dot(oc, d)
        cc = dot(oc, oc) - sph[3] * sph[3]
        disc = b * b - cc
        ok = ~(disc < F32(0))
        sq = np.sqrt(disc)
        t2 = -b - sq
        t2 = np.where(t2 < EPS, -b + sq, t2).astype(F32)
        ok &= ~(t2 < EPS)
    return ok, t2


def ref_queries(d, o, dirs, tmax=None):
    """closest hit and occlusion of every ray, in the reference's order, t carried from tmax"""
    o = np.ascontiguousarray(o, F32)
    dirs = np.ascontiguousarray(dirs, F32)
    n = o.shape[0]
    t0 = np.full(n, FLT_MAX, F32) if tmax is None else np.ascontiguousarray(tmax, F32).copy()
    t = t0.copy()
    uv = np.zeros((n, 2), F32)
    geom = np.full(n, -1, np.int32)
    prim = np.full(n, -1, np.int32)
    occ = np.zeros(n, bool)
    for gi, g in enumerate(d["geometry"]):
        vert, fi = g["vertex"], g["face_index"]
        for f in range(fi.shape[0]):
            ok, t2, u2, v2 = tri_test(o, dirs, vert[fi[f, 0]], vert[fi[f, 1]], vert[fi[f, 2]])
            occ |= ok & ~(t2 >= t0)
            acc = ok & ~(t2 >= t)
            t[acc] = t2[acc]
            uv[acc, 0] = u2[acc]
            uv[acc, 1] = v2[acc]
            geom[acc] = gi
            prim[acc] = f
    for k, s in enumerate(d["spheres"]):
        ok, t2 = sph_test(o, dirs, s)
        occ |= ok & ~(t2 >= t0)
        acc = ok & ~(t2 >= t)
        t[acc] = t2[acc]
        uv[acc] = 0
        geom[acc] = -1
        prim[acc] = k
    return {"t": t, "geom": geom, "prim": prim, "uv": uv}, occ.astype(np.uint8)


def normals_and_ks(d, hit, o, dirs):
    """main.cpp:723-738 (quirk S1: u == 0) through orc_cross / orc_normalize, and the hit's ks"""
    lib = ol.oracle()
    n = o.shape[0]
    N = np.zeros((n, 3), F32)
    ks = np.zeros((n, 3), F32)
    has = np.zeros(n, bool)
    out = np.zeros(3, F32)
    for i in range(n):
        g, p = int(hit["geom"][i]), int(hit["prim"][i])
        if g >= 0:
            G = d["geometry"][g]
            f = G["face_index"][p]
            e1 = (G["vertex"][f[1]] - G["vertex"][f[0]]).astype(F32)
            e2 = (G["vertex"][f[2]] - G["vertex"][f[0]]).astype(F32)
            cr = np.zeros(3, F32)
            lib.orc_cross(ol.fp(e1), ol.fp(e2), ol.fp(cr))
            lib.orc_normalize(ol.fp(cr), ol.fp(out))
            if len(G["normals"]):
                u, v = F32(0), F32(hit["uv"][i, 1])
                a = ((G["normals"][f[1]] * u).astype(F32) + (G["normals"][f[2]] * v).astype(F32)).astype(F32)
                a = (a + (G["normals"][f[0]] * F32(F32(F32(1) - u) - v)).astype(F32)).astype(F32)
                lib.orc_normalize(ol.fp(np.ascontiguousarray(a)), ol.fp(out))
            N[i] = out
            ks[i] = G["material"][6:9]
            has[i] = True
        elif p >= 0:
            s = d["spheres"][p]
            pt = ((o[i] + (dirs[i] * hit["t"][i]).astype(F32)).astype(F32) - s[:3]).astype(F32)
            lib.orc_normalize(ol.fp(np.ascontiguousarray(pt)), ol.fp(out))
            N[i] = out
            ks[i] = d["sphere_materials"][p][6:9]
            has[i] = True
    return N, ks, has


# ---- the colour of one ray ----------------------------------------------------------------------------
def ray_colours(d, origins, llc, fixed_face=0, shadows=True, horizontal=(1, 0, 0)):
    """per ray: a hand-built orc_camera (origin o_i, lower_left_corner llc_i); its pixel (0, 0) of a 2x2
    frame is scan_row's colour for (o_i, get_ray(cam, 0, 0)).  -> (dirs, rgb)

    The frame's row 0 has a second pixel.  With horizontal = (0, 0, 0) it is the same ray as pixel (0, 0),
    whose colour is unchanged (llc + (1, 0, 0) * 0 and llc + 0 * 0 are the same sum), and that is asserted:
    then every power the oracle takes inside is one of the ray that is compared, and a pow table's miss
    counter speaks of those rays alone."""
    lib = ol.oracle()
    osc = ol.OracleScene(d)
    opts = ol.orc_options(1 if shadows else 0, ol.ORC_FACE_FIXED, fixed_face, 0, ol.ORC_QUIRK_ALL)
    n = origins.shape[0]
    dirs, rgb = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    img, out, cnt = np.zeros((2, 2, 3), F32), np.zeros(3, F32), ol.orc_counters()
    for i in range(n):
        cam = ol.orc_camera()
        for k in range(3):
            cam.origin[k] = float(origins[i, k])
            cam.lower_left_corner[k] = float(llc[i, k])
            cam.horizontal[k] = float(horizontal[k])
            cam.vertical[k] = (0.0, 1.0, 0.0)[k]
        lib.orc_camera_get_ray(C.byref(cam), C.c_float(0), C.c_float(0), ol.fp(out))
        dirs[i] = out
        img[:] = 0
        lib.orc_render(C.byref(osc.c), C.byref(cam), 2, 2, 0, 1, C.byref(opts), ol.fp(img), C.byref(cnt), 1)
        if not any(horizontal):
            assert np.array_equal(img[0, 0].view(np.uint32), img[0, 1].view(np.uint32)) or np.isnan(img[0]).any()
        rgb[i] = img[0, 0]
    return dirs, rgb


# ---- the rule of include/esctp1_rt.h in numpy ---------------------------------------------------------
def mix_hi32(seed, pixel, light=0xFFFFFFFF):
    """the light-face hash's 64-bit mixer (splitmix64's finaliser), high 32 bits, before the modulo"""
    with np.errstate(over="ignore"):
        z = U64(seed % (1 << 64)) + ((pixel.astype(U64) << U64(32)) | U64(light)) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return (z >> U64(32)).astype(np.uint32)


def bounce(o, dr, t0, N, ks, tr, w, mode, seed_k, q, bias, swap_bias=False):
    """one bounce of every ray -> (go, o', x, w', what) with d' = normalize(x); what: 0 mirror (or the path
    ends), 1 refracted, 2 fresnel_reflected, 3 total_internal.  swap_bias puts the origins of a
    transmissive hit on the wrong sides (the bias case shows that this changes the result)."""
    one, two = F32(1), F32(2)
    bias = F32(bias)
    tf, ni = tr[:, :3], tr[:, 3]
    glass = (mode != OFF) & ((tf[:, 0] > 0) | (tf[:, 1] > 0) | (tf[:, 2] > 0)) & (ni > 0)
    s = dot(dr, N)
    pos = s > 0
    Nf = np.where(pos[:, None], -N, N).astype(F32)
    c1 = np.where(pos, s, -s).astype(F32)
    eta = np.where(pos, ni, one / ni).astype(F32)
    k = (one - ((eta * eta).astype(F32) * (one - (c1 * c1).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    tir = glass & ~(k >= 0)
    sq = np.sqrt(k).astype(F32)
    fres = np.zeros(len(o), bool)
    if mode == FRESNEL:
        r0 = ((ni - one).astype(F32) / (ni + one).astype(F32)).astype(F32)
        r0 = (r0 * r0).astype(F32)
        cx = np.where(pos, sq, c1).astype(F32)
        m = (one - cx).astype(F32)
        m2 = (m * m).astype(F32)
        Fr = (r0 + ((one - r0).astype(F32) * ((m2 * m2).astype(F32) * m).astype(F32)).astype(F32)).astype(F32)
        u = ((mix_hi32(seed_k, q) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
        fres = glass & ~tir & (u < Fr)
    reflect = tir | fres
    refr = glass & ~reflect
    P = (o + (dr * t0[:, None]).astype(F32)).astype(F32)
    nb = (Nf * bias).astype(F32)
    near, far = (P + nb).astype(F32), (P - nb).astype(F32)
    if swap_bias:
        o2 = np.where(glass[:, None], np.where(refr[:, None], near, far), near)
    else:
        o2 = np.where(refr[:, None], far, near)
    xr = (dr - (N * (two * s).astype(F32)[:, None]).astype(F32)).astype(F32)
    xt = ((dr * eta[:, None]).astype(F32) + (Nf * ((eta * c1).astype(F32) - sq).astype(F32)[:, None]).astype(F32))
    x = np.where(refr[:, None], xt.astype(F32), xr)
    w2 = np.where(glass[:, None], np.where(reflect[:, None], w, (w * tf).astype(F32)), (w * ks).astype(F32))
    go = (glass & reflect) | (w2[:, 0] > 0) | (w2[:, 1] > 0) | (w2[:, 2] > 0)
    what = np.where(refr & go, 1, np.where(fres, 2, np.where(tir, 3, 0)))
    return go, o2.astype(F32), x.astype(F32), w2.astype(F32), what


def reflect(o, dirs, t0, N, bias):
    """bounce's mirror branch alone, (o', x, d'), for the tests that compose a trace of millions of rays
    from the public GPU calls; test_ray_oracle_cpu.py holds it to bounce"""
    s = dot(dirs, N)
    Nf = np.where((s > 0)[:, None], -N, N).astype(F32)
    o2 = ((o + (dirs * t0[:, None]).astype(F32)).astype(F32) + (Nf * F32(bias)).astype(F32)).astype(F32)
    x = (dirs - (N * (F32(2) * s).astype(F32)[:, None]).astype(F32)).astype(F32)
    with np.errstate(all="ignore"):
        return o2, x, normalize(x)


def transmission_rows(d, hit):
    """the side table's entry (tf, ni) of every ray's hit; (0, 0, 0, 1) where there is none"""
    tr = np.tile(np.array([0, 0, 0, 1], F32), (len(hit["geom"]), 1))
    for i, (g, p) in enumerate(zip(hit["geom"], hit["prim"])):
        if g >= 0:
            tr[i] = d.get("transmission", {}).get(int(g), tr[i])
        elif p >= 0:
            tr[i] = d.get("sphere_transmission", {}).get(int(p), tr[i])
    return tr


def oracle_trace(d, o, targets, max_depth, bias, mode=OFF, fixed_face=0, shadows=True, seed=77, pixel_base=1234,
                 swap_bias=False, colours=ray_colours):
    """-> {"dirs", "rgb", "usable", "depth_rays", "hit_rays0", "refracted", "fresnel_reflected",
    "total_internal"}.  The three counters count the rays a branch sent on to the next level, as
    esc_transmit_stats does, so that with the mirror bounces they add up to depth_rays of the following
    level.  colours: a callable with ray_colours' signature that gives each level's colours, or None: only
    level 0 is coloured (for its directions) and "rgb" and "usable" say nothing about the bounces."""
    n = o.shape[0]
    dirs0, c = (colours or ray_colours)(d, o, targets, fixed_face, shadows)
    Cc = c.copy()
    usable = np.ones(n, bool)
    counts = [n] + [0] * 16
    ev = [0, 0, 0, 0]
    idx = np.arange(n)
    co, cd, w = o.copy(), dirs0.copy(), np.ones((n, 3), F32)
    hits0 = 0
    with np.errstate(all="ignore"):
        for k in range(max_depth):
            if len(idx) == 0:
                break
            hit, _ = ref_queries(d, co, cd)
            N, ks, has = normals_and_ks(d, hit, co, cd)
            if k == 0:
                hits0 = int(has.sum())
            q = ((pixel_base + idx) % (1 << 32)).astype(np.uint32)
            go, o2, x, w, what = bounce(co, cd, hit["t"], N, ks, transmission_rows(d, hit), w, mode, seed + 64 * k,
                                        q, bias, swap_bias)
            go &= has
            for j in (1, 2, 3):
                ev[j] += int(((what == j) & go).sum())
            d2 = normalize(x)
            idx, co, cd, w, x = idx[go], o2[go], d2[go], w[go], x[go]
            counts[k + 1] = len(idx)
            if len(idx) == 0:
                break
            if colours is not None:
                got_d, c = colours(d, co, (x * F32(2.0 ** 40)).astype(F32), fixed_face, shadows)
                usable[idx[~same_bits(got_d, cd).all(axis=1)]] = False
                Cc[idx] = (Cc[idx] + (w * c).astype(F32)).astype(F32)
    return {"dirs": dirs0, "rgb": Cc, "usable": usable, "depth_rays": counts, "hit_rays0": hits0,
            "refracted": ev[1], "fresnel_reflected": ev[2], "total_internal": ev[3]}


def stats_of(want):
    """oracle_trace's result as esc_transmit_stats reports it"""
    return {k: want[k] for k in ("refracted", "fresnel_reflected", "total_internal")}
