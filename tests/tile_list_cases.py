"""Scenes, cameras and the reference's answer for the membership of the primary tile lists
(csrc/rt_lists.h: k_bin_spheres, k_bin_triangles, k_bin_tri_escape).  Plain module: no pytest and no GPU.
tests/test_tile_list_cases_cpu.py shows on the reference alone that every case does what it was built for,
tests/test_tile_list_members.py reads the lists of a rendered frame back and holds them to `needed`.

What a list must hold.  A primary ray tests the slots of its 32 x 4 pixel tile's list and the short global
list, nothing else.  Primitive q is NEEDED in tile T iff some pixel of T has a ray the reference does not
reject before `t2 >= t` (ray_oracle.tri_test / sph_test, pinned pair by pair to the oracle by
test_ray_queries.py::test_numpy_restatement_pinned): an accept with t carried from FLT_MAX, whether or not a
nearer primitive hides it.  A frame comparison sees a missing entry only where the primitive is the closest
hit of that tile; `needed` does not care.

A case is a dict: "scene" (the scene dict of oracle_lib), "cam" (the four camera vectors as an object with
.c, as Renderer takes it), "W", "H", "pieces" (the partition the frame is rendered in) and what the case
declares about itself.  Primitives are placed in IMAGE coordinates -- the point at (s, t, depth) is
o + depth (A + s H + t V), camera.h:31-34 -- so one layout serves every camera, lens and image plane.

Pieces.  ("rows", r0, r1) is esc_render_rows over rows [r0, r1): local row lr is image row r0 + lr.
("strips", strip_rows, first, stride) is esc_render_strips: the image is cut into strips of strip_rows rows
counted from h = 0, the call renders strips first, first + stride, ... packed in ascending h.  Local tile
row j holds local rows [4 j, 4 j + 4), tile (tx, j) the pixels [32 tx, 32 tx + 32) of them; the lists are
indexed j * tiles_x + tx (local_rows restates the partition; the product's code is not asked).

Slivers.  rt_lists.h sends a triangle to the global list when rho <= 0x1.4p-10 emax, rho being the largest
distance of a vertex from the centroid and emax = max(|e1|, |e2|).  One end of the longer of e1, e2 is at
least emax / 2 from any point, so rho >= emax / 2 for every triangle with finite coordinates: no triangle
has rho near 2^-10 emax, and that branch is left to exactly degenerate input (e1 = 0, or e1 and e2
parallel in exact arithmetic).  The sliver case therefore takes its three ratios 0.9, 1.1 and 1.5 x 2^-10
for the triangle's HEIGHT over emax (needles, which the rectangle, the hull and the dilation all have to
cope with), adds exactly degenerate triangles, and declares only the latter as possible globals.
"""
import functools
import types

import numpy as np

import esctp1raytracer_amd as esc
import oracle_lib as ol
import ray_oracle as ro

F32 = np.float32
F64 = np.float64
PAD_SLOT = (2 ** 31 - 1) // 2  # what sg_orig / tg_orig hold for a pad slot
TILE_W, TILE_H = 32, 4
GLOBAL_CAP = 64  # rt_device.h kTileGlobalCap


# ---- cameras and rays ---------------------------------------------------------------------------------
def ref_dirs(cam, W, H):
    """unit directions of every pixel exactly as the reference computes them (fp32, same order)"""
    o = np.array(cam.origin, F32)
    llc = np.array(cam.lower_left_corner, F32)
    hor = np.array(cam.horizontal, F32)
    ver = np.array(cam.vertical, F32)
    s = (np.arange(W, dtype=F32) / F32(W - 1)).astype(F32)
    t = (np.arange(H, dtype=F32) / F32(H - 1)).astype(F32)
    p = ((llc[None, None, :] + hor[None, None, :] * s[None, :, None]).astype(F32) +
         (ver[None, None, :] * t[:, None, None]).astype(F32)).astype(F32)
    p = (p - o[None, None, :]).astype(F32)
    n2 = ((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]).astype(F32) + p[..., 2] * p[..., 2]).astype(F32)
    n = np.sqrt(n2).astype(F32)
    return (p / n[..., None]).astype(F32)  # [H, W, 3]


def camera_struct(eye, look, W, H, skew=None, vfov=60.0):
    cam = esc.Camera.for_image(eye, look, W, H, vfov=vfov).c
    if skew is not None:  # an image plane that is not a rectangle: the C ABI takes any four vectors
        h = np.array(cam.horizontal, F32)
        v = np.array(cam.vertical, F32)
        h2 = (h + F32(skew[0]) * v).astype(F32)
        v2 = (v + F32(skew[1]) * h).astype(F32)
        for k in range(3):
            cam.horizontal[k] = h2[k]
            cam.vertical[k] = v2[k]
    return cam


def camera(eye, look, W, H, skew=None, vfov=60.0):
    """camera_struct as the object Renderer's calls take (.c)"""
    return types.SimpleNamespace(c=camera_struct(eye, look, W, H, skew, vfov))


def cam_vectors(cam):
    """(o, A, Hh, V) in float64: p(s, t) = A + s Hh + t V, A = llc - o"""
    c = cam.c
    o, llc = np.array(c.origin, F64), np.array(c.lower_left_corner, F64)
    return o, llc - o, np.array(c.horizontal, F64), np.array(c.vertical, F64)


def at_image(cam, s, t, depth):
    """the world point that pixel coordinates (s, t) in [0, 1]^2 see at `depth` image-plane distances"""
    o, A, Hh, V = cam_vectors(cam)
    s, t, depth = (np.asarray(x, F64) for x in (s, t, depth))
    return o + depth[..., None] * (A + s[..., None] * Hh + t[..., None] * V)


def pixel_of(cam, W, H, pts):
    """float64 pixel coordinates (w, h) and the depth b_3 . (X - o) of world points (n, 3): the image of
    the line from the camera through X, both nappes (depth < 0: behind the camera, point-mirrored)"""
    o, A, Hh, V = cam_vectors(cam)
    Binv = np.linalg.inv(np.stack([Hh, V, A], axis=1))  # rows b_1, b_2, b_3 of rt_lists.h
    q = (np.asarray(pts, F64) - o) @ Binv.T
    with np.errstate(all="ignore"):
        return q[:, 0] / q[:, 2] * (W - 1), q[:, 1] / q[:, 2] * (H - 1), q[:, 2]


def plane_distance(cam, pts):
    """signed distance of world points from the camera plane (through o, parallel to the image plane),
    positive in front"""
    o, A, Hh, V = cam_vectors(cam)
    n = np.cross(Hh, V)
    n /= np.linalg.norm(n)
    if n @ A < 0:
        n = -n
    return (np.asarray(pts, F64) - o) @ n


# ---- the partition ------------------------------------------------------------------------------------
def local_rows(piece, H):
    """image row of every local row of the piece, in the order the call packs them"""
    if piece[0] == "rows":
        return np.arange(piece[1], piece[2])
    _, strip_rows, first, stride = piece
    rows = []
    for k in range(first, (H + strip_rows - 1) // strip_rows, stride):
        rows += list(range(k * strip_rows, min((k + 1) * strip_rows, H)))
    return np.array(rows, int)


def tile_grid(piece, W, H):
    """(tiles_x, tile_rows) of the piece's lists"""
    return (W + TILE_W - 1) // TILE_W, (len(local_rows(piece, H)) + TILE_H - 1) // TILE_H


def tiles_of_image_box(piece, W, H, w0, w1, h0, h1, ring=1):
    """the local tiles (boolean, flat j * tiles_x + tx) that hold a pixel of the image rectangle
    [w0, w1] x [h0, h1] (inclusive pixel coordinates), the rectangle's tiles grown by `ring` tiles all round"""
    tiles_x, tile_rows = tile_grid(piece, W, H)
    rows = local_rows(piece, H)
    out = np.zeros((tile_rows, tiles_x), bool)
    tx0, tx1 = (int(w0) >> 5) - ring, (int(w1) >> 5) + ring
    j0, j1 = (int(h0) >> 2) - ring, (int(h1) >> 2) + ring
    for j in range(tile_rows):
        img_j = rows[4 * j:4 * j + 4] >> 2  # the image tile rows this local tile row holds rows of
        if ((img_j >= j0) & (img_j <= j1)).any():
            out[j, max(tx0, 0):max(tx1 + 1, 0)] = True
    return out.reshape(-1)


# ---- primitives ---------------------------------------------------------------------------------------
def triangles_of(d):
    """(n, 3, 3) fp32: the scene's triangles in the order of the original index (faces geometry by geometry)"""
    out = [g["vertex"][g["face_index"].astype(int)] for g in d["geometry"]]
    return np.concatenate(out).astype(F32) if out else np.zeros((0, 3, 3), F32)


# ---- the reference ------------------------------------------------------------------------------------
def rays(case, piece):
    """the reference's fp32 primary rays of the piece's rows: (origins, dirs), each (n_local_rows, W, 3)"""
    dirs = ref_dirs(case["cam"].c, case["W"], case["H"])[local_rows(piece, case["H"])]
    o = np.broadcast_to(np.array(case["cam"].c.origin, F32), dirs.shape)
    return np.ascontiguousarray(o), np.ascontiguousarray(dirs)


def _per_tile(ok, W):
    """[rows, W] bool -> [tile_rows * tiles_x] any"""
    n = ok.shape[0]
    tr, tx = (n + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    pad = np.zeros((tr * TILE_H, tx * TILE_W), bool)
    pad[:n, :W] = ok
    return pad.reshape(tr, TILE_H, tx, TILE_W).any(axis=(1, 3)).reshape(-1)


_analysis = {}


def analyse(case, k=0):
    """piece k of the case against the reference's tests, cached:
      "ok"      {0: [n_sph, rows, W] bool, 1: [n_tri, rows, W] bool}   tri_test / sph_test `ok` per pixel
      "needed"  {0: [tiles, n_sph] bool, 1: [tiles, n_tri] bool}
      "closest" (kind, prim) per pixel of the reference's closest hit (kind -1: none), main.cpp:176-192 order
    """
    key = (case["name"], k)
    if key in _analysis:
        return _analysis[key]
    d, W = case["scene"], case["W"]
    o, dirs = rays(case, case["pieces"][k])
    n_rows = dirs.shape[0]
    of, df = o.reshape(-1, 3), dirs.reshape(-1, 3)
    tris, sph = triangles_of(d), d["spheres"]
    ok = {0: np.zeros((len(sph), n_rows, W), bool), 1: np.zeros((len(tris), n_rows, W), bool)}
    t = np.full(len(of), ro.FLT_MAX, F32)
    kind = np.full(len(of), -1, int)
    prim = np.full(len(of), -1, int)
    for i, tv in enumerate(tris):
        m, t2, _, _ = ro.tri_test(of, df, tv[0], tv[1], tv[2])
        ok[1][i] = m.reshape(n_rows, W)
        acc = m & ~(t2 >= t)
        t[acc], kind[acc], prim[acc] = t2[acc], 1, i
    for i, s in enumerate(sph):
        m, t2 = ro.sph_test(of, df, s)
        ok[0][i] = m.reshape(n_rows, W)
        acc = m & ~(t2 >= t)
        t[acc], kind[acc], prim[acc] = t2[acc], 0, i
    needed = {w: (np.stack([_per_tile(a, W) for a in ok[w]], axis=1) if len(ok[w])
                  else np.zeros((_per_tile(np.zeros((n_rows, W), bool), W).size, 0), bool)) for w in (0, 1)}
    for a in list(ok.values()) + list(needed.values()):
        a.setflags(write=False)
    out = {"ok": ok, "needed": needed, "closest": (kind.reshape(n_rows, W), prim.reshape(n_rows, W))}
    _analysis[key] = out
    return out


def first_needed_pixel(case, k, which, tile, prim):
    """(w, h) image coordinates of the first pixel of `tile` that needs `prim`, for a failure's report"""
    tiles_x, _ = tile_grid(case["pieces"][k], case["W"], case["H"])
    j, tx = divmod(int(tile), tiles_x)
    blk = analyse(case, k)["ok"][which][prim][4 * j:4 * j + 4, 32 * tx:32 * tx + 32]
    lr, w = np.argwhere(blk)[0]
    return int(32 * tx + w), int(local_rows(case["pieces"][k], case["H"])[4 * j + lr])


def exact_inside(case, k, prim):
    """per pixel of piece k: does the LINE of the reference's fp32 ray, taken exactly (float64 on the fp32
    inputs), meet triangle `prim` inside it and in front of the origin?  The triangle's exact projection."""
    o, dirs = rays(case, case["pieces"][k])
    v = triangles_of(case["scene"])[prim].astype(F64)
    o, dd = o.astype(F64), dirs.astype(F64)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    pv = np.cross(dd, e2)
    det = pv @ e1
    tv = o - v[0]
    with np.errstate(all="ignore"):
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        vv = (dd * qv).sum(-1) / det
        t = (qv @ e2) / det
    return (det != 0) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (t > 0)


# ---- what rt_lists.h documents, restated (float64 unless the kernel says fp32) ---------------------------
def sphere_reach(case, centre, r2):
    """R of k_bin_spheres for a sorted record (centre fp32, r2 fp32), as documented:
    (sqrt(r2) + 0x1.2p-10 A1)(1 + 2^-20) + 2^-22 A1 + 2^-60, A1 = |centre - origin|_1"""
    o = np.array(case["cam"].c.origin, F64)
    A1 = np.abs(np.asarray(centre, F64) - o).sum()
    return (np.sqrt(F64(r2)) + float.fromhex("0x1.2p-10") * A1) * (1.0 + 2.0 ** -20) + 2.0 ** -22 * A1 + 2.0 ** -60


def tri_shape(v0, e1, e2):
    """rho (largest distance of a vertex from the centroid), emax, |n1|, l1 -- float64 on fp32 inputs"""
    e1, e2 = np.asarray(e1, F64), np.asarray(e2, F64)
    s3 = (e1 + e2) / 3.0
    rho = np.sqrt(max(s3 @ s3, (e1 - s3) @ (e1 - s3), (e2 - s3) @ (e2 - s3)))
    l1, l2 = np.sqrt(e1 @ e1), np.sqrt(e2 @ e2)
    return rho, max(l1, l2), np.linalg.norm(np.cross(e2, e1)), l1


def tri_corners(case, v0, e1, e2, kK=1.0):
    """the 12 corners v_i +- rho' e_a +- rho' e_b of (S_t) and the ball radius `slack` each is taken with:
    rho' = kK rho (1 + 1e-5) + slack, slack = 2^-20 (|v0 - o|_1 + |e1|_1 + |e2|_1) + 2^-60 -> ((12, 3), slack)"""
    o = np.array(case["cam"].c.origin, F64)
    v0, e1, e2 = np.asarray(v0, F64), np.asarray(e1, F64), np.asarray(e2, F64)
    rho, _, nn, l1 = tri_shape(v0, e1, e2)
    slack = 2.0 ** -20 * (np.abs(v0 - o).sum() + np.abs(e1).sum() + np.abs(e2).sum()) + 2.0 ** -60
    rp = kK * rho * (1.0 + 1e-5) + slack
    ea = e1 / l1
    eb = np.cross(np.cross(e2, e1), ea) / nn
    pts = [v + sa * rp * ea + sb * rp * eb for v in (v0, v0 + e1, v0 + e2) for sa in (-1, 1) for sb in (-1, 1)]
    return np.array(pts), slack


def tri_escape(v0, e1, e2, o, slack_k):
    """tri_escape_at / tri_escape of rt_lists.h in fp32 -> (possible, bounded, H, h): an accept through the
    `nearly parallel` escape at threshold tau / slack_k needs the origin within H of the plane; h is the
    origin's distance from it.  A doubtful triangle (no usable normal, tau too large) is possible, unbounded."""
    v0, e1, e2, o = (np.asarray(x, F32) for x in (v0, e1, e2, o))
    u = F32(2.0 ** -24)
    tv = (o - v0).astype(F32)
    at = F32(F32(abs(tv[0]) + abs(tv[1])) + abs(tv[2]))
    n1 = ro.cross(e2, e1)
    nn = np.sqrt(ro.dot(n1, n1))
    a1 = F32(F32(abs(e1[0]) + abs(e1[1])) + abs(e1[2]))
    a2 = F32(F32(abs(e2[0]) + abs(e2[1])) + abs(e2[2]))
    l1, l2 = np.sqrt(ro.dot(e1, e1)), np.sqrt(ro.dot(e2, e2))
    s3 = ((e1 + e2).astype(F32) * F32(1.0 / 3.0)).astype(F32)
    rho = np.sqrt(max(ro.dot(s3, s3), ro.dot((e1 - s3).astype(F32), (e1 - s3).astype(F32)),
                      ro.dot((e2 - s3).astype(F32), (e2 - s3).astype(F32))))
    emax = max(l1, l2)
    if not (rho > F32(float.fromhex("0x1.2p-10")) * emax) or not (nn > 0):
        return True, False, F32(0), F32(0)
    p12 = F32(a1 * a2)
    k = F32(F32(F32(F32(F32(3.2) * u) * emax) / rho) * F32(1.0001)) / F32(slack_k)
    tau = F32(k * F32(F32(F32(F32(10.04) * a2 + F32(5.04) * a1) * at) + F32(20.1) * p12))
    if not (tau < F32(0.1) * nn):
        return True, False, F32(0), F32(0)
    ted = F32(F32(tau + F32(10.05) * u * p12) * F32(1.0 + 4.0 * 2.0 ** -24))
    U, V = F32(ted + F32(10.04) * u * at * a2), F32(ted + F32(5.04) * u * at * a1)
    Hh = F32(F32(max(V / l1, U / l2) + at * tau / nn) * F32(2.0 * l1 * l2 / nn) * F32(1.0 / 0.99))
    h = F32(abs(ro.dot(tv, n1)) / nn)
    possible = not (h > F32(Hh * F32(1.01) + F32(2.0 ** -20) * at))
    return possible, True, Hh, h


def dilation_level(v, o):
    """-> (kK, cone): the dilation k_bin_triangles documents for triangle v (3, 3) fp32 seen from o -- the
    smallest of 1/8, 1/4, 1/2, 1 at which the camera cannot take the escape at all; cone: the camera can
    take it at k = 1 and the triangle leaves a cone entry"""
    v = np.asarray(v, F32)
    e1, e2 = (v[1] - v[0]).astype(F32), (v[2] - v[0]).astype(F32)
    possible, bounded, _, _ = tri_escape(v[0], e1, e2, o, 1.0)
    if possible:
        return 1.0, bounded
    for kc in (0.125, 0.25, 0.5):
        p, b, _, _ = tri_escape(v[0], e1, e2, o, kc)
        if b and not p:
            return kc, False
    return 1.0, False


def may_go_global(case):
    """{0: [n_sph] bool, 1: [n_tri] bool}: the primitives the case declares as possibly global, from the
    geometry rt_lists.h documents and nothing the kernels answer.  A sphere: the camera plane comes within
    1.001 R of its centre (its region of the image is unbounded).  A triangle: degenerate by the binning
    threshold (rho <= 0x1.4p-10 emax, no normal, e1 = 0); no usable escape bound (tri_escape: possible and
    unbounded); or its 12 corners at the LARGEST dilation (kK = 1) are not all on one side of the camera
    plane and further from it than 1.001 of their ball's radius."""
    d = case["scene"]
    o32 = np.array(case["cam"].c.origin, F32)
    sph = np.zeros(len(d["spheres"]), bool)
    for i, s in enumerate(d["spheres"]):
        R = sphere_reach(case, s[:3], F32(s[3] * s[3]))
        sph[i] = abs(plane_distance(case["cam"], s[None, :3].astype(F64))[0]) <= 1.001 * R
    tris = triangles_of(d)
    tri = np.zeros(len(tris), bool)
    for i, v in enumerate(tris):
        e1, e2 = (v[1] - v[0]).astype(F32), (v[2] - v[0]).astype(F32)
        rho, emax, nn, l1 = tri_shape(v[0], e1, e2)
        if not (rho > float.fromhex("0x1.4p-10") * emax) or not nn > 0 or not l1 > 0:
            tri[i] = True
            continue
        possible, bounded, _, _ = tri_escape(v[0], e1, e2, o32, 1.0)
        if possible and not bounded:
            tri[i] = True
            continue
        pts, slack = tri_corners(case, v[0], e1, e2, 1.0)
        dist = plane_distance(case["cam"], pts)
        tri[i] = not ((dist > 1.001 * slack).all() or (dist < -1.001 * slack).all())
    return {0: sph, 1: tri}


# ---- scenes -------------------------------------------------------------------------------------------
def _mat(c):
    return ol.material13(ka=c, kd=c)


LOWER = (0.03, 0.97, 0.04, 0.42)  # (s0, s1, t0, t1): the lower two fifths of the image
LEFT = (0.03, 0.47, 0.0, 1.0)     # the left half, every row (for frames rendered in pieces)
SMALL = (0.05, 1.0, 0.0, 0.45)    # 33 x 9: the first tile row of both tile columns (the second is 1 pixel wide)


def light_for(cam):
    """one small light triangle above and behind the camera: every scene is lit, none shows its light"""
    p = at_image(cam, 0.5, 3.0, -4.0)
    _, _, Hh, V = cam_vectors(cam)
    a, b = Hh / np.linalg.norm(Hh), V / np.linalg.norm(V)
    v = np.array([p, p + 0.2 * a, p + 0.2 * b])
    return {"vertex": v.astype(F32), "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_A}


def cloud_spheres(cam, n, region=LOWER, seed=1, depth=(6.0, 14.0), size=(0.015, 0.05)):
    """c2-like: n spheres spread over `region` of the image at several depths; radius in image-plane units"""
    rng = np.random.default_rng(seed)
    s, t = rng.uniform(region[0], region[1], n), rng.uniform(region[2], region[3], n)
    z = rng.uniform(depth[0], depth[1], n)
    _, _, Hh, _ = cam_vectors(cam)
    r = rng.uniform(size[0], size[1], n) * z * np.linalg.norm(Hh)
    return np.concatenate([at_image(cam, s, t, z), r[:, None]], axis=1)


def patch_triangles(cam, nx, ny, region=LOWER, depth=(7.0, 12.0), seed=2, wobble=0.25):
    """a tessellated patch, nx x ny quads of two triangles, over `region`; its depth runs from depth[0] at
    the left to depth[1] at the right and every vertex is moved a little, so no two triangles share a plane"""
    rng = np.random.default_rng(seed)
    s = np.linspace(region[0], region[1], nx + 1)
    t = np.linspace(region[2], region[3], ny + 1)
    S, T = np.meshgrid(s, t)
    Z = depth[0] + (depth[1] - depth[0]) * (S - region[0]) / (region[1] - region[0])
    Z = Z + wobble * rng.uniform(-1, 1, Z.shape)
    P = at_image(cam, S, T, Z)
    out = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, e = P[j, i], P[j, i + 1], P[j + 1, i + 1], P[j + 1, i]
            out += [[a, b, c], [a, c, e]]
    return np.array(out)


def scatter_triangles(cam, n, region=LOWER, seed=3, depth=(6.0, 14.0), size=0.03):
    """n small triangles spread over `region`, each turned its own way in the image and leaning a little
    in depth; `size`: the circumradius of its image, in image widths"""
    rng = np.random.default_rng(seed)
    s, t = rng.uniform(region[0], region[1], n), rng.uniform(region[2], region[3], n)
    z = rng.uniform(depth[0], depth[1], n)
    _, _, Hh, V = cam_vectors(cam)
    ang = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2])
    ds, dt = size * np.cos(ang), size * np.sin(ang) * np.linalg.norm(Hh) / np.linalg.norm(V)
    return at_image(cam, s[:, None] + ds, t[:, None] + dt, z[:, None] * (1 + rng.uniform(-0.03, 0.03, (n, 3))))


def scene(cam, tris=None, spheres=None):
    """the scene dict: one geometry of the case's triangles (their original indices are 0 .. n - 1), the
    light's triangle after them (original index n), the spheres"""
    geoms = []
    if tris is not None and len(tris):
        t = np.asarray(tris, F64).reshape(-1, 3)
        geoms.append({"vertex": t.astype(F32), "face_index": np.arange(len(t)).reshape(-1, 3),
                      "material": _mat((0.6, 0.6, 0.65))})
    geoms.append(light_for(cam))
    sp = None if spheres is None or not len(spheres) else np.asarray(spheres, F64).astype(F32)
    mats = None if sp is None else np.stack([_mat((0.4 + 0.002 * (k % 200), 0.5, 0.8)) for k in range(len(sp))])
    return ol.scene_dict(geoms, sp, mats)


def make_case(name, cam, W, H, tris=None, spheres=None, pieces=None, **declared):
    c = {"name": name, "cam": cam, "W": W, "H": H, "scene": scene(cam, tris, spheres),
         "pieces": pieces or [("rows", 0, H)], "ordinary": False, "expect_cones": False}
    c.update(declared)
    n_tri, n_sph = len(triangles_of(c["scene"])), len(c["scene"]["spheres"])
    c["kinds"] = [w for w, n in ((0, n_sph), (1, n_tri)) if n >= 64]  # the kinds that get lists
    assert c["kinds"] and n_tri <= 250 and n_sph <= 250, (name, n_tri, n_sph)
    assert W <= 192 and H <= 64
    return c


VIEWS = {
    "synthetic view": ((0, 3, 6), (0, 2, -8), None, 60.0),
    "cornell view": ((0, 1, 3), (0, 1, 0), None, 60.0),
    "far from the world origin": ((1000.5, 2003, -3006), (1000.5, 2002, -3020), None, 60.0),
    "skewed image plane": ((1, 2, 5), (0.5, 1, -4), (0.3, -0.2), 60.0),
    "narrow lens": ((0, 3, 6), (0, 2, -8), None, 5.0),
    "wide lens": ((0, 3, 6), (0, 2, -8), None, 140.0),
}


def _view(view, W, H):
    eye, look, skew, vfov = VIEWS[view]
    return camera(eye, look, W, H, skew, vfov)


def _ordinary(name, view, what, W=192, H=64, region=LOWER, pieces=None, ordinary=True, layers=1):
    cam = _view(view, W, H)
    sph = cloud_spheres(cam, 120, region) if what in ("spheres", "both") else None
    tri = None
    if what in ("triangles", "both"):  # (a second layer behind the first is needed like the first)
        tri = np.concatenate([patch_triangles(cam, 10, 5, region, (7.0 + 6 * k, 12.0 + 6 * k), seed=2 + k)
                              for k in range(layers)])
    return make_case(name, cam, W, H, tri, sph, pieces, ordinary=ordinary)


def _hidden(name, wall):
    """100 small spheres and 100 small triangles (the lower two fifths of the image, depth 8 to 14) behind a
    wall at depth 2 that covers the lower 55 % of the frame and far more to the sides and below: two large
    triangles, or one large sphere.  The frame shows the wall and, above it, nothing."""
    W, H = 192, 64
    cam = _view("synthetic view", W, H)
    sph = cloud_spheres(cam, 100, depth=(8.0, 14.0))
    tri = scatter_triangles(cam, 100, depth=(8.0, 14.0))
    if wall == "triangles":
        q = at_image(cam, np.array([-1.0, 2.0, 2.0, -1.0]), np.array([-2.0, -2.0, 0.55, 0.55]), np.full(4, 2.0))
        tri = np.concatenate([tri, np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]])])
    else:  # the sphere's upper limb passes through (0.5, 0.6) of the image; it is lower towards the sides
        o, A, Hh, V = cam_vectors(cam)
        top = A + 0.5 * Hh + 0.6 * V
        top /= np.linalg.norm(top)
        down = -V / np.linalg.norm(V)
        down = down - (down @ top) * top  # square to the tangent ray: the centre is R below it
        R = 40.0
        c = o + 2.0 * top + R * down / np.linalg.norm(down)
        sph = np.concatenate([sph, np.array([[c[0], c[1], c[2], R]])])
    return make_case(name, cam, W, H, tri, sph, hidden=(100, 100))


def _grazing(name, elev, dist=10.0):
    """the floor of test_gpu_parity.py::test_bvh_grazing_rays_on_large_triangles, 24 x 28 in the plane y = 0,
    as 6 x 8 quads (96 triangles 4 x 3.5 in size), its wall and its ceiling as 4 x 4 quads each; the camera
    `dist` from the floor's near edge and dist * elev above its plane looks along it at the floor's middle"""
    W, H = 192, 63  # (an odd H: the middle row's rays lie along the view direction, in the floor)
    R = _generic_rotation()  # the whole scene turned
    eye, look = R @ (0.3, dist * elev, 4.0 + dist), R @ (0.3, 0.0, -10.0)
    cam = types.SimpleNamespace(c=esc.Camera.for_image(tuple(eye), tuple(look), W, H, vup=tuple(R @ (0.0, 1.0, 0.0))).c)

    def quads(p00, du, dv, nu, nv):
        p00, du, dv = (np.asarray(x, F64) for x in (p00, du, dv))
        out = []
        for j in range(nv):
            for i in range(nu):
                a, b = p00 + i * du + j * dv, p00 + (i + 1) * du + j * dv
                c, e = p00 + (i + 1) * du + (j + 1) * dv, p00 + i * du + (j + 1) * dv
                out += [[R @ a, R @ b, R @ c], [R @ a, R @ c, R @ e]]
        return out

    floor = quads((-12, 0, 4), (4, 0, 0), (0, 0, -3.5), 6, 8)
    wall = quads((-12, 0, 4), (0, 0, -7), (0, 2.25, 0), 4, 4)
    ceil = quads((-12, 9, 4), (6, 0, 0), (0, 0, -7), 4, 4)
    return make_case(name, cam, W, H, np.array(floor + wall + ceil), None, n_floor=len(floor),
                     expect_cones=elev <= 1e-3)  # (at 1e-2 the camera is 0.1 above the plane, beyond every H_t)


def _generic_rotation():
    """0.7 rad about (1, 2, 3): in no axis-aligned plane the products of det, u and v cancel without rounding"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K


IN_PLANE_ROWS = (2, 10, 18, 26, 34, 42, 50, 58)


def _in_planes():
    """eight tessellated floors (5 x 3 quads each, 20 to 60 from the camera), each in the plane of the camera
    and one pixel row: every ray of those rows runs in the plane of 30 triangles, as nearly as fp32 vertices
    allow.  There det is rounding noise and so are the numerators of u and v: now and then a ray is accepted
    by a triangle its line passes far from -- accepts that only the cone entries of k_bin_tri_escape can
    serve (escape_only_pairs).  They are rare by nature (u and v must both land in (0, 1] by chance): this
    layout has three such (tile, triangle) pairs among 68 needed ones."""
    W, H = 192, 63
    R = _generic_rotation()
    cam = types.SimpleNamespace(c=esc.Camera.for_image(tuple(R @ (0.3, 1.0, 14.0)), tuple(R @ (0.3, 0.0, -10.0)), W, H,
                                                       vup=tuple(R @ (0.0, 1.0, 0.0))).c)
    tri = []
    for row in IN_PLANE_ROWS:
        s, z = np.meshgrid(np.linspace(0.08, 0.92, 6), np.linspace(20.0, 60.0, 4))
        P = at_image(cam, s, np.full(s.shape, row / (H - 1.0)), z)
        for j in range(3):
            for i in range(5):
                a, b, c, e = P[j, i], P[j, i + 1], P[j + 1, i + 1], P[j + 1, i]
                tri += [[a, b, c], [a, c, e]]
    return make_case("in the planes of eight rows", cam, W, H, np.array(tri), None, expect_cones=True)


def escape_only_pairs(case, k=0):
    """[tiles, n_tri] bool: needed pairs whose tile lies outside the tile box, grown by one ring, of the
    float64 images of the triangle's 12 corners at the largest dilation (kK = 1) -- accepts that statement
    (S_t) of rt_lists.h cannot account for, whatever the hull cuts: only (E_t) puts them in a list"""
    nd = analyse(case, k)["needed"][1]
    out = np.zeros_like(nd)
    for q, v in enumerate(triangles_of(case["scene"])):
        if not nd[:, q].any():
            continue
        pts, _ = tri_corners(case, v[0], v[1] - v[0], v[2] - v[0], 1.0)
        w, h, depth = pixel_of(case["cam"], case["W"], case["H"], pts)
        if not (depth > 0).all():
            continue
        box = tiles_of_image_box(case["pieces"][k], case["W"], case["H"], max(np.floor(w.min()), 0),
                                 max(np.floor(w.max()), 0), max(np.floor(h.min()), 0), max(np.floor(h.max()), 0))
        if w.max() < 0 or h.max() < 0:
            box[:] = False
        out[:, q] = nd[:, q] & ~box
    return out


DILATION_HEIGHTS = [2.0 ** (-16 + 0.25 * k) for k in range(56)]  # 1.5e-5 .. 0.21 below the camera


def _dilation():
    """one family of 56 identical triangles (translates of one: the same e1, e2 bit for bit) in planes y =
    const that pass 2^-16 .. 2^-2.25 under the camera, in steps of 2^(1/4): the camera's distance steps
    through the thresholds H(tau / k) of k = 1, 1/2, 1/4, 1/8, a factor of two apart.  Seen edge-on they all
    lie on the horizon; the camera is rolled so that the horizon runs across the frame, and a patch fills
    the rest of the list."""
    W, H = 192, 64
    eye = (0.0, 2.0, 0.0)
    cam = types.SimpleNamespace(c=esc.Camera.for_image(eye, (0.0, 2.0, -10.0), W, H, vup=(0.3, 1.0, 0.0)).c)
    fam = []
    for k, h in enumerate(DILATION_HEIGHTS):
        x, z = -6.0 + 0.25 * k, -6.0 - 0.125 * (k % 8)
        y = float(F32(2.0) - F32(h))
        fam.append([(x, y, z), (x + 0.75, y, z - 1.5), (x - 0.5, y, z - 1.0)])
    fam = np.array(fam)
    patch = patch_triangles(cam, 6, 4, (0.05, 0.45, 0.55, 0.95))
    return make_case("dilation levels", cam, W, H, np.concatenate([fam, patch]), None, family=len(fam),
                     expect_cones=True)


def _camera_plane():
    """primitives cut by the camera plane, touching it (within a hair of it, on either side), just in
    front of it, and wholly behind the camera -- among them a line of spheres and a line of triangles behind
    the camera whose images, point-mirrored, still cross the frame -- beside an ordinary cloud and patch.
    Coordinates (x, y, z) below are to the right, up and forward of the camera; the view reaches 60 degrees
    to the sides and 30 degrees up and down, and everything here stays in its lower half or at its sides."""
    W, H = 192, 64
    cam = _view("synthetic view", W, H)
    o, A, Hh, V = cam_vectors(cam)
    right, up = Hh / np.linalg.norm(Hh), V / np.linalg.norm(V)
    fwd = np.cross(right, up)
    fwd *= np.sign(fwd @ A)

    def at(x, y, z):
        return o + x * right + y * up + z * fwd

    sph = list(cloud_spheres(cam, 90))
    tri = list(patch_triangles(cam, 8, 4))
    own_sph = [((0.8, -0.3, 0.1), 0.5), ((-0.9, -0.4, -0.05), 0.6), ((0.5, -0.5, 0.0), 0.3),      # cut
               ((1.0, -0.5, 0.3), 0.29999), ((-1.0, -0.6, 0.25), 0.25001), ((0.7, -0.6, -0.2), 0.2),  # touching
               ((1.0, -0.4, 0.6), 0.35), ((-0.8, -0.5, 0.5), 0.3)]                                  # just in front
    sph += [list(at(*c)) + [r] for c, r in own_sph]
    for k in range(24):  # a line of spheres behind the camera, from upper right to upper left: mirrored, below
        sph.append(list(at(1.5 - 0.125 * k, 0.3 + 0.02 * k, -(3.0 + 0.1 * k))) + [0.1 + 0.005 * k])
    own_tri = []
    for k in range(6):   # strips of a floor under the camera, from in front of it to behind it
        own_tri.append([at(0.6 + 0.3 * k, -1.0, 2.0), at(0.85 + 0.3 * k, -1.0, 2.0), at(0.6 + 0.3 * k, -1.0, -1.0 - 0.3 * k)])
    for k in range(4):   # touching: one vertex within a hair of the plane, in front of it or behind
        own_tri.append([at(-1.5 + 0.2 * k, -0.8, 1.0), at(-1.3 + 0.2 * k, -0.8, 1.0), at(-1.4 + 0.2 * k, -0.9, 1e-6 * (k - 1.5))])
    for k in range(20):  # a line of triangles wholly behind the camera
        a = np.array([-1.2 + 0.12 * k, 0.4 + 0.01 * k, -(2.0 + 0.15 * k)])
        own_tri.append([at(*a), at(*(a + (0.3, 0, 0))), at(*(a + (0, 0.3, 0.05)))])
    tri += own_tri
    return make_case("camera plane", cam, W, H, np.array(tri), np.array(sph), behind=(24, 20))


SLIVER_RATIOS = (0.9, 1.1, 1.5)


def _slivers():
    """needles whose height is 0.9, 1.1 and 1.5 x 2^-10 of their longest edge (24 of each, turned every
    way, some in the plane of the view, some across it), 8 exactly degenerate triangles (e2 = 2 e1, e2 = e1 / 2,
    e1 = 0: rho <= 0x1.4p-10 emax can hold for nothing else, see the module's docstring), and a patch"""
    W, H = 192, 64
    cam = _view("synthetic view", W, H)
    rng = np.random.default_rng(9)
    _, _, Hh, V = cam_vectors(cam)
    tri = []
    for k in range(72):
        ratio = SLIVER_RATIOS[k % 3] * 2.0 ** -10
        a = at_image(cam, rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.4), rng.uniform(5.0, 8.0))
        e = rng.normal(size=3)
        e *= rng.uniform(2.0, 5.0) / np.linalg.norm(e)
        n = np.cross(e, rng.normal(size=3))
        n /= np.linalg.norm(n)
        tri.append([a, a + e, a + rng.uniform(0.2, 0.8) * e + ratio * np.linalg.norm(e) * n])
    degenerate = []
    for k in range(8):
        a = at_image(cam, 0.1 + 0.1 * k, 0.3, 8.0).astype(F32).astype(F64)
        e = np.array([2.0, 0.5 * (k % 3), -1.0 * (k % 2)]) * (1 + k)   # (exact in fp32, and so are 2 e, e / 2)
        a = np.round(a * 4) / 4                                           # a + e, a + 2 e exact too
        degenerate.append([a, a + e, a + 2 * e] if k % 3 == 0 else [a, a + e, a + e / 2] if k % 3 == 1 else [a, a, a + e])
    tri = np.concatenate([np.array(tri), np.array(degenerate), patch_triangles(cam, 5, 3, (0.1, 0.9, 0.05, 0.35))])
    return make_case("slivers", cam, W, H, tri, None, degenerate=(72, 80))


ADVICE_VARIANTS = {"upright": ((1, 0, 0, 1), (0.0, 0.0), 0.0),
                   "quarter turn": ((0, -1, 1, 0), (0.0, 0.0), 0.0),
                   "half turn, moved along the edge": ((-1, 0, 0, -1), (0.0, -512.0), 0.0),
                   "mirrored": ((1, 0, 0, -1), (0.0, 256.0), 0.0),
                   "tilted": ((1, 0, 0, 1), (0.0, 0.0), 1e-7)}
# v0, v1, v2 in the plane: e2 = (0, 4096), e1 = (4096, 2560), so u = (x - x0) / 4096 and the reference's
# reject `u2 < EPS` (EPS = 2^-23) is x < x0 + 2^-11: with x0 = -2^-11 the accepted half of the plane begins
# at the axis, whichever way the triangle is turned
ADVICE_BASE = np.array([[-2.0 ** -11, -2048.0], [4096.0 - 2.0 ** -11, 512.0], [-2.0 ** -11, 2048.0]])


def _advice(variant):
    """ADVICE.md's hull item: one large triangle, 4,096 wide, in a plane parallel to the camera plane and 1.3 x
    the radius of the 2^-20 |.|_1 ball each of its 12 corners is taken with in front of it (0.016: 3.9e-6 of
    its width; at the 1.5e-6 the advisor guessed, the ball reaches the camera plane and the triangle is global).
    All 12 corners stay in front, the triangle is not global.  Through a 1.2 degree lens -- (H - 1) / (2 tan
    0.6 deg) = 3,000 px per unit of x / z -- its dilated corners, up to 8,100 to the side, project to 1.5e9 px:
    past the +-1e9 px the extents are clamped to, coordinate by coordinate.  The camera sits at the origin and
    looks along -z, so the plane z = -depth is exact in fp32.  The frame sees 1e-3 of the plane, all of it
    inside the triangle, next to the middle of the edge v0 -> v2; the reference rejects u2 < EPS, a strip 4.9e-4
    wide along that edge which ends at the axis, so the triangle is needed in one half of the frame.  Variants
    turn and mirror the triangle in its plane, move it along that edge, tilt it by 1e-7 rad about the edge.
    A small patch behind it fills the list."""
    W, H = 192, 64
    m, shift, tilt = ADVICE_VARIANTS[variant]
    cam = camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H, vfov=1.2)
    m = np.array(m, F64).reshape(2, 2)
    xy = (ADVICE_BASE + np.array(shift)) @ m.T
    e1, e2 = xy[1] - xy[0], xy[2] - xy[0]
    slack = 2.0 ** -20 * (np.abs(xy[0]).sum() + np.abs(e1).sum() + np.abs(e2).sum())
    depth = float(F32(1.3 * slack))
    z = np.array([-depth, -depth - tilt * 4096.0, -depth])
    big = np.concatenate([xy, z[:, None]], axis=1)
    patch = patch_triangles(cam, 8, 4, (0.55, 0.9, 0.55, 0.9), depth=(5.0, 6.0), wobble=0.1)
    return make_case(f"advice/{variant}", cam, W, H, np.concatenate([big[None], patch]), None, advice=0,
                     expect_cones=True)


BANDS = [("rows", 0, 24), ("rows", 24, 44), ("rows", 44, 60), ("rows", 60, 62)]  # H = 62: a last short band
STRIPS = [("strips", 8, 1, 3)]

CASES = {
    "spheres/synthetic view": lambda n: _ordinary(n, "synthetic view", "spheres"),
    "triangles/synthetic view": lambda n: _ordinary(n, "synthetic view", "triangles"),
    **{f"both/{v}": (lambda n, v=v: _ordinary(n, v, "both")) for v in VIEWS},
    "ragged 130x50": lambda n: _ordinary(n, "cornell view", "both", 130, 50),
    "ragged 33x9": lambda n: _ordinary(n, "synthetic view", "both", 33, 9, SMALL, ordinary=False),  # (6 tiles)
    "hidden behind triangles": lambda n: _hidden(n, "triangles"),
    "hidden behind a sphere": lambda n: _hidden(n, "sphere"),
    **{f"grazing {e:g}": (lambda n, e=e: _grazing(n, e)) for e in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6)},
    "in the planes of eight rows": lambda n: _in_planes(),
    "dilation levels": lambda n: _dilation(),
    "camera plane": lambda n: _camera_plane(),
    "slivers": lambda n: _slivers(),
    **{f"advice/{v}": (lambda n, v=v: _advice(v)) for v in ADVICE_VARIANTS},
    "bands": lambda n: _ordinary(n, "synthetic view", "both", 192, 62, LEFT, BANDS, layers=2),
    "strips": lambda n: _ordinary(n, "synthetic view", "both", 192, 64, LEFT, STRIPS, layers=2),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name](name)
    c["name"] = name
    return c
