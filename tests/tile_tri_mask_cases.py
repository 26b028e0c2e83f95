"""Scenes, cameras and the reference's answer for the per-tile triangle MASKS of a directly swept triangle
table (csrc/rt_lists.h "Per-tile triangle masks", k_bin_tri_masks).  Plain module: no pytest and no GPU.  It
extends tests/tile_list_cases.py -- the rays, the pieces, `analyse` and its `needed`, the restated geometry
of rt_lists.h are that module's -- with scenes of 1 to 33 triangles, too few for groups and lists.
tests/test_tile_tri_mask_cases_cpu.py shows on the reference alone that every case does what it was built
for; tests/test_tile_tri_masks.py reads the masks of a rendered frame back and holds them to `needed`.

A case is the dict of tile_list_cases plus
  "eye", "look"   the camera as the oracle takes it (vfov 60, vup +y): the frames are compared with it
  "masks"         per piece: does the frame get masks at all (33 triangles, a band off the 4-row grid: no)
  "global"        {triangle: reason} -- the triangles the case declares as possibly global, reason one of
                  "crossing" (its 12 corners, at the dilation rt_lists.h documents for this camera, are not
                  all on one side of the camera plane), "in plane" (the camera within H of its plane:
                  tri_escape possible), "no bound" (tri_escape has no H to offer: possible, unbounded) and
                  "degenerate" (no normal: a sliver by the binning threshold)
  "zero"          triangles with three equal vertices: never accepted, never binned
The triangles are the case's own, then the light's triangle as the last index.
"""
import functools
import types

import numpy as np

import esctp1raytracer_amd as esc
import oracle_lib as ol
import tile_list_cases as tc

F32 = np.float32
F64 = np.float64
EYE, LOOK = (0.0, 3.0, 6.0), (0.0, 2.0, -8.0)


def camera(W, H, eye=EYE, look=LOOK):
    return types.SimpleNamespace(c=esc.Camera.for_image(eye, look, W, H).c)


def light_at(cam, s, t, depth, size=0.08):
    """the light's triangle around image position (s, t), facing the camera roughly; size in image widths"""
    p = tc.at_image(cam, np.array([s, s + size, s]), np.array([t, t, t + 2.5 * size]), np.full(3, depth))
    return {"vertex": p.astype(F32), "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_A}


def scene(tris, light, spheres=None):
    geoms = []
    if tris is not None and len(tris):
        t = np.asarray(tris, F64).reshape(-1, 3)
        geoms.append({"vertex": t.astype(F32), "face_index": np.arange(len(t)).reshape(-1, 3),
                      "material": ol.material13(ka=(0.6, 0.6, 0.65), kd=(0.6, 0.6, 0.65))})
    geoms.append(light)
    sp = None if spheres is None or not len(spheres) else np.asarray(spheres, F64).astype(F32)
    mats = None if sp is None else np.stack([ol.material13(ka=(0.4, 0.5, 0.8), kd=(0.4 + 0.05 * k, 0.5, 0.8))
                                             for k in range(len(sp))])
    return ol.scene_dict(geoms, sp, mats)


def make_case(name, W, H, tris, light, spheres=None, pieces=None, masks=None, glob=None, zero=(), eye=EYE,
              look=LOOK, **declared):
    cam = camera(W, H, eye, look)
    light = light(cam) if callable(light) else light
    tris = tris(cam) if callable(tris) else tris
    spheres = spheres(cam) if callable(spheres) else spheres
    pieces = pieces or [("rows", 0, H)]
    c = {"name": name, "cam": cam, "eye": eye, "look": look, "W": W, "H": H, "scene": scene(tris, light, spheres),
         "pieces": pieces, "masks": masks if masks is not None else [True] * len(pieces),
         "global": dict(glob or {}), "zero": tuple(zero)}
    c.update(declared)
    c["n_tri"] = len(tc.triangles_of(c["scene"]))
    assert (W <= 160 and H <= 40) or c.get("large"), name
    return c


def few_spheres(cam, n=5, seed=4):
    return tc.cloud_spheres(cam, n, (0.1, 0.9, 0.1, 0.5), seed=seed, depth=(5.0, 9.0), size=(0.02, 0.04))


def floor_pair(x=20.0, z0=-2.0, z1=-60.0, y=0.0):
    """two triangles of a floor in the plane y = const, all of it well in front of the camera plane (the
    camera at z = 6 looks along -z): the lower part of the frame, the horizon across it, sky above"""
    a, b, c, e = (-x, y, z0), (x, y, z0), (x, y, z1), (-x, y, z1)
    return np.array([[a, b, c], [a, c, e]], F64)


def _c3_layout(name, W=160, H=36, pieces=None, masks=None, n_sph=5, **declared):
    """the floor pair, the light's triangle in view above the horizon, n_sph spheres over the floor (80: enough
    for sphere groups, tile lists and light lists -- the frame kernel's forms without a fallback sweep)"""
    return make_case(name, W, H, floor_pair(), lambda cam: light_at(cam, 0.62, 0.78, 6.0),
                     lambda cam: few_spheres(cam, n_sph), pieces, masks, c3=True, **declared)


def _counted(name, n_tri, W=128, H=24):
    """n_tri triangles in all: n_tri - 1 small ones scattered over the frame and the light's"""
    masks = [n_tri <= 32]
    return make_case(name, W, H, (lambda cam: tc.scatter_triangles(cam, n_tri - 1, (0.05, 0.95, 0.05, 0.95), seed=n_tri,
                                                                   depth=(6.0, 12.0), size=0.06)) if n_tri > 1 else None,
                     lambda cam: light_at(cam, 0.3, 0.4, 5.0, size=0.12), lambda cam: few_spheres(cam, 3), None, masks)


def _camera_plane(name):
    """the floor pair; [2] wholly behind the camera, its mirror image crossing the frame; [3] a strip of floor
    that runs from in front of the camera to behind it (cut by the camera plane: global)"""
    def tris(cam):
        o, A, Hh, V = tc.cam_vectors(cam)
        right, up = Hh / np.linalg.norm(Hh), V / np.linalg.norm(V)
        fwd = np.cross(right, up)
        fwd *= np.sign(fwd @ A)
        at = lambda x, y, z: o + x * right + y * up + z * fwd
        behind = [at(-0.4, 0.2, -3.0), at(0.4, 0.2, -3.0), at(0.0, 0.8, -3.2)]
        cut = [at(0.6, -1.0, 3.0), at(1.1, -1.0, 3.0), at(0.8, -1.0, -2.0)]
        return np.concatenate([floor_pair(), np.array([behind, cut])])
    return make_case(name, 128, 24, tris, lambda cam: light_at(cam, 0.2, 0.8, 6.0), few_spheres, glob={3: "crossing"},
                     behind=2)


def _in_plane(name):
    """[0] lies in the plane through the camera and pixel row 9: every ray of that row runs in its plane, as
    nearly as fp32 vertices allow (global through E.possible); [1], [2] the floor"""
    W, H = 128, 24

    def tris(cam):
        p = tc.at_image(cam, np.array([0.2, 0.8, 0.5]), np.full(3, 9.0 / (H - 1.0)), np.array([6.0, 7.0, 14.0]))
        return np.concatenate([p[None], floor_pair()])
    return make_case(name, W, H, tris, lambda cam: light_at(cam, 0.7, 0.8, 6.0), few_spheres, glob={0: "in plane"})


def _degenerate(name):
    """[0] e2 = 2 e1 exactly (a sliver by the binning threshold: global), [1] three equal vertices (zero: never
    binned), [2] a needle 1.5 x 2^-10 high (no sliver by the binning threshold; H of tri_escape_at grows like
    |e1| |e2| / |n1|, a thousandfold for it, and reaches the camera: global through E.possible), [3], [4] the floor"""
    def tris(cam):
        a = np.round(tc.at_image(cam, 0.3, 0.6, 8.0) * 4) / 4
        e = np.array([2.0, 0.5, -1.0])
        z = np.round(tc.at_image(cam, 0.6, 0.6, 8.0) * 4) / 4
        b = tc.at_image(cam, 0.2, 0.7, 6.0)
        d = tc.at_image(cam, 0.8, 0.75, 6.0) - b
        n = np.cross(d, (0.0, 0.0, 1.0))
        needle = [b, b + d, b + 0.4 * d + 1.5 * 2.0 ** -10 * np.linalg.norm(d) * n / np.linalg.norm(n)]
        return np.concatenate([np.array([[a, a + e, a + 2 * e], [z, z, z], needle]), floor_pair()])
    return make_case(name, 128, 24, tris, lambda cam: light_at(cam, 0.7, 0.8, 6.0), few_spheres, glob={0: "degenerate", 2: "in plane"},
                     zero=(1,))


def _cover_and_off(name):
    """[0] covers the whole frame from behind everything else, [1] lies wholly off screen (to the right),
    [2], [3] two small ones in the frame"""
    def tris(cam):
        big = tc.at_image(cam, np.array([-1.5, 3.5, 0.5]), np.array([-1.0, -1.0, 4.0]), np.full(3, 30.0))
        off = tc.at_image(cam, np.array([2.5, 3.0, 2.7]), np.array([0.2, 0.3, 0.7]), np.full(3, 8.0))
        return np.concatenate([big[None], off[None], tc.scatter_triangles(cam, 2, (0.2, 0.8, 0.2, 0.8), seed=5, size=0.08)])
    return make_case(name, 128, 24, tris, lambda cam: light_at(cam, 0.1, 0.1, 6.0), few_spheres, cover=0, off=1)


CASES = {
    "c3 layout": lambda n: _c3_layout(n),
    "c3 layout, 80 spheres": lambda n: _c3_layout(n, n_sph=80),
    **{f"{k} triangles": (lambda n, k=k: _counted(n, k)) for k in (1, 2, 7, 8, 32, 33)},
    "behind and across the camera plane": _camera_plane,
    "camera in a triangle's plane": _in_plane,
    "sliver and zero": _degenerate,
    "whole frame and off screen": _cover_and_off,
    "W 130": lambda n: _c3_layout(n, W=130, H=24),                  # 130 = 4 x 32 + 2
    "H 22": lambda n: _c3_layout(n, W=96, H=22),                    # no multiple of 4 or 8
    # a band that starts off the 4-row grid gets no masks; its neighbour on the grid does
    "bands": lambda n: _c3_layout(n, W=96, H=36, pieces=[("rows", 6, 22), ("rows", 8, 24), ("rows", 32, 36)],
                                  masks=[False, True, True]),
    "strips of 8": lambda n: _c3_layout(n, W=96, H=36, pieces=[("strips", 8, 1, 2), ("strips", 8, 0, 2)]),  # (the second
    # ends in the image's short last strip, rows 32 .. 35)
    "strips of 16": lambda n: _c3_layout(n, W=96, H=40, pieces=[("strips", 16, 0, 2), ("strips", 16, 1, 2)]),
}


# k_bin_tri_masks shares one triangle's tiles out over gridDim.y = clamp(tiles / 4096, 1, 64) workgroups
# (esc_launch_tile_lists); every case above has at most 45 tiles and runs it with one.  The one frame that is
# not small: 64 x 129 = 8,256 tiles, two workgroups per triangle, each wave striding over its share.
LARGE = "c3 layout, 2048x516"
LARGE_CASES = {LARGE: lambda n: _c3_layout(n, W=2048, H=516, large=True)}


def mask_workgroups(n_tiles):
    """gridDim.y of k_bin_tri_masks as esc_launch_tile_lists documents it"""
    return min(64, max(1, n_tiles // (256 * 16)))


@functools.lru_cache(maxsize=None)
def case(name):
    if name in LARGE_CASES:
        c = LARGE_CASES[name](name)
        c["name"] = "masks/" + name
        return c
    c = CASES[name](name)
    c["name"] = "masks/" + name  # (tile_list_cases.analyse caches by name)
    return c


def needed(c, k=0):
    """[tiles, n_tri] bool of piece k: tile_list_cases' `needed` for the triangles"""
    return tc.analyse(c, k)["needed"][1]


def global_reasons(c):
    """{triangle: reason} from the geometry rt_lists.h documents, nothing the kernels answer: "degenerate"
    (rho <= 0x1.4p-10 emax, no normal, e1 = 0 -- a zero triangle is left out: it is never binned), "in plane"
    (tri_escape: possible and bounded), "no bound" (possible, unbounded), "crossing" (the 12 corners at the camera's dilation level not all further than
    1.001 of their ball's radius on one side of the camera plane)"""
    o32 = np.array(c["cam"].c.origin, F32)
    out = {}
    for i, v in enumerate(tc.triangles_of(c["scene"])):
        e1, e2 = (v[1] - v[0]).astype(F32), (v[2] - v[0]).astype(F32)
        if not e1.any() and not e2.any():
            continue
        rho, emax, nn, l1 = tc.tri_shape(v[0], e1, e2)
        if not (rho > float.fromhex("0x1.4p-10") * emax) or not nn > 0 or not l1 > 0:
            out[i] = "degenerate"
            continue
        possible, bounded, _, _ = tc.tri_escape(v[0], e1, e2, o32, 1.0)
        if possible:
            out[i] = "in plane" if bounded else "no bound"
            continue
        kK, _ = tc.dilation_level(v, o32)
        pts, slack = tc.tri_corners(c, v[0], e1, e2, kK)
        dist = tc.plane_distance(c["cam"], pts)
        if not ((dist > 1.001 * slack).all() or (dist < -1.001 * slack).all()):
            out[i] = "crossing"
    return out


def corner_box(c, k, q):
    """the local tiles (flat bool) of piece k inside the tile box, grown by one ring, of triangle q's 12 corners
    at the LARGEST dilation (kK = 1) -- None when a corner does not lie in front of the camera plane (no box)"""
    v = tc.triangles_of(c["scene"])[q]
    pts, _ = tc.tri_corners(c, v[0], v[1] - v[0], v[2] - v[0], 1.0)
    w, h, depth = tc.pixel_of(c["cam"], c["W"], c["H"], pts)
    if not (depth > 0).all() or not (np.isfinite(w).all() and np.isfinite(h).all()):
        return None
    tiles_x, tile_rows = tc.tile_grid(c["pieces"][k], c["W"], c["H"])
    if w.max() < -2 or h.max() < -2 or w.min() > c["W"] + 1 or h.min() > c["H"] + 1:  # (two pixels off: the
        # kernel's own rectangle is one pixel and a rounding wider)
        return np.zeros(tiles_x * tile_rows, bool)
    cl = lambda x, hi: float(min(max(x, 0.0), hi))
    return tc.tiles_of_image_box(c["pieces"][k], c["W"], c["H"], np.floor(cl(w.min(), c["W"] - 1)),
                                 np.ceil(cl(w.max(), c["W"] - 1)), np.floor(cl(h.min(), c["H"] - 1)),
                                 np.ceil(cl(h.max(), c["H"] - 1)), ring=1)
