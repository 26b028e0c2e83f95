"""The binning rule of the sphere light lists restated per HALF (csrc/rt_lists.h light_half_reach /
light_half_rect), for the tests of the packed cells (k_pack_light_cells): a cell keeps the halves of its stored
records whose OWN rectangle holds it.

In double from the scene's host tables (sg_sorted2, header, light_points), with the rectangles' radius from the
cone of origins (lc.sphere_reaches' Rx) and the kernel's 1e-3 cells of growth.  The tangent directions are
computed by angles where the kernel solves the conic: the same numbers up to rounding, which moves a rectangle's
edge only where an extent lies within ~1e-12 of a cell border -- this restatement serves statistics and
fixtures; the device lists are held to the rays themselves (test_light_list_packed.py).
"""
import math

import numpy as np

import light_list_cases as lc
import oracle_lib as ol

R = 128  # cells per face side (rt_device.h kLightListRes)
NONE, RECT, GLOBAL = 0, 1, 2


class HalfRects:
    """kind[li, f, j, h] in (NONE, RECT, GLOBAL); rect[li, f, j, h] = (u0, u1, w0, w1), clipped to the face"""

    def __init__(self, d):
        sc = ol.scene_to_product(d)
        self.rec = sc.table("sg_sorted2").view(np.float32).reshape(-1, 4, 2).astype(np.float64)
        hdr = sc.table("header").view(np.float32)
        rho = float(hdr[3])
        self.points = lc.light_points(d).astype(np.float64)
        n_rec = len(self.rec)
        self.kind = np.zeros((len(self.points), 6, n_rec, 2), np.int8)
        self.rect = np.zeros((len(self.points), 6, n_rec, 2, 4), np.int32)
        for li, P in enumerate(self.points):
            for j in range(n_rec):
                for h in range(2):
                    r2 = self.rec[j, 3, h]
                    if not r2 >= 0.0:
                        continue  # a pad half
                    C = self.rec[j, 0:3, h]
                    R0, Rx = lc.sphere_reaches(hdr, P, C, r2)
                    c = C - P
                    cn = math.sqrt(float(c @ c))
                    if not cn > R0 * 1.001 + 1e-4 * rho:  # P (all but) inside the reach: every face's own list
                        self.kind[li, :, j, h] = GLOBAL
                        continue
                    for f in range(6):
                        m, ia, ib, sign = lc.face_axes(f)
                        depth = sign * c[m]
                        if depth > R0 * (1.0 + 1e-9):  # wholly in front of the face's plane through P
                            e = []
                            for a in (ia, ib):
                                th = math.atan2(c[a], depth)
                                al = math.asin(min(1.0, Rx / math.hypot(c[a], depth)))
                                e += [int(math.floor((math.tan(th - al) + 1.0) * R / 2 - 1e-3)),
                                      int(math.floor((math.tan(th + al) + 1.0) * R / 2 + 1e-3))]
                            u0, u1, w0, w1 = max(0, e[0]), min(R - 1, e[1]), max(0, e[2]), min(R - 1, e[3])
                            if u0 <= u1 and w0 <= w1:
                                self.kind[li, f, j, h] = RECT
                                self.rect[li, f, j, h] = (u0, u1, w0, w1)
                        else:  # cut by (or behind) the plane
                            ang = math.acos(max(-1.0, min(1.0, depth / cn)))
                            if not ang > 0.95532 + math.asin(min(1.0, R0 / cn)) + 1e-6:
                                self.kind[li, f, j, h] = GLOBAL

    def figures(self):
        """over all lights, faces and records off the faces' own lists -> (entries, kept, both): the stored
        (cell, record) entries (the union of the two halves' rectangles), the halves whose own rectangle holds
        the entry's cell (the sum of the two areas), and the entries that keep both halves (the intersection)"""
        entries = kept = both = 0
        n_l, _, n_rec, _ = self.kind.shape
        for li in range(n_l):
            for f in range(6):
                for j in range(n_rec):
                    k = self.kind[li, f, j]
                    if (k == GLOBAL).any():
                        continue
                    q = [self.rect[li, f, j, h] for h in range(2) if k[h] == RECT]
                    area = [int((u1 - u0 + 1) * (w1 - w0 + 1)) for u0, u1, w0, w1 in q]
                    inter = 0
                    if len(q) == 2:
                        du = min(q[0][1], q[1][1]) - max(q[0][0], q[1][0]) + 1
                        dw = min(q[0][3], q[1][3]) - max(q[0][2], q[1][2]) + 1
                        inter = int(max(du, 0) * max(dw, 0))
                    kept += sum(area)
                    both += inter
                    entries += sum(area) - inter
        return entries, kept, both


def shadowed_pixels(d, view, size, **kw):
    """pixels of the reference's frame that some occluder changes"""
    on = ol.oracle_render(d, view[0], view[1], size[0], size[1], threads=8, **kw)
    off = ol.oracle_render(d, view[0], view[1], size[0], size[1], threads=8, shadows=False, **kw)
    return int((on.view(np.uint32) != off.view(np.uint32)).any(axis=2).sum())


def packed_cases():
    """the scenes of test_light_list_packed.py: name -> (scene dict, views, (w, h), fixed faces, members key,
    overflow: None / "cell" / "global")"""
    out = {}
    slab = (lc.W, lc.H)  # (light_list_cases restates the shadow rays of square frames of this size)
    out["far apart"] = (lc.far_apart_scene(), lc.SLAB_VIEWS, slab, (0,), ("slab", "far apart"), None)
    out["overlapping"] = (lc.overlapping_scene(), lc.SLAB_VIEWS, slab, (0,), ("slab", "overlapping"), None)
    for lights in lc.CORNER_ORDERS:
        c, _ = lc.corner_case(lights)
        out["corner: " + " then ".join(lights)] = (lc.build(c), c["views"], (lc.W, lc.H), (0,), ("corner", lights), None)
    c = lc.make_case(n_sph=95)
    out["pad half"] = (lc.build(c), c["views"], (lc.W, lc.H), (0,), ("packed", "pad half"), None)
    for name in ("cell overflow, spheres", "global overflow, spheres", "P inside a sphere's reach", "P inside a sphere",
                 "spheres cut by face planes", "two lights", "five lights"):
        c = lc.case(name)
        out[name] = (lc.build(c), c["views"], (lc.W, lc.H), (0,), ("case", name), lc.EXPECT[name]["over"])
    c = lc.fixed_face_case()
    out["fixed faces 0, 1"] = (lc.build(c), c["views"], (lc.W, lc.H), (0, 1), "fixed face", None)
    c = lc.room("spheres")
    out["room: spheres"] = (lc.build(c), c["views"], (lc.W, lc.H), (0,), ("room", "spheres"), None)
    return out
