"""GPU: the light lists bin each sphere of a pair record on its own (csrc/rt_lists.h k_bin_light_pairs).

A pair record holds any two of the 8 spheres of a k-d leaf.  It is appended to the cells of half 0's
rectangle on a cube face and to those cells of half 1's rectangle that half 0's does not hold -- not to the
bounding rectangle of both -- and the rectangles' radius comes from the cone of origins that can meet the
sphere (never more than the box reach R0).  What decides whether a half has a rectangle at all (`around`,
in front of the face's plane, cut by it) stays on R0.

The rule is restated here on the CPU in double from the scene's own host tables (the group-sorted pair
table, the grown scene box): per light, face and half the tangent extents of the sphere of radius R0 seen
from P, grown by ONE cell on every side (the kernel grows by 1e-3 cells), and the records that go on a
face's short list.  The device lists must stay inside that restatement; that they hold every record a ray
needs is what the frames show: every case renders bit-equal three ways -- lists on, group sweep, CPU oracle.
"""
import math

import numpy as np
import pytest

import light_list_cases as lc
import oracle_lib as ol
from light_list_cases import SLAB_VIEWS, corner_case, far_apart_scene, overlapping_scene

pytestmark = pytest.mark.gpu

R = 128          # cells per face side (rt_device.h LightLists)
SLAB_SIZE = (224, 128)


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
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bit_equal(gpu, ref, what):
    nb = int((bits(gpu) != bits(ref)).sum())
    assert nb == 0, f"{what}: {nb} of {ref.size} fp32 values differ, max abs {float(np.abs(gpu - ref).max())}"


# ---- the rule, restated ---------------------------------------------------------------------------------
def face_axes(face):
    m = face >> 1
    return m, (1 if m == 0 else 0), (1 if m == 2 else 2), (-1.0 if face & 1 else 1.0)


class Restated:
    """per light li, face f, record j, half h: rect[li][f][j][h] = (u0, u1, w0, w1) cells (grown by one,
    clipped to the face) or None; on_face_list[li][f][j]: some half sends the record to the face's short list;
    margin: how far the nearest decision (around / in front / corner rule) is from its threshold"""

    def __init__(self, d):
        sc = ol.scene_to_product(d)
        self.rec = sc.table("sg_sorted2").view(np.float32).reshape(-1, 4, 2).astype(np.float64)
        hdr = sc.table("header").view(np.float32).astype(np.float64)
        g, rho, lo, hi = hdr[0:3], hdr[3], hdr[4:7], hdr[7:10]
        self.lo, self.hi = lo, hi
        self.points = lc.light_points(d).astype(np.float64)
        n_rec = len(self.rec)
        self.rect, self.on_face_list, self.margin = [], [], math.inf
        self.r0 = np.zeros((len(self.points), n_rec, 2))
        self.dist = np.zeros((len(self.points), n_rec, 2))
        for li, P in enumerate(self.points):
            delta = 2.0 ** -20 * (rho + np.abs(P - g).sum())
            rect = [[[None, None] for _ in range(n_rec)] for _ in range(6)]
            glob = np.zeros((6, n_rec), bool)
            for j in range(n_rec):
                for h in range(2):
                    r2 = self.rec[j, 3, h]
                    if not r2 >= 0.0:
                        continue  # a pad half
                    C = self.rec[j, 0:3, h]
                    far = math.sqrt((np.maximum(np.abs(C - lo), np.abs(C - hi)) ** 2).sum())
                    R0 = (math.sqrt(r2) + float.fromhex("0x1.6p-10") * far) * (1.0 + 2.0 ** -20) + delta + 2.0 ** -60
                    c = C - P
                    cn = math.sqrt((c * c).sum())
                    self.r0[li, j, h], self.dist[li, j, h] = R0, cn
                    t_around = R0 * 1.001 + 1e-4 * rho
                    self.margin = min(self.margin, abs(cn - t_around))
                    if not cn > t_around:
                        glob[:, j] = True
                        continue
                    for f in range(6):
                        m, ia, ib, sign = face_axes(f)
                        depth = sign * c[m]
                        self.margin = min(self.margin, abs(depth - R0))
                        if depth > R0 * (1.0 + 1e-9):
                            e = []
                            for a in (ia, ib):
                                th = math.atan2(c[a], depth)
                                al = math.asin(min(1.0, R0 / math.hypot(c[a], depth)))
                                e += [int(math.floor((math.tan(th - al) + 1.0) * R / 2)) - 1,
                                      int(math.floor((math.tan(th + al) + 1.0) * R / 2)) + 1]
                            u0, u1, w0, w1 = max(0, e[0]), min(R - 1, e[1]), max(0, e[2]), min(R - 1, e[3])
                            if u0 <= u1 and w0 <= w1:
                                rect[f][j][h] = (u0, u1, w0, w1)
                        else:
                            ang = math.acos(max(-1.0, min(1.0, depth / cn)))
                            lim = 0.95532 + math.asin(min(1.0, R0 / cn)) + 1e-6
                            self.margin = min(self.margin, abs(ang - lim))
                            if not ang > lim:
                                glob[f, j] = True
            self.rect.append(rect)
            self.on_face_list.append(glob)

    def real(self, j, h):
        return self.rec[j, 3, h] >= 0.0

    def cell_rects(self, li, f, j):
        """the rectangles the record may be appended to on that face: none when it is on the short list"""
        if self.on_face_list[li][f][j]:
            return []
        return [q for q in self.rect[li][f][j] if q is not None]

    def mask(self, skip=None):
        """(lights * 6, R, R) bool: cells inside some half's rectangle (of records other than `skip`)"""
        m = np.zeros((len(self.points) * 6, R, R), bool)
        for li in range(len(self.points)):
            for f in range(6):
                for j in range(len(self.rec)):
                    if j == skip:
                        continue
                    for u0, u1, w0, w1 in self.cell_rects(li, f, j):
                        m[li * 6 + f, w0:w1 + 1, u0:u1 + 1] = True
        return m

    def cells(self):
        """the number of (cell, half) pairs of all rectangles"""
        return sum((u1 - u0 + 1) * (w1 - w0 + 1) for li in range(len(self.points)) for f in range(6)
                   for j in range(len(self.rec)) for u0, u1, w0, w1 in self.cell_rects(li, f, j))


def three_ways(esc, renderer, d, views, size, what):
    """lists == group sweep == oracle, bit for bit, per view -> the sphere light lists' statistics"""
    renderer.upload(ol.scene_to_product(d))
    off = esc.ESC_RENDER_NO_TILE_LISTS | esc.ESC_RENDER_NO_LIGHT_LISTS
    w, h = size
    st = None
    for i, (eye, look) in enumerate(views):
        cam = esc.Camera.for_image(eye, look, w, h)
        ref = ol.oracle_render(d, eye, look, w, h, threads=8)
        gpu = renderer.render(cam, w, h)
        if st is None:
            st = renderer.tile_lists(2)
        assert_bit_equal(gpu, ref, f"{what}/view {i}/lists")
        assert_bit_equal(renderer.render(cam, w, h, flags=off), ref, f"{what}/view {i}/sweep")
    return st


def check_inside_restatement(st, x, what):
    """the device lists against the restated rule -> counts as (lights * 6, R, R)"""
    assert st is not None and st["off"] == 0, f"{what}: no light lists of sphere pair records"
    assert x.margin > 1e-7, f"{what}: a decision of the rule is too close to call ({x.margin})"
    cnt = st["counts"].reshape(len(x.points) * 6, R, R)
    outside = cnt[~x.mask()]
    assert int(outside.max(initial=0)) == 0, f"{what}: {int((outside > 0).sum())} cells outside every sphere's rectangle hold records"
    assert int(cnt.sum()) <= x.cells(), f"{what}: {int(cnt.sum())} appended, the spheres' own rectangles hold {x.cells()}"
    want = max(int(g[f].sum()) for g in x.on_face_list for f in range(6))
    assert st["global"] == want, f"{what}: longest face list {st['global']}, restated {want}"
    return cnt


def shadowed_pixels(d, view, size):
    on = ol.oracle_render(d, view[0], view[1], size[0], size[1], threads=8)
    off = ol.oracle_render(d, view[0], view[1], size[0], size[1], threads=8, shadows=False)
    return int((on.view(np.uint32) != off.view(np.uint32)).any(axis=2).sum())


def test_far_apart_partners(esc, renderer):
    """partners tens of cells apart: the record is in each sphere's own rectangle and nowhere between"""
    d = far_apart_scene()
    x = Restated(d)
    assert len(x.points) == 1
    # the fixture (CPU only): what the bounding rectangle of a record's halves would add
    mask = x.mask()
    between = np.zeros_like(mask)
    bounding = 0
    for f in range(6):
        for j in range(len(x.rec)):
            q = x.cell_rects(0, f, j)
            if len(q) == 2:
                u0, u1 = min(q[0][0], q[1][0]), max(q[0][1], q[1][1])
                w0, w1 = min(q[0][2], q[1][2]), max(q[0][3], q[1][3])
                bounding += (u1 - u0 + 1) * (w1 - w0 + 1)
                between[f, w0:w1 + 1, u0:u1 + 1] = True
    between &= ~mask
    assert int(between.sum()) > 0, "no cell lies between two partners and outside every rectangle"
    assert bounding > 5 * x.cells(), (bounding, x.cells())  # partners ARE far apart here
    assert sum(shadowed_pixels(d, v, SLAB_SIZE) for v in SLAB_VIEWS) > 0
    st = three_ways(esc, renderer, d, SLAB_VIEWS, SLAB_SIZE, "far-apart partners")
    cnt = check_inside_restatement(st, x, "far-apart partners")
    assert int(cnt[between].max()) == 0, "a cell between two partners' rectangles holds a record"
    assert int(cnt.max()) >= 1


def test_overlapping_partners(esc, renderer):
    """two spheres of one record in the same cells: those cells hold the record once"""
    d = overlapping_scene()
    x = Restated(d)
    twins = [j for j in range(len(x.rec)) if x.real(j, 0) and x.real(j, 1)
             and np.abs(x.rec[j, 0:3, 0] - x.rec[j, 0:3, 1]).max() < 0.02]
    assert len(twins) >= 32, f"only {len(twins)} records hold one cluster"
    assert sum(shadowed_pixels(d, v, SLAB_SIZE) for v in SLAB_VIEWS) > 0
    st = three_ways(esc, renderer, d, SLAB_VIEWS, SLAB_SIZE, "overlapping partners")
    cnt = check_inside_restatement(st, x, "overlapping partners")
    checked = 0
    for j in twins:
        others = x.mask(skip=j)
        for f in range(6):
            if x.on_face_list[0][f][j]:
                continue
            # the cell of each centre's direction is inside both halves' kernel rectangles
            for h in range(2):
                c = x.rec[j, 0:3, h] - x.points[0]
                m, ia, ib, sign = face_axes(f)
                if not (sign * c[m] > 0 and max(abs(c[ia]), abs(c[ib])) < sign * c[m]):
                    continue
                cu = int(math.floor((c[ia] / abs(c[m]) + 1.0) * R / 2))
                cw = int(math.floor((c[ib] / abs(c[m]) + 1.0) * R / 2))
                if not others[f, cw, cu]:
                    assert int(cnt[f, cw, cu]) == 1, f"record {j}: cell ({cu}, {cw}) of face {f} holds {int(cnt[f, cw, cu])}"
                    checked += 1
    assert checked >= 32


# ---- the room of light_list_cases: P surrounded, every face in use ---------------------------------------------
def room_three_ways(esc, renderer, c, what):
    d = lc.build(c)
    return d, three_ways(esc, renderer, d, c["views"], (lc.W, lc.H), what)


def test_partners_on_different_faces_and_a_cut_half(esc, renderer):
    """the lattice around P plus spheres the planes through P cut: records whose halves are seen through
    different faces, and records with one half on a face's short list while the other has a rectangle there"""
    c = lc.case("spheres cut by face planes")
    x = Restated(lc.build(c))
    split = cut = 0
    cut_cells = []
    for j in range(len(x.rec)):
        faces = [{f for f in range(6) if x.rect[0][f][j][h] is not None and not x.on_face_list[0][f][j]} for h in range(2)]
        if faces[0] and faces[1] and not (faces[0] & faces[1]):
            split += 1
        for f in range(6):
            if x.on_face_list[0][f][j] and not x.on_face_list[0].all(axis=0)[j]:
                for q in x.rect[0][f][j]:
                    if q is not None:  # the other half is in front of this face: no rectangle for it here
                        cut += 1
                        cut_cells.append((f, q, j))
    assert split >= 1, "no record with its halves on different faces"
    assert cut >= 1, "no record with one half cut by a face's plane and the other in front of it"
    d, st = room_three_ways(esc, renderer, c, "cut halves")
    cnt = check_inside_restatement(st, x, "cut halves")  # (the mask leaves out a short-listed record's rectangles)
    for f, (u0, u1, w0, w1), j in cut_cells:
        free = ~x.mask(skip=j)[f, w0:w1 + 1, u0:u1 + 1]
        assert int(cnt[f, w0:w1 + 1, u0:u1 + 1][free].max(initial=0)) == 0, f"record {j} is on face {f}'s list AND in its cells"
    per_face = cnt.reshape(6, -1)
    assert (per_face.max(axis=1) > 0).all()


def test_pad_half(esc, renderer):
    """95 spheres: the last record of the sorted table is half empty"""
    c = lc.make_case(n_sph=95)
    x = Restated(lc.build(c))
    assert sum(1 for j in range(len(x.rec)) if x.real(j, 0) != x.real(j, 1)) >= 1, "no half-empty record"
    d, st = room_three_ways(esc, renderer, c, "pad half")
    cnt = check_inside_restatement(st, x, "pad half")
    assert (cnt.reshape(6, -1).max(axis=1) > 0).all()


@pytest.mark.parametrize("lights", [("corner",), ("centre", "corner"), ("corner", "centre")],
                         ids=["corner", "centre then corner", "corner then centre"])
def test_cone_reach(esc, renderer, lights):
    """the rectangles' reach from the cone of origins: a light in a corner of the box and one near its middle,
    a sphere with R0 > |c - P| / 2 (the reach falls back to the box's), a cone that leaves the box through
    an edge; with two lights the second one's rays can start outside the box (quirk S3) and take the sweep"""
    c, corner = corner_case(lights)
    d = lc.build(c)
    x = Restated(d)
    assert len(x.points) == len(lights)
    li = lights.index("corner")
    assert np.abs(x.points[li] - corner).max() < 1e-6
    assert (x.points[li] > x.lo).all() and (x.points[li] < x.hi).all()
    assert 5.0 - np.abs(corner).max() < 0.7 and 5.0 - np.abs(c["p"]).max() > 4.0  # in a corner / near the middle
    near = [(j, h) for j in range(len(x.rec)) for h in range(2) if x.real(j, h)
            and abs(math.sqrt(x.rec[j, 3, h]) - 0.035) < 1e-6]
    assert len(near) == 1
    j, h = near[0]
    assert x.r0[li, j, h] > 0.5 * x.dist[li, j, h] * 1.05 and not x.on_face_list[li].all(axis=0)[j]
    st = three_ways(esc, renderer, d, c["views"], (lc.W, lc.H), f"cone reach {lights}")
    cnt = check_inside_restatement(st, x, f"cone reach {lights}")
    assert (cnt.reshape(len(lights), 6, -1).max(axis=2) > 0).any(axis=1).all()
