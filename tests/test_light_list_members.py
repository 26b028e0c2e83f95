"""GPU: the light lists of the shadow pass hold every pair record a shadow ray needs.

k_bin_light_pairs, k_bin_light_tri_pairs and k_bin_light_tri_escape (csrc/rt_lists.h "Light lists") decide which
pair records a shadow ray tests at all: those of its own cell of the light's cube map and of that face's short
list.  A frame comparison sees a missing record only where the dropped primitive is the ray's ONLY occluder (the
last light) or its first one in index order (an earlier light: quirk S3 moves the next light's origin); here the
lists of a rendered frame are read back (Renderer.light_lists) and held to tests/light_list_cases.py's `needed`:
every (ray, primitive) pair the reference's any-hit test accepts with the ray's own initial t, whether or not
another occluder would have ended the sweep first.  tests/test_light_list_cases_cpu.py shows on the reference
alone that the cases are not vacuous (one needed entry in six is reached only by rays with a second acceptor).

The cell of a ray is light_list_cell restated (lc.cell_of); a ray within 2^-12 cells of a cell border is held to
both cells, which the 1e-3 cells the binning kernels grow their extents by cover.  Only rays the lists serve are
counted: those whose origin passes shadow_wave_lists' fp32 box test (lc.in_box) and whose light has lists.  The
first light's rays all start on a surface and must all pass; later lights' origins follow quirk S3 and may
leave the box -- their number is printed.

The other direction is bounded for triangles, so that "everything everywhere" cannot pass (spheres:
test_light_list_pairs.py's Restated): a record off the face lists lies in the box of its triangles' 12 corners at
the largest dilation, projected on the face and grown by one ring of cells.

The four overflow cases of light_list_cases.CASES stay with the frame tests: a cell or a face list over its cap
sends the wave to the group sweep, so membership says nothing about those rays.
"""
import numpy as np
import pytest

import light_list_cases as lc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PAD_SLOT = (2 ** 31 - 1) // 2  # what sg_orig / tg_orig hold for a pad slot
KINDS = {2: "sph", 3: "tri"}    # esc_tile_list_counts' numbering of the light lists -> the keys of lc.needed


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


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the scene's own tables: which record holds which original primitive ---------------------------------------
def record_map(sc, d, which):
    """-> (rec_of [n_prims]: the pair record of every original primitive of the kind, n_rec: the records up to
    the last one with a real half, their numbers).  Pair
    record j holds the sorted slots 2 j and 2 j + 1; sg_orig / tg_orig give a slot's original primitive.  That
    the record's own numbers ARE that primitive's is asserted for every real half, bit for bit."""
    if which == 2:
        orig = sc.table("sg_orig").view(np.int32)
        rec = sc.table("sg_sorted2").view(np.float32).reshape(-1, 4, 2)
        prims = d["spheres"]
        assert len(orig) == 2 * len(rec)
        for s, q in enumerate(orig):
            j, h = s >> 1, s & 1
            if q == PAD_SLOT:
                assert rec[j, 3, h] == -np.inf, f"pad slot {s} holds a sphere"
                continue
            want = np.append(prims[q, :3], F32(prims[q, 3] * prims[q, 3]))
            assert same_bits(rec[j, :, h], want), f"sphere slot {s} is not original sphere {q}"
    else:
        orig = sc.table("tg_orig").view(np.int32)
        rec = sc.table("tg_sorted").view(np.float32).reshape(-1, 12)
        prims = lc.triangles_of(d)
        assert len(orig) == len(rec) and len(rec) % 2 == 0
        for s, q in enumerate(orig):
            if q == PAD_SLOT:
                assert not rec[s, 3:9].any(), f"pad slot {s} holds a triangle"
                continue
            v = prims[q]
            want = np.concatenate([v[0], (v[1] - v[0]).astype(F32), (v[2] - v[0]).astype(F32)])
            assert same_bits(rec[s, :9], want), f"triangle slot {s} is not original triangle {q}"
    real = orig[orig != PAD_SLOT]
    assert np.array_equal(np.sort(real), np.arange(len(prims))), "every original primitive has exactly one slot"
    rec_of = np.zeros(len(prims), int)
    rec_of[real] = np.flatnonzero(orig != PAD_SLOT) >> 1
    n_rec = int(rec_of.max()) + 1  # (the tables are padded to whole sweep steps: records of two pad slots follow)
    return rec_of, n_rec, rec[:n_rec] if which == 2 else rec[:2 * n_rec]


# ---- the lists as sets --------------------------------------------------------------------------------------------
def as_sets(ll, n_rec, what):
    """Renderer.light_lists -> (present [n_listed, 6 R R, n_rec] bool, on_face [n_listed, 6, n_rec] bool), with
    the bounds on the read-back itself: every stored id a record index, none twice in a cell or a face list,
    as many stored as the counts say"""
    n, R, cap, gcap = ll["n_listed"], ll["R"], ll["cap"], ll["global_cap"]
    ids = ll["ids"].reshape(n, 6 * R * R, cap)
    cnt = ll["counts"].reshape(n, 6 * R * R)
    stored = ids >= 0
    assert np.array_equal(stored.sum(axis=2), np.minimum(cnt, cap)), f"{what}: stored ids against the counts"
    assert not (np.diff(stored.astype(np.int8), axis=2) > 0).any(), f"{what}: a stored id after an empty slot"
    assert int(ids.max()) < n_rec and int(ids.min()) >= -1, f"{what}: a stored id is no pair record with a real half ({int(ids.max())})"
    present = np.zeros((n, 6 * R * R, n_rec), bool)
    li, cell, k = np.nonzero(stored)
    present[li, cell, ids[li, cell, k]] = True
    assert int(present.sum()) == int(stored.sum()), f"{what}: a record is stored twice in a cell"
    fids, fcnt = ll["face_ids"], ll["face_counts"]
    fst = fids >= 0
    assert np.array_equal(fst.sum(axis=2), np.minimum(fcnt, gcap)), f"{what}: face lists against their counts"
    assert int(fids.max(initial=-1)) < n_rec, f"{what}: a face-list id is no pair record"
    on_face = np.zeros((n, 6, n_rec), bool)
    li, f, k = np.nonzero(fst)
    on_face[li, f, fids[li, f, k]] = True
    assert int(on_face.sum()) == int(fst.sum()), f"{what}: face-list ids are not distinct"
    return present, on_face


def first_missing(rays, counted, nd, rec_of, present, on_face, P, R):
    """completeness of one kind for one view -> None, or the description of the first needed record that is
    neither among the stored ids of one of the ray's cells nor on that (light, face)'s list.
    counted: the rays to hold the lists to; nd [n_rays, n_prims]; n_acc [n_rays]: acceptors of both kinds"""
    for li in range(present.shape[0]):
        sel = np.flatnonzero(counted & (rays["light"] == li))
        if not len(sel):
            continue
        face, cells, u, w = lc.cell_of(P[li], rays["hitp"][sel], R)
        r, q = np.nonzero(nd[sel])
        j = rec_of[q]
        listed = on_face[li, face[r], j]
        for k in range(cells.shape[1]):  # the ray's cell, and its neighbours where it lies on a border
            bad = ~listed & ~present[li, cells[r, k], j]
            if bad.any():
                b = int(np.flatnonzero(bad)[0])
                ray = int(sel[r[b]])
                cell = int(cells[r[b], k])
                return {"ray": ray, "light": li, "face": int(face[r[b]]), "cu": cell % R, "cw": (cell // R) % R,
                        "u": float(u[r[b]]), "w": float(w[r[b]]), "prim": int(q[b]), "record": int(j[b]),
                        "n_missing": int(bad.sum())}
    return None


def assert_complete(what, size, rays, counted, nd_all, which, rec_of, present, on_face, P, R):
    kind = KINDS[which]
    miss = first_missing(rays, counted, nd_all[kind], rec_of, present, on_face, P, R)
    if miss is None:
        return
    ray = miss["ray"]
    pixel = int(rays["pixel"][ray])
    others = int(nd_all["tri"][ray].sum() + nd_all["sph"][ray].sum()) - 1
    seen = "no other primitive accepts the ray: a frame could have seen it" if others == 0 else \
        f"{others} other primitives accept the ray: no frame comparison can see it"
    raise AssertionError(
        f"{what}: {miss['n_missing']} needed (ray, cell, record) entries of kind {kind} are in no list; first: pixel "
        f"(w={pixel % size}, h={pixel // size}), light {miss['light']}, face {lc.FACE_NAMES[miss['face']]}, cell "
        f"(cu={miss['cu']}, cw={miss['cw']}) for coordinates ({miss['u']:.6f}, {miss['w']:.6f}), original "
        f"{'sphere' if kind == 'sph' else 'triangle'} {miss['prim']} in pair record {miss['record']}; {seen}")


# ---- tightness of the triangle lists ------------------------------------------------------------------------------
def tri_boxes(rec, hdr, P, R):
    """per sorted triangle slot and face: the cell box (u0, u1, w0, w1), grown by one ring, of the 12 corners
    v_i +- rp e_a +- rp e_b at the largest dilation k = 1 (rt_lists.h: rp = rho (1 + 1e-5) + slack), projected on
    the face in float64 -- or None where not all 12 lie at least rp in front of the face's plane through P (the
    kernel may then project through P or send the record to the face list); "pad" for a pad slot"""
    hdr = hdr.astype(F64)
    g, rho_max, lo, hi = hdr[0:3], hdr[3], hdr[4:7], hdr[7:10]
    P = P.astype(F64)
    delta = 2.0 ** -20 * (rho_max + np.abs(P - g).sum())
    out = []
    for s in range(len(rec)):
        v0, e1, e2 = (rec[s, 3 * i:3 * i + 3].astype(F64) for i in range(3))
        if not e1.any() and not e2.any():
            out.append("pad")
            continue
        s3 = (e1 + e2) / 3.0
        rho = np.sqrt(max(s3 @ s3, (e1 - s3) @ (e1 - s3), (e2 - s3) @ (e2 - s3)))
        at = np.maximum(np.abs(v0 - lo), np.abs(v0 - hi)).sum()
        slack = 2.0 ** -20 * (at + np.abs(e1).sum() + np.abs(e2).sum()) + delta + 2.0 ** -60
        rp = rho * (1.0 + 1e-5) + slack
        n1 = np.cross(e2, e1)
        l1, nn = np.sqrt(e1 @ e1), np.sqrt(n1 @ n1)
        if not (l1 > 0 and nn > 0):
            out.append([None] * 6)
            continue
        ea = e1 / l1
        eb = np.cross(n1, ea) / nn
        pts = np.array([v + sa * rp * ea + sb * rp * eb - P for v in (v0, v0 + e1, v0 + e2)
                        for sa in (-1, 1) for sb in (-1, 1)])
        boxes = []
        for face in range(6):
            m, ia, ib, sign = lc.face_axes(face)
            depth = sign * pts[:, m]
            if not (depth >= rp).all():
                boxes.append(None)
                continue
            u, w = (pts[:, ia] / depth + 1.0) * (R / 2.0), (pts[:, ib] / depth + 1.0) * (R / 2.0)
            boxes.append((int(np.floor(u.min())) - 1, int(np.floor(u.max())) + 1,
                          int(np.floor(w.min())) - 1, int(np.floor(w.max())) + 1))
        out.append(boxes)
    return out


def check_tri_tightness(what, rec, hdr, P, present, on_face, R):
    """-> held [n_slots] bool: the triangle was held to its box on some face"""
    n_rec = len(rec) >> 1
    held = np.zeros(len(rec), bool)
    n_checked = 0
    for li in range(present.shape[0]):
        boxes = tri_boxes(rec, hdr, P[li], R)
        cells = present[li].reshape(6, R, R, n_rec)
        for j in range(n_rec):
            halves = [boxes[2 * j + h] for h in range(2) if boxes[2 * j + h] != "pad"]
            for face in range(6):
                if on_face[li, face, j]:
                    continue
                bx = [b[face] for b in halves]
                if not bx or any(b is None for b in bx):
                    continue
                if len(bx) == 2 and bx[0][0] <= bx[1][1] + 1 and bx[1][0] <= bx[0][1] + 1 and \
                        bx[0][2] <= bx[1][3] + 1 and bx[1][2] <= bx[0][3] + 1:
                    # the kernel appends two rectangles that touch as one: their bounding rectangle
                    bx = [(min(bx[0][0], bx[1][0]), max(bx[0][1], bx[1][1]), min(bx[0][2], bx[1][2]), max(bx[0][3], bx[1][3]))]
                allowed = np.zeros((R, R), bool)
                for u0, u1, w0, w1 in bx:
                    allowed[max(w0, 0):max(w1 + 1, 0), max(u0, 0):max(u1 + 1, 0)] = True
                outside = cells[face, :, :, j] & ~allowed
                assert not outside.any(), (f"{what}: light {li}, face {lc.FACE_NAMES[face]}: pair record {j} is in cells "
                                           f"(cw, cu) {np.argwhere(outside)[:4].tolist()} outside its corners' box {bx}")
                n_checked += 1
                for h in range(2):
                    if boxes[2 * j + h] != "pad":
                        held[2 * j + h] = True
    print(f"{what}: {int(held.sum())} triangles held to their corners' box, {n_checked} (light, face, record) checks")
    return held


# ---- one scene -------------------------------------------------------------------------------------------------------
def check_scene(esc, renderer, what, d, views, want, key, fixed_face=0, upload=True, lattice_tris=None):
    """upload, render every view at 96 x 96 with default flags, read the lists (per scene and sample point) and hold
    them to `needed`.  want: {"sph": bool, "tri": bool} the kinds that must have lists.  lattice_tris: original
    indices of triangles that must all be held to their box and be on no face list (non-vacuity)"""
    sc = ol.scene_to_product(d)
    if upload:
        renderer.upload(sc)
    hdr = sc.table("header").view(np.float32)
    points = lc.light_points(d)
    size = lc.W
    lists, maps = {}, {}
    for vi, view in enumerate(views):
        vw = f"{what}/view {vi}"
        cam = esc.Camera.for_image(view[0], view[1], size, size)
        # the rays `needed` was computed for are the rays the frame traces
        rays, nd = lc.members((key, vi, fixed_face), d, view, fixed_face)
        o_gpu, d_gpu = renderer.camera_rays(cam, size, size)
        renderer.synchronize()
        assert same_bits(d_gpu.cpu().numpy(), rays["dirs"]) and \
            same_bits(o_gpu.cpu().numpy(), np.broadcast_to(rays["origin"], rays["dirs"].shape)), f"{vw}: primary rays"
        ref, ref_cnt = ol.oracle_render(d, view[0], view[1], size, size, threads=8, fixed_face=fixed_face,
                                        return_counters=True)
        renderer.reset_counters()
        gpu = renderer.render(cam, size, size, fixed_face=fixed_face)
        got_cnt = renderer.counters()
        nb = int((bits(gpu) != bits(ref)).sum())
        assert nb == 0, f"{vw}: {nb} fp32 values differ from the oracle's frame"
        assert got_cnt["shadow_rays"] == ref_cnt["shadow_rays"] == len(rays["tb"]), \
            f"{vw}: shadow rays: frame {got_cnt['shadow_rays']}, oracle {ref_cnt['shadow_rays']}, restated {len(rays['tb'])}"
        if vi == 0:  # the lists are per scene and sample point: read once
            for which, kind in KINDS.items():
                st, ll = renderer.tile_lists(which), renderer.light_lists(which)
                assert (st is not None) == (ll is not None) == want[kind], f"{what}: light lists of kind {kind}"
                if ll is None:
                    continue
                # preconditions, hard
                assert st["off"] == 0, f"{what}: kind {kind}: the lists switched themselves off"
                assert int(ll["counts"].max()) <= ll["cap"], f"{what}: kind {kind}: a cell holds {int(ll['counts'].max())}"
                assert int(ll["face_counts"].max()) <= ll["global_cap"], \
                    f"{what}: kind {kind}: a face list holds {int(ll['face_counts'].max())}"
                assert np.array_equal(ll["counts"].reshape(-1), st["counts"].reshape(-1)) and \
                    st["global"] == int(ll["face_counts"].max()), f"{what}: the two read-backs disagree"
                n_all = len(d["light_sources"])
                assert ll["R"] == 128 and ll["n_listed"] == min(n_all, 4), (what, ll["R"], ll["n_listed"])
                P = points[ll["point"]]
                for li in range(ll["n_listed"]):  # the sample point the lists were built for is the rays' P
                    assert same_bits(P[li], rays["P"][li]), f"{what}: light {li}: lists for {P[li]}, rays towards {rays['P'][li]}"
                rec_of, n_rec, rec = record_map(sc, d, which)
                maps[which] = (rec_of, rec, P, st["cones"])
                lists[which] = as_sets(ll, n_rec, f"{what}: kind {kind}")
                print(f"{what}: kind {kind}: {int(ll['counts'].sum())} stored in cells, longest face list "
                      f"{int(ll['face_counts'].max())}, {st['cones']} cone entries")
        # which rays count
        inside = lc.in_box(hdr, rays["hitp"])
        first = rays["light"] == 0
        assert inside[first].all(), f"{vw}: {int((~inside[first]).sum())} rays of the first light start outside the scene box"
        n_listed = min(len(d["light_sources"]), 4)
        counted = inside & (rays["light"] < n_listed)
        print(f"{vw}: {len(inside)} shadow rays, {int(counted.sum())} counted, {int((~inside).sum())} start outside the box, "
              f"{int((rays['light'] >= n_listed).sum())} towards a light without lists")
        for which in lists:
            rec_of, rec, P, _ = maps[which]
            present, on_face = lists[which]
            assert_complete(vw, size, rays, counted, nd, which, rec_of, present, on_face, P, 128)
    for which, kind in KINDS.items():  # the lists are still the ones that were read
        if which in lists:
            st = renderer.tile_lists(which)
            assert np.array_equal(st["counts"].reshape(-1), lists[which][0].sum(axis=2).reshape(-1)), f"{what}: lists changed"
    held = None
    if 3 in lists:
        rec_of, rec, P, cones = maps[3]
        present, on_face = lists[3]
        if cones == 0:
            held = check_tri_tightness(what, rec, hdr, P, present, on_face, 128)
        else:
            print(f"{what}: {cones} cone entries put records anywhere: triangle tightness not checked")
        if lattice_tris is not None:
            assert cones == 0, f"{what}: an ordinary case with cone entries skips triangle tightness"
            # The light's own triangle has P for a vertex and is listed for every direction by rule; the k-d
            # order gives it a lattice triangle for a partner, whose record is therefore on every face list.
            # That one apart, every lattice triangle is held to its box and its record is on no face list.
            orig = sc.table("tg_orig").view(np.int32)[:len(rec)]
            lat = np.isin(orig, lattice_tris)
            other = (orig != PAD_SLOT) & ~lat
            shared = lat & other.reshape(-1, 2)[:, ::-1].reshape(-1)  # lattice slots whose partner is no lattice triangle
            assert int(lat.sum()) == len(lattice_tris) and int(shared.sum()) <= 1, (what, np.flatnonzero(shared).tolist())
            assert all(orig[s ^ 1] == 12 for s in np.flatnonzero(shared)), f"{what}: a lattice triangle shares a record with a wall"
            slots = np.flatnonzero(lat & ~shared)
            assert held[slots].all(), f"{what}: lattice triangles never held to a box: slots {slots[~held[slots]].tolist()}"
            assert not on_face[:, :, np.unique(slots >> 1)].any(), f"{what}: a lattice triangle's record is on a face list"
    return lists, maps


def n_fixed_tris(c):
    """triangles before the lattice's in the original order: walls, lights, the case's own (lc.build)"""
    return 12 + len(c["lights"]) * (1 if c["light_faces"] == 1 else 2) + len(c["extra_tris"])


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room(esc, renderer, variant):
    c = lc.room(variant)
    n_tri, n_sph = lc.ROOMS[variant]
    d = lc.build(c)
    lattice = np.arange(n_fixed_tris(c), n_fixed_tris(c) + n_tri) if variant == "triangles" else None
    check_scene(esc, renderer, variant, d, c["views"], {"sph": n_sph > 0, "tri": n_tri > 0}, ("room", variant),
                lattice_tris=lattice)


MEMBER_CASES = [n for n in lc.CASES if lc.EXPECT[n]["over"] is None]


@pytest.mark.parametrize("name", MEMBER_CASES)
def test_geometry_class(esc, renderer, name):
    c = lc.case(name)
    check_scene(esc, renderer, name, lc.build(c), c["views"], lc.EXPECT[name], ("case", name))


def test_fixed_face_lists_are_rebuilt(esc, renderer):
    """faces 0, 1, 0 of a two-face light: the lists are rebuilt for the other sample point and back, and the
    membership follows"""
    c = lc.fixed_face_case()
    d = lc.build(c)
    seen = []
    for n, face in enumerate((0, 1, 0)):
        lists, maps = check_scene(esc, renderer, f"fixed face {face}", d, c["views"], {"sph": True, "tri": True},
                                  "fixed face", fixed_face=face, upload=n == 0)
        seen.append((lists[3][0], maps[3][2]))
    assert np.array_equal(seen[0][0], seen[2][0]) and not np.array_equal(seen[0][0], seen[1][0])
    assert same_bits(seen[0][1], seen[2][1]) and not same_bits(seen[0][1], seen[1][1])


@pytest.mark.parametrize("scene", ["far apart", "overlapping"])
def test_slab_partners(esc, renderer, scene):
    d = lc.far_apart_scene() if scene == "far apart" else lc.overlapping_scene()
    check_scene(esc, renderer, scene, d, lc.SLAB_VIEWS, {"sph": True, "tri": False}, ("slab", scene))


@pytest.mark.parametrize("lights", lc.CORNER_ORDERS, ids=[" then ".join(q) for q in lc.CORNER_ORDERS])
def test_corner_light(esc, renderer, lights):
    c, _ = lc.corner_case(lights)
    check_scene(esc, renderer, f"corner {lights}", lc.build(c), c["views"], {"sph": True, "tri": False}, ("corner", lights))
