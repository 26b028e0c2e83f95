"""CPU: the cases of tests/tile_list_cases.py do what they were built for, shown on the reference alone
(ray_oracle.tri_test / sph_test on the reference's fp32 primary rays) before any GPU reads a list.  A case
that is vacuous -- nothing needed, everything needed, nothing hidden, no corner beyond the clamp -- would
let tests/test_tile_list_members.py pass whatever the binning kernels do.
"""
import numpy as np
import pytest

import tile_list_cases as tc

F64 = np.float64
ALL = list(tc.CASES)


def pieces(c):
    return range(len(c["pieces"]))


@pytest.mark.parametrize("name", ALL)
def test_case_is_not_vacuous(name):
    """every piece and kind: at least 20 % of the tiles need something, at least 20 % need nothing; an ordinary
    case has at least 200 needed (tile, primitive) pairs of each kind and declares no possible global; every
    kind under test has 64 to 250 primitives"""
    c = tc.case(name)
    may = tc.may_go_global(c)
    for w in c["kinds"]:
        assert 64 <= len(may[w]) <= 250
        assert int(may[w].sum()) <= tc.GLOBAL_CAP, (name, w, int(may[w].sum()))
        pairs = 0
        for k in pieces(c):
            nd = tc.analyse(c, k)["needed"][w]
            tx, tr = tc.tile_grid(c["pieces"][k], c["W"], c["H"])
            assert nd.shape == (tx * tr, len(may[w]))
            some = nd.any(axis=1)
            assert some.mean() >= 0.2 and (~some).mean() >= 0.2, (name, w, k, float(some.mean()))
            pairs += int(nd.sum())
        if c["ordinary"]:
            assert pairs >= 200, (name, w, pairs)
            assert not may[w].any(), (name, w, np.flatnonzero(may[w]).tolist())


def test_the_cases_cover_the_listed_classes():
    names = set(ALL)
    for v in tc.VIEWS:
        assert f"both/{v}" in names
    assert {"spheres/synthetic view", "triangles/synthetic view", "ragged 130x50", "ragged 33x9", "bands", "strips",
            "hidden behind triangles", "hidden behind a sphere", "dilation levels", "camera plane", "slivers"} <= names
    assert tc.case("ragged 130x50")["W"] % 32 == 2 and tc.case("ragged 130x50")["H"] % 4 == 2
    assert tc.case("spheres/synthetic view")["kinds"] == [0] and tc.case("triangles/synthetic view")["kinds"] == [1]
    assert tc.case("both/cornell view")["kinds"] == [0, 1]


def test_partitions():
    """the pieces' rows: bands on multiples of 4 with a last short one that end where the image does; the
    strips 1, 4, 7 of 8 rows"""
    b = tc.case("bands")
    assert [p[1] % 4 for p in b["pieces"]] == [0] * len(b["pieces"])
    rows = np.concatenate([tc.local_rows(p, b["H"]) for p in b["pieces"]])
    assert np.array_equal(rows, np.arange(b["H"])) and len(tc.local_rows(b["pieces"][-1], b["H"])) < 4
    s = tc.case("strips")
    assert s["pieces"] == [("strips", 8, 1, 3)]
    assert tc.local_rows(s["pieces"][0], s["H"]).tolist() == list(range(8, 16)) + list(range(32, 40)) + list(range(56, 64))
    assert tc.tile_grid(s["pieces"][0], s["W"], s["H"]) == (6, 6)
    # a strip image whose last strip is short, and one piece of tiles_of_image_box: image tile rows 8 .. 9 of
    # the strips above are local tile rows 2 .. 3, and the ring adds nothing the call did not render
    assert tc.local_rows(("strips", 8, 1, 2), 29).tolist() == list(range(8, 16)) + list(range(24, 29))
    m = tc.tiles_of_image_box(s["pieces"][0], s["W"], s["H"], 40, 70, 33, 38, ring=0).reshape(6, 6)
    assert m[2:4, 1:3].all() and m.sum() == 4
    m = tc.tiles_of_image_box(s["pieces"][0], s["W"], s["H"], 40, 70, 33, 38, ring=1).reshape(6, 6)
    assert m[2:4, 0:4].all() and m.sum() == 8


@pytest.mark.parametrize("name", ["hidden behind triangles", "hidden behind a sphere"])
def test_hidden_primitives_are_needed_and_never_seen(name):
    c = tc.case(name)
    a = tc.analyse(c)
    kind, prim = a["closest"]
    n_sph, n_tri = c["hidden"]
    assert not ((kind == 0) & (prim < n_sph)).any(), "a small sphere shows"
    assert not ((kind == 1) & (prim < n_tri)).any(), "a small triangle shows"
    assert a["needed"][0][:, :n_sph].any(axis=0).all(), "a small sphere is needed nowhere"
    assert a["needed"][1][:, :n_tri].any(axis=0).all(), "a small triangle is needed nowhere"
    assert (kind >= 0).mean() > 0.4 and (kind < 0).mean() > 0.2  # the wall, and the open rows above it


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("grazing")])
def test_grazing_accepts_outside_the_exact_projection(name):
    """the camera 1e-1 ... 1e-5 above the floor's plane: in every case some pixel's ray is accepted by a floor
    triangle that its line, taken exactly, does not meet -- statement (E_t) of rt_lists.h, not only (S_t); from
    1e-3 of elevation down floor triangles leave cone entries by tri_escape_at's formula, at 1e-2 none does"""
    c = tc.case(name)
    a = tc.analyse(c)
    assert a["needed"][1][:, :c["n_floor"]].sum() >= 8  # (one pixel row lies along the floor)
    outside = 0
    for q in range(c["n_floor"]):
        ok = a["ok"][1][q]
        if ok.any():
            outside += int((ok & ~tc.exact_inside(c, 0, q)).sum())
    o = np.array(c["cam"].c.origin, np.float32)
    cones = sum(tc.dilation_level(v, o)[1] for v in tc.triangles_of(c["scene"])[:c["n_floor"]])
    assert outside >= 1, name
    assert (cones >= 1) == c["expect_cones"], (name, cones)
    print(f"{name}: {outside} needed pixels outside the exact projection, {cones} floor triangles with a cone")


def test_accepts_that_only_the_cone_entries_serve():
    """the camera in the planes of eight tessellated floors: every triangle leaves a cone entry, and some
    (tile, triangle) pair is needed outside the tile box of the triangle's 12 corners at the largest dilation"""
    c = tc.case("in the planes of eight rows")
    o = np.array(c["cam"].c.origin, np.float32)
    tris = tc.triangles_of(c["scene"])[:-1]
    assert all(tc.dilation_level(v, o) == (1.0, True) for v in tris)
    eo = tc.escape_only_pairs(c)
    assert eo.sum() >= 1
    print(f"{int(eo.sum())} of {int(tc.analyse(c)['needed'][1].sum())} needed pairs lie outside (S_t)'s box: "
          f"{np.argwhere(eo).tolist()}")


def test_dilation_family_brackets_the_four_levels():
    """nearest plane first: cone entries (kK = 1), then 1 / 2, 1 / 4, 1 / 8, each at least once and in that
    order; seen from a camera 100 further up every one of them takes 1 / 8"""
    c = tc.case("dilation levels")
    o = np.array(c["cam"].c.origin, np.float32)
    fam = tc.triangles_of(c["scene"])[:c["family"]]
    e = [(v[1] - v[0], v[2] - v[0]) for v in fam]
    assert all(np.array_equal(x[0], e[0][0]) and np.array_equal(x[1], e[0][1]) for x in e), "not translates"
    lv = [tc.dilation_level(v, o) for v in fam]
    kk = [l[0] for l in lv]
    assert sorted(kk, reverse=True) == kk, kk
    assert set(kk) == {1.0, 0.5, 0.25, 0.125}, kk
    assert lv[0] == (1.0, True) and sum(l[1] for l in lv) >= 4 and all(l[0] == 1.0 for l in lv if l[1])
    assert all(tc.dilation_level(v, o + np.float32([0, 100, 0])) == (0.125, False) for v in fam)
    print("kK of the family, nearest plane first:", kk)


def test_camera_plane_classes():
    c = tc.case("camera plane")
    may = tc.may_go_global(c)
    a = tc.analyse(c)
    n_sph, n_tri = len(c["scene"]["spheres"]), len(tc.triangles_of(c["scene"])) - 1  # (the light is last)
    b_sph, b_tri = c["behind"]
    # wholly behind the camera, needed nowhere -- yet the lines through them cross the image
    sp = c["scene"]["spheres"][n_sph - b_sph:]
    assert (tc.plane_distance(c["cam"], sp[:, :3].astype(F64)) + sp[:, 3] < 0).all()
    assert not a["needed"][0][:, n_sph - b_sph:].any()
    w, h, depth = tc.pixel_of(c["cam"], c["W"], c["H"], sp[:, :3].astype(F64))
    assert ((w >= 0) & (w < c["W"]) & (h >= 0) & (h < c["H"])).sum() >= 8 and (depth < 0).all()
    tr = tc.triangles_of(c["scene"])[n_tri - b_tri:n_tri]
    assert (tc.plane_distance(c["cam"], tr.reshape(-1, 3).astype(F64)) < 0).all()
    assert not a["needed"][1][:, n_tri - b_tri:n_tri].any()
    w, h, depth = tc.pixel_of(c["cam"], c["W"], c["H"], tr[:, 0].astype(F64))
    assert ((w >= 0) & (w < c["W"]) & (h >= 0) & (h < c["H"])).sum() >= 8
    # cut and touching: declared, and only those (8 own spheres before the line, 10 own triangles)
    own_s = np.arange(n_sph - b_sph - 8, n_sph - b_sph)
    assert may[0][own_s[:6]].all() and not may[0][own_s[6:]].any() and may[0].sum() == 6
    own_t = np.arange(n_tri - b_tri - 10, n_tri - b_tri)
    assert may[1][own_t].all() and may[1].sum() == 10
    # some of them are needed in front of the camera, where only a list can serve them
    assert a["needed"][0][:, own_s[:6]].any() and a["needed"][1][:, own_t].any()


def test_sliver_classes():
    """needles of the three height ratios, none of them a sliver by the binning threshold; the exactly
    degenerate triangles are, and are the only declared globals"""
    c = tc.case("slivers")
    may = tc.may_go_global(c)
    tris = tc.triangles_of(c["scene"]).astype(F64)
    lo, hi = c["degenerate"]
    thr = float.fromhex("0x1.4p-10")
    for q in range(lo):
        v = tris[q]
        rho, emax, nn, l1 = tc.tri_shape(v[0], v[1] - v[0], v[2] - v[0])
        longest = max(emax, np.linalg.norm(v[2] - v[1]))
        ratio = nn / longest / longest * 2.0 ** 10  # height over the longest edge, in units of 2^-10
        assert abs(ratio / tc.SLIVER_RATIOS[q % 3] - 1) < 0.02, (q, ratio)
        assert rho >= 0.5 * emax > thr * emax
    for q in range(lo, hi):
        v = tris[q]
        rho, emax, nn, l1 = tc.tri_shape(v[0], v[1] - v[0], v[2] - v[0])
        assert nn == 0.0 or l1 == 0.0, q
    assert np.flatnonzero(may[1]).tolist() == list(range(lo, hi))
    assert tc.analyse(c)["needed"][1][:, :lo].any(axis=0).sum() >= 20  # needles that some ray accepts


@pytest.mark.parametrize("variant", list(tc.ADVICE_VARIANTS))
def test_advice_corners_project_beyond_the_clamp(variant):
    """float64: some of the 12 corners of the large triangle, at the dilation the kernel documents for this
    camera, project beyond 1e9 px in magnitude; all 12 lie in front of the camera plane, further from it than
    their ball's radius (not global); the triangle is needed in part of the frame"""
    c = tc.case(f"advice/{variant}")
    v = tc.triangles_of(c["scene"])[0]
    o = np.array(c["cam"].c.origin, np.float32)
    kK, cone = tc.dilation_level(v, o)
    assert (kK, cone) == (1.0, True)
    pts, slack = tc.tri_corners(c, v[0], v[1] - v[0], v[2] - v[0], kK)
    w, h, _ = tc.pixel_of(c["cam"], c["W"], c["H"], pts)
    big = np.maximum(np.abs(w), np.abs(h))
    assert (big > 1e9).sum() >= 2, big.max()
    dist = tc.plane_distance(c["cam"], pts)
    assert (dist > 1.2 * slack).all(), (dist.min(), slack)
    assert not tc.may_go_global(c)[1].any()
    nd = tc.analyse(c)["needed"][1][:, 0]
    assert 0.2 <= nd.mean() <= 0.8, nd.mean()
    print(f"advice/{variant}: corners reach {big.max():.3g} px, {int((big > 1e9).sum())} of 12 beyond 1e9; "
          f"needed in {int(nd.sum())} of {nd.size} tiles")
