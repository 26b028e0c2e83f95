"""CPU: the cases of tests/tile_tri_mask_cases.py do what they were built for, shown on the reference alone
(ray_oracle.tri_test on the reference's fp32 primary rays) before any GPU builds a mask.  A case in which
every tile needs every triangle, or none does, would let tests/test_tile_tri_masks.py pass whatever
k_bin_tri_masks answers.
"""
import numpy as np
import pytest

import tile_list_cases as tc
import tile_tri_mask_cases as mc

ALL = list(mc.CASES)


@pytest.mark.parametrize("name", ALL)
def test_case_has_needed_and_unneeded_pairs(name):
    """every piece of every case: some (tile, triangle) pair is needed, some is not; a few dozen tiles"""
    c = mc.case(name)
    assert len(c["pieces"]) == len(c["masks"])
    for k, piece in enumerate(c["pieces"]):
        nd = mc.needed(c, k)
        tx, tr = tc.tile_grid(piece, c["W"], c["H"])
        assert nd.shape == (tx * tr, c["n_tri"]) and 3 <= tx * tr <= 60, (name, k, nd.shape)
        assert nd.any() and (~nd).any(), (name, k)
        print(f"{name}/piece {k}: {int(nd.sum())} of {nd.size} (tile, triangle) pairs needed")


@pytest.mark.parametrize("name", ALL)
def test_declared_globals_are_exactly_the_geometric_ones(name):
    """the triangles a case declares as possibly global are exactly those with a corner on both sides of the
    camera plane, a camera within H of their plane (or no H to be had), or no normal at all -- each for the
    reason it declares"""
    c = mc.case(name)
    assert mc.global_reasons(c) == c["global"], (name, mc.global_reasons(c))
    tris = tc.triangles_of(c["scene"])
    for q in c["zero"]:
        assert not (tris[q] - tris[q][0]).any() and not mc.needed(c)[:, q].any()


def test_the_cases_cover_the_listed_classes():
    n_tri = {name: mc.case(name)["n_tri"] for name in ALL}
    assert [n_tri[f"{k} triangles"] for k in (1, 2, 7, 8, 32, 33)] == [1, 2, 7, 8, 32, 33]
    assert mc.case("33 triangles")["masks"] == [False] and mc.case("32 triangles")["masks"] == [True]
    assert n_tri["c3 layout"] == 3 and len(mc.case("c3 layout")["scene"]["spheres"]) == 5
    assert set(mc.case("behind and across the camera plane")["global"].values()) == {"crossing"}
    assert set(mc.case("camera in a triangle's plane")["global"].values()) == {"in plane"}
    assert set(mc.case("sliver and zero")["global"].values()) == {"degenerate", "in plane"} and mc.case("sliver and zero")["zero"]
    assert mc.case("W 130")["W"] % 32 == 2
    assert mc.case("H 22")["H"] % 4 == 2
    b = mc.case("bands")
    assert [p[1] % 4 == 0 for p in b["pieces"]] == b["masks"] == [False, True, True]
    assert len(tc.local_rows(b["pieces"][2], b["H"])) == 4
    assert [p[1] for p in mc.case("strips of 8")["pieces"]] == [8, 8]
    assert [p[1] for p in mc.case("strips of 16")["pieces"]] == [16, 16]
    s = mc.case("strips of 8")
    assert tc.local_rows(s["pieces"][1], s["H"]).tolist() == list(range(0, 8)) + list(range(16, 24)) + list(range(32, 36))


def test_c3_layout_leaves_room():
    """the floor pair and the light: the reference alone needs the light's triangle in fewer than half of the
    tiles, the sky's tiles need no triangle at all, and nearly every tile needs at most one"""
    c = mc.case("c3 layout")
    nd = mc.needed(c)
    assert c.get("c3") and not c["global"]
    assert nd[:, 2].any() and nd[:, 2].mean() < 0.5
    per_tile = nd.sum(axis=1)
    assert (per_tile == 0).mean() >= 0.2 and (per_tile <= 1).mean() >= 0.6, per_tile.tolist()
    assert nd[:, 0].any() and nd[:, 1].any()
    print(f"c3 layout: needed triangles per tile {np.bincount(per_tile).tolist()} (0, 1, 2, ...)")


def test_camera_plane_classes():
    c = mc.case("behind and across the camera plane")
    tris = tc.triangles_of(c["scene"])
    q = c["behind"]
    assert (tc.plane_distance(c["cam"], tris[q].astype(np.float64)) < 0).all() and not mc.needed(c)[:, q].any()
    w, h, depth = tc.pixel_of(c["cam"], c["W"], c["H"], tris[q].astype(np.float64))
    assert (depth < 0).all() and ((w >= 0) & (w < c["W"]) & (h >= 0) & (h < c["H"])).any(), "its mirror image misses the frame"
    d = tc.plane_distance(c["cam"], tris[3].astype(np.float64))
    assert d.min() < 0 < d.max() and mc.needed(c)[:, 3].any()


def test_in_plane_triangle_is_within_H():
    c = mc.case("camera in a triangle's plane")
    v = tc.triangles_of(c["scene"])[0]
    possible, bounded, Hh, h = tc.tri_escape(v[0], v[1] - v[0], v[2] - v[0], np.array(c["cam"].c.origin, np.float32), 1.0)
    assert possible and bounded and h <= Hh * 1.01 + 1e-6, (Hh, h)


def test_whole_frame_and_off_screen():
    c = mc.case("whole frame and off screen")
    nd = mc.needed(c)
    assert nd[:, c["cover"]].all() and not nd[:, c["off"]].any()
    assert not mc.corner_box(c, 0, c["off"]).any()


def test_large_case_takes_several_workgroups_per_triangle():
    """the one large frame: enough tiles that k_bin_tri_masks shares a triangle's tiles out over two workgroups,
    with needed and unneeded pairs for every triangle"""
    c = mc.case(mc.LARGE)
    tx, tr = tc.tile_grid(c["pieces"][0], c["W"], c["H"])
    assert mc.mask_workgroups(tx * tr) == 2 and mc.mask_workgroups(45) == 1
    nd = mc.needed(c)
    assert nd.shape == (tx * tr, 3) and nd.any(axis=0).all() and (~nd).any(axis=0).all()
    assert not c["global"] and mc.global_reasons(c) == {}
