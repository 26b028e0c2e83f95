"""The fixtures of tests/light_list_cases.py do what they were built for -- shown on the reference alone
(oracle frames and ray_oracle's closest hits), before anything of them runs on a GPU.  With these in
place a pair record missing from any cell of the light lists that a shadow ray uses changes a pixel of
tests/test_light_list_directions.py.  Run with -s to see the figures.
"""
import numpy as np
import pytest

import light_list_cases as lc


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_light_point_comes_from_the_table(variant):
    c = lc.room(variant)
    d = lc.build(c)
    P = lc.light_points(d)
    assert P.shape == (1, 3) and np.array_equal(P[0], c["p"].astype(np.float32))
    n_tri, n_sph = lc.ROOMS[variant]
    assert len(c["tris"]) == n_tri and len(c["spheres"]) == n_sph
    assert all(n == 0 or n >= 64 for n in (n_tri, n_sph)), "a kind that is present must be grouped"
    # no two occluders overlap seen from P: angular radii against the angle between their directions
    ctr = np.concatenate([c["tris"].mean(axis=1), c["spheres"][:, :3]]) - c["p"]
    rad = np.concatenate([np.linalg.norm(c["tris"] - c["tris"].mean(axis=1, keepdims=True), axis=2).max(axis=1),
                          c["spheres"][:, 3]])
    dist = np.linalg.norm(ctr, axis=1)
    assert dist.min() >= 0.99 and dist.max() <= 3.01
    ang = np.arcsin(rad / dist)
    cosines = (ctr / dist[:, None]) @ (ctr / dist[:, None]).T
    between = np.arccos(np.clip(cosines, -1, 1)) + 10.0 * np.eye(len(ctr))
    assert (between > ang[:, None] + ang[None, :]).all()
    assert ang.max() < 0.1, "an occluder subtends a few cells of 2 / 128"


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_shadow_rays_start_on_every_face(variant):
    """hit - P by dominant axis and sign, over the six views: every face of the cube map gets origins"""
    c = lc.room(variant)
    d = lc.build(c)
    shares, per_view = lc.face_shares(d, c["views"], lc.light_points(d)[0].astype(float))
    print(f"\n{variant}: share of shadow-ray origins per face", dict(zip(lc.FACE_NAMES, np.round(shares, 3))))
    assert shares.min() > 0.10, shares
    assert all((f > 0).sum() >= 3 for f in per_view), "a view sees at least three faces' worth of walls"


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_views_have_lit_and_shadowed_pixels(variant):
    c = lc.room(variant)
    d = lc.build(c)
    for i, v in enumerate(c["views"]):
        hit, sh = lc.lit_and_shadowed(d, v)
        n_hit, n_sh = int(hit.sum()), int((hit & sh).sum())
        print(f"\n{variant} view {i}: {n_hit} hit pixels, {n_sh / n_hit:.3f} shadowed")
        assert n_sh > 100 and n_hit - n_sh > 100
        assert not (sh & ~hit).any()


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_every_occluder_casts_a_shadow_of_its_own(variant):
    """leaving occluder k out changes pixels that do not show k, in some view: k is their sole occluder"""
    sole = lc.sole_shadows(lc.room(variant))
    counts = np.array(list(sole.values()))
    print(f"\n{variant}: pixels only occluder k shadows: min {counts.min()}, median {np.median(counts)}")
    assert counts.min() >= 1, [k for k, n in sole.items() if n == 0]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case_has_lit_and_shadowed_pixels_where_its_primitives_matter(name):
    c = lc.case(name)
    d = lc.build(c)
    P = lc.light_points(d)
    assert len(P) == len(c["lights"])
    assert all(np.array_equal(P[i], np.asarray(q).astype(np.float32)) for i, q in enumerate(c["lights"]))
    n_tri = sum(len(g["face_index"]) for g in d["geometry"])
    assert (n_tri >= 64) == lc.EXPECT[name]["tri"] and (len(d["spheres"]) >= 64) == lc.EXPECT[name]["sph"]
    lit = shadowed = 0
    for v in c["views"]:
        hit, sh = lc.lit_and_shadowed(d, v)
        reached = (lc.frame(d, v) != 0).any(axis=2)  # by some light (all of them where ~sh)
        lit, shadowed = lit + int((hit & reached).sum()), shadowed + int((hit & sh).sum())
    assert lit > 100 and shadowed > 100
    if len(c["extra_tris"]) or len(c["extra_spheres"]):
        m = np.array(lc.extras_matter(c))
        print(f"\n{name}: pixels its primitives change {m[:, 0].sum()}, shadowed {m[:, 1].sum()}, lit {m[:, 2].sum()}")
        assert m[:, 1].sum() > 0 and (m[:, 2].sum() > 0 or not lc.EXPECT[name]["seen"])


def test_geometry_of_the_cases():
    """the numbers the case descriptions rest on"""
    c = lc.case("triangle cut by face planes")
    for t in c["extra_tris"]:
        v = t - c["p"]
        n = np.cross(t[1] - t[0], t[2] - t[0])
        dist = abs(v[0] @ n) / np.linalg.norm(n)
        assert 1.0 <= dist <= 2.0
        u = v / np.linalg.norm(v, axis=1)[:, None]
        assert min(u[0] @ u[1], u[1] @ u[2], u[0] @ u[2]) < 0.0, "spans more than 90 degrees"
        assert len(set(lc.face_of(v))) == 3, "its corners lie on three faces"
    c = lc.case("P nearly in triangles' planes")
    dists = []
    for t in c["extra_tris"].astype(np.float32).astype(float):
        n = np.cross(t[1] - t[0], t[2] - t[0])
        dists.append(abs((t[0] - c["p"]) @ n) / np.linalg.norm(n))
        assert np.linalg.norm(t - c["p"], axis=1).max() > 3.0
    assert min(dists) == 0.0 and sorted(dists)[1] < 2e-6 and max(dists) < 1.2e-4, dists
    c = lc.case("P inside a sphere's reach")
    s = c["extra_spheres"][0]
    assert abs(np.linalg.norm(s[:3] - c["p"]) - s[3] - 0.01) < 1e-6
    s = lc.case("P inside a sphere")["extra_spheres"][0]
    assert np.linalg.norm(s[:3] - c["p"]) < s[3]
    t = lc.case("P beside a small triangle")["extra_tris"][0]
    n = np.cross(t[1] - t[0], t[2] - t[0])
    assert abs(abs((t[0] - c["p"]) @ n) / np.linalg.norm(n) - 1e-3) < 1e-6
    assert np.linalg.norm(t - c["p"], axis=1).max() < 0.06
    c = lc.case("spheres cut by face planes")
    corner = np.degrees(np.arccos(1 / np.sqrt(3)))
    within = beyond = 0
    for s in c["extra_spheres"]:
        v = s[:3] - c["p"]
        m = int(np.argmin(np.abs(v)))  # the plane through P that cuts it
        assert abs(v[m]) < s[3]
        reach = np.degrees(np.arccos(abs(v[m]) / np.linalg.norm(v)) - np.arcsin(s[3] / np.linalg.norm(v)))
        within, beyond = within + (reach < corner - 5), beyond + (reach > corner + 5)
    assert within >= 2 and beyond >= 4
    for kind in ("spheres", "triangles"):
        c = lc.case(f"cell overflow, {kind}")
        ctr = (c["extra_spheres"][:, :3] if kind == "spheres" else c["extra_tris"].mean(axis=1)) - c["p"]
        assert len(ctr) > 4 * 64 and len(set(lc.face_of(ctr))) == 1
        u = ctr / np.linalg.norm(ctr, axis=1)[:, None]
        assert (u @ u[0]).min() > 1 - 1e-9, "one direction"
        c = lc.case(f"global overflow, {kind}")
        assert len(c["extra_spheres"]) + len(c["extra_tris"]) > 2 * 64 + 2
    c = lc.case("far from the origin")
    assert np.linalg.norm(c["centre"]) > 2000
    c = lc.case("two lights")
    assert c["lights"][0][1] > c["p"][1] + 3.5 and c["lights"][1][1] < c["p"][1] - 3.5
    assert len(lc.case("five lights")["lights"]) == 5


def test_fixed_face_case_has_two_sample_points():
    c = lc.fixed_face_case()
    P = lc.light_points(lc.build(c))
    assert P.shape == (2, 3) and np.array_equal(P[0], c["p"].astype(np.float32))
    assert np.linalg.norm(P[1] - P[0]) > 0.5
