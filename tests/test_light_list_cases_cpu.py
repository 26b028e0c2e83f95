"""The fixtures of tests/light_list_cases.py do what they were built for -- shown on the reference alone
(oracle frames and ray_oracle's closest hits), before anything of them runs on a GPU.  With these in
place a pair record missing from any cell of the light lists that a shadow ray uses changes a pixel of
tests/test_light_list_directions.py.  Run with -s to see the figures.
"""
import numpy as np
import pytest

import light_list_cases as lc
import oracle_lib as ol


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


# ---- membership (tests/test_light_list_members.py): the restated shadow rays are the reference's, and the
# fixtures give the membership test something no frame shows -------------------------------------------------------
def _scene(which):
    """(key, scene dict, views) as tests/test_light_list_members.py names them"""
    if which in lc.ROOMS:
        c = lc.room(which)
        return ("room", which), lc.build(c), c["views"]
    if which in lc.CASES:
        c = lc.case(which)
        return ("case", which), lc.build(c), c["views"]
    c, _ = lc.corner_case(which)
    return ("corner", which), lc.build(c), c["views"]


@pytest.mark.parametrize("which", list(lc.ROOMS) + ["two lights", "five lights"])
def test_restated_shadow_rays_are_the_oracles(which):
    """lc.shadow_rays restates scan_row; it is pinned, not trusted: as many rays as the oracle counts, and the
    occluded bits it implies reproduce the oracle frames' lit / shadowed split pixel by pixel -- exactly with one
    light; with several, within the two sets lc.implied_split can decide from the rays alone -- and every ray's
    hitp, L, initial t and occluded bit equal the oracle's own record of them (orc_shadow_ray_record)"""
    key, d, views = _scene(which)
    nl = len(d["light_sources"])
    for vi, view in enumerate(views):
        rays, _ = lc.members((key, vi, 0), d, view)
        _, cnt = ol.oracle_render(d, view[0], view[1], lc.W, lc.H, threads=8, return_counters=True)
        assert cnt["shadow_rays"] == len(rays["tb"]) == cnt["hit_pixels"] * nl, (which, vi, cnt, len(rays["tb"]))
        shows, sh = lc.lit_and_shadowed(d, view)
        hit, sure, maybe = lc.implied_split(rays)
        shows, sh = shows.reshape(-1), sh.reshape(-1)
        assert int(hit.sum()) == cnt["hit_pixels"] and not (shows & ~hit).any(), (which, vi)
        print(f"\n{which} view {vi}: {len(rays['tb'])} shadow rays, {int(sh.sum())} pixels differ with shadows, "
              f"{int(sure.sum())} must, {int(maybe.sum())} may")
        assert not (sure & ~sh).any(), f"{which} view {vi}: {int((sure & ~sh).sum())} pixels restated as shadowed are not"
        assert not (sh & ~maybe).any(), f"{which} view {vi}: {int((sh & ~maybe).sum())} shadowed pixels without an occluded ray"
        if nl == 1:
            assert np.array_equal(sh, sure)
        # ... and ray by ray against the oracle's own record of what scan_row traced, bit for bit
        rec = ol.oracle_shadow_rays(d, view[0], view[1], lc.W, lc.H)
        assert np.array_equal(np.flatnonzero(rec[:, :, 7].reshape(-1) > 0), rays["pixel"] * nl + rays["light"]), (which, vi)
        got = rec[rays["pixel"], rays["light"]]
        for k, want in (("hitp", got[:, 0:3]), ("L", got[:, 3:6]), ("tb", got[:, 6])):
            assert np.array_equal(rays[k].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (which, vi, k)
        assert np.array_equal(rays["occluded"], got[:, 7] == 2.0), (which, vi)


@pytest.mark.parametrize("which", list(lc.ROOMS) + ["two shells", "light beside a wall"])
def test_membership_is_not_vacuous(which):
    """every cube face has needed pairs; of a face's cells that hold a ray origin at least a fifth need something
    and at least a fifth need nothing; in the rooms at least a tenth of the needed (cell, primitive) pairs are
    reached only by rays with a second acceptor"""
    key, d, views = _scene(which)
    fig = lc.membership_figures(key, d, views)
    share = len(fig["hidden"]) / len(fig["pairs"])
    print(f"\n{which}: {fig['rays']} shadow rays, {len(fig['pairs'])} needed (cell, primitive) pairs, {len(fig['hidden'])} "
          f"({share:.3f}) only through rays with a second acceptor")
    for f in range(6):
        no, nn = fig["origins"][f], fig["needing"][f]
        print(f"   face {lc.FACE_NAMES[f]}: {no} cells with a ray origin, {nn} of them need something")
        assert nn > 0, f"{which}: face {lc.FACE_NAMES[f]} needs nothing"
        assert nn >= 0.2 * no and no - nn >= 0.2 * no, (which, lc.FACE_NAMES[f], no, nn)
    assert fig["inside"][0] == 1.0, f"{which}: rays of the first light start outside the scene box"
    if which in lc.ROOMS:
        assert share >= 0.10, (which, share)


def test_two_shells_outer_occluders_are_hidden():
    """every occluder of the outer shell has needed pairs that only rays with a second acceptor reach"""
    c = lc.case("two shells")
    key, d, views = _scene("two shells")
    fig = lc.membership_figures(key, d, views)
    n = c["shell"]
    assert len(c["tris"]) == len(c["spheres"]) == 2 * n and not len(c["extra_tris"]) and not len(c["extra_spheres"])
    first_tri = len(lc.triangles_of(d)) - 2 * n  # the lattice's triangles come last (lc.build)
    for kind, outer in (("tri", range(first_tri + n, first_tri + 2 * n)), ("sph", range(n, 2 * n))):
        per = {q: 0 for q in outer}
        for _, k, q in fig["hidden"]:
            if k == kind and q in per:
                per[q] += 1
        print(f"\ntwo shells: hidden pairs per outer {kind}: min {min(per.values())}, median {np.median(list(per.values()))}")
        assert min(per.values()) >= 1, (kind, [q for q, m in per.items() if m == 0])
    # (the twins do line up: most of what the outer shell needs is hidden)
    outer_all = [p for p in fig["pairs"] if (p[1] == "tri" and p[2] >= first_tri + n) or (p[1] == "sph" and p[2] >= n)]
    outer_hidden = [p for p in outer_all if p in fig["hidden"]]
    print(f"two shells: {len(outer_hidden)} of the outer shell's {len(outer_all)} needed pairs are hidden")
    assert len(outer_hidden) >= 0.5 * len(outer_all)


def test_light_beside_a_wall_has_a_short_cone_reach():
    """for at least half of the lattice spheres the reach Rx from the cone of origins (rt_lists.h, float64) is
    below 0.75 R0 AND the case's rays need the sphere"""
    c = lc.case("light beside a wall")
    key, d, views = _scene("light beside a wall")
    assert abs(c["p"][0] + lc.HALF - lc.WALL_GAP) < 1e-6 and len(c["extra_spheres"]) == 1
    hdr = ol.scene_to_product(d).table("header").view(np.float32)
    P = lc.light_points(d)[0]
    sph = d["spheres"]
    ratio = np.ones(len(sph))
    for k in range(1, len(sph)):  # (sphere 0 is the case's own)
        R0, Rx = lc.sphere_reaches(hdr, P, sph[k, :3], np.float32(sph[k, 3] * sph[k, 3]))
        ratio[k] = Rx / R0
    used = np.zeros(len(sph), bool)
    for vi, view in enumerate(views):
        used |= lc.members((key, vi, 0), d, view)[1]["sph"].any(axis=0)
    tight = ratio < 0.75
    print(f"\nlight beside a wall: {len(sph) - 1} lattice spheres, Rx < 0.75 R0 for {int(tight.sum())}, "
          f"{int((tight & used).sum())} of those needed; Rx / R0 from {ratio[1:].min():.3f} to {ratio[1:].max():.3f}")
    assert int((tight & used).sum()) >= 0.5 * (len(sph) - 1)
    assert used[0], "the sphere between P and the wall is needed by nothing"


@pytest.mark.parametrize("which", ["two lights", "five lights"] + lc.CORNER_ORDERS, ids=str)
def test_later_lights_keep_rays_in_the_box(which):
    """quirk S3 moves the later lights' origins; at least a quarter of every light's rays still start in the scene
    box, where the lists serve them -- and the first light's all do"""
    key, d, views = _scene(which)
    fig = lc.membership_figures(key, d, views)
    print(f"\n{which}: share of each light's rays that start inside the scene box: {np.round(fig['inside'], 4).tolist()}")
    assert fig["inside"][0] == 1.0 and (fig["inside"] >= 0.25).all(), fig["inside"]
