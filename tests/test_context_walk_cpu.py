"""CPU: the walks of tests/context_walk_cases.py cover what tests/test_context_walk.py claims for them, and the
oracle alone shows that their frames tell a stale table from a fresh one -- conditions on the pool, no
measurements:

 1. coverage: the walks together upload every ordered pair of distinct scenes, take every ordered pair of values
    of every option axis on a standing scene and camera, and change each key field of ALONE with nothing else;
 2. not vacuous: wherever a frame step follows a frame step of the same size and band and differs from it in
    scene, camera, shadows, fixed_face (on `mixed`) or the HASH seed (under a light with several faces), the two
    oracle images differ in at least 8 pixels of that band -- the previous frame would not pass;
 3. every (scene, camera, size) rendered with shadows has at least 8 pixels whose shadows-on and shadows-off
    colours differ, and at least 8 hit pixels;
 4. `mixed`: fixed_face 0 and 1 give different frames; `mesh`: FIXED lists two lights and HASH one (from the
    scene dict); `spheres`: esc_scene_shadow_origins_inside is 1 for camera A and 0 for camera D;
 5. the pool is what its table says (counts against the thresholds of csrc/rt_device.h), the per-row reference
    is oracle_render's frame, and the walks are deterministic.
"""
import collections

import numpy as np
import pytest

import context_walk_cases as cw
import oracle_lib as ol


@pytest.fixture(scope="module")
def walks():
    return cw.walks()


def differing_pixels(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1).sum())


def test_walks_are_deterministic_and_replayable(walks):
    again = cw.walks()
    assert list(walks) == list(again) == list(cw.WALK_NAMES) and all(again[k] == walks[k] for k in again)
    from context_walk_cases import Opt  # noqa: F401  (what a printed step names)
    for steps in walks.values():
        assert eval(repr(steps)) == steps
        assert steps[0][0] == "upload"


def test_tour_takes_every_ordered_pair_once():
    for n in (2, 4, 7, 15):
        t = cw.tour(range(n))
        pairs = list(zip(t, t[1:]))
        assert len(pairs) == n * (n - 1) == len(set(pairs)) and all(a != b for a, b in pairs)


def test_pool_is_what_its_table_says():
    P = cw.pool()
    count = lambda d: (sum(len(g["face_index"]) for g in d["geometry"]), len(d["spheres"]))  # noqa: E731
    assert count(P["spheres"]["dict"]) == (3, 300) and count(P["spheres_small"]["dict"]) == (3, 70)
    assert count(P["tiny"]["dict"]) == (3, 10) and count(P["masks_only"]["dict"]) == (6, 0)
    assert count(P["mixed"]["dict"]) == (84, 96) and count(P["mesh"]["dict"]) == (291, 0)
    assert count(P["flat"]["dict"]) == (73, 0)
    # groups from 64 primitives of a kind (kSphGroupMinSpheres, kTriGroupMinTris), masks for 1..32 triangles
    for name, e in P.items():
        hdr = ol.scene_to_product(e["dict"]).table("header").view(np.int32)
        n_tri, n_sph = count(e["dict"])
        sg, tg = int(hdr[10]), int(hdr[13])
        assert (sg > 0) == (n_sph >= 64) and (tg > 0) == (n_tri >= 64), (name, sg, tg)
    assert P["mixed"]["light_faces"] == [2, 2] and P["mesh"]["light_faces"] == [1, 2]
    assert cw.FACES[1] in P["mixed"]["faces"] and all(cw.FACES[1] not in P[n]["faces"] for n in P if n != "mixed")
    # the flat arrays are the other upload entry's input, and pass its host-side check
    flat = cw.product("flat")
    flat.check()
    assert (flat.num_triangles, flat.num_lights) == (73, 1)


def test_header_layout_read_above():
    """hdr[10], hdr[13] above are sg_n_grp and tg_n_grp: c4 has sphere groups only, c5 triangle groups only"""
    import esctp1raytracer_amd as esc
    a = esc.Scene.synthetic("c4", 300).table("header").view(np.int32)
    b = esc.Scene.synthetic("c5", 12).table("header").view(np.int32)
    assert a[10] > 0 and a[13] == 0 and b[10] == 0 and b[13] > 0


def test_coverage(walks):
    cov = cw.coverage(walks.values())
    want = {(a, b) for a in cw.SCENES for b in cw.SCENES if a != b}
    assert cov["scenes"] >= want, sorted(want - cov["scenes"])
    for axis, values in cw.AXES.items():
        want = {(a, b) for a in values for b in values if a != b}
        assert cov["axes"][axis] >= want, (axis, sorted(want - cov["axes"][axis]))
    assert cov["alone"] == set(cw.ALONE), sorted(set(cw.ALONE) - cov["alone"])
    # the directed walk alone names every key of its comments at least once
    d = cw.coverage([walks["directed"]])
    assert d["alone"] == set(cw.ALONE)
    assert all(len(d["axes"][k]) > 0 for k in cw.AXES)
    kinds = {s[1] for s in walks["directed"] if s[0] == "rays"}
    assert kinds == set(cw.RAY_KINDS)
    assert {s[0] for steps in walks.values() for s in steps} == {"upload", "frame", "record", "adaptive", "rays"}
    # the tree by name (BVH_HEURISTIC_PADS under ESC_STAGE_BVH) is visited from and left for the list path
    tree = [i for i, _, _, _, _, o in cw.frame_states(walks["directed"]) if cw.stage_of(o) == cw.TREE]
    assert len(tree) >= 4


def test_steps_are_legal(walks):
    P = cw.pool()
    for name, steps in walks.items():
        for i, scene, cam, size, band, o in cw.frame_states(steps):
            where = (name, i, steps[i])
            assert scene in P and cam in cw.CAMERAS and size in cw.SIZES, where
            assert cw.band_rows(band, size[1]), where
            assert cw.face_of(o) in P[scene]["faces"], where
            assert cw.flags_ok(o.flags, o.stage) and o.px in cw.PX and o.stage in cw.STAGES, where
            if steps[i][0] == "record":
                assert band[0] == "strips" and band[1] % 8 == 0, where
                assert not o.flags & cw.esc.ESC_RENDER_TIME_KERNELS, where
            if o.flags & cw.esc.ESC_RENDER_TIME_KERNELS:
                assert o.flags & cw.esc.ESC_RENDER_TWO_KERNELS, where
        scene = cam = None
        for s in steps:
            if s[0] == "upload":
                scene, cam = s[1], None
            elif s[0] == "rays":
                assert s[1] in cw.RAY_KINDS and s[2] in cw.CAMERAS and s[2] != cam and scene, (name, s)
            else:
                cam = s[1]


def test_reference_is_the_oracles_frame():
    for key in (("mixed", "A", 67, 13, 1, cw.HASH, 0, 7), ("spheres", "D", 33, 21, 1, cw.FIXED, 0, 0)):
        img, u8, cnt = cw.oracle_frame(key)
        eye, look, vfov = cw.pool()[key[0]]["cams"][key[1]]
        ref, rc = ol.oracle_render(cw.pool()[key[0]]["dict"], eye, look, key[2], key[3], shadows=True,
                                   face_mode=key[5], fixed_face=key[6], seed=key[7], vfov=vfov, return_counters=True)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)) and np.array_equal(u8, ol.oracle_quantise(ref))
        assert dict(zip(cw.COUNTERS, cnt.sum(axis=0))) == rc
        assert not img.flags.writeable
    step = ("frame", "A", (67, 13), ("strips", 8, 1, 3), cw.DEFAULT)
    rows, _, c = cw.reference(step, "spheres")
    assert rows.shape == (5, 67, 3) and c["primary_rays"] == 5 * 67
    assert cw.band_rows(("rows", 3, 11), 9) == [3, 4, 5, 6, 7, 8] and cw.band_rows(("strips", 8, 1, 3), 8) == []
    assert cw.band_rows(("strips", 16, 0, 2), 33) == list(range(16)) + [32]


def test_a_stale_frame_would_not_pass(walks):
    P = cw.pool()
    checked = collections.Counter()
    for name, steps in walks.items():
        st = list(cw.frame_states(steps))
        for a, b in zip(st, st[1:]):
            if a[3] != b[3] or a[4] != b[4]:
                continue
            ch = cw.changed(a, b)
            multi = max(P[b[1]]["light_faces"]) > 1
            must = ch & {"scene", "camera direction", "camera origin", "shadows"}
            lit = a[5].shadows and b[5].shadows  # (the light's sample point shows in the shadow rays alone)
            if "fixed_face" in ch and b[1] == "mixed" and lit:
                must.add("fixed_face")
            if "seed" in ch and multi and lit:
                must.add("seed")
            if not must:
                continue
            ra = cw.reference(steps[a[0]], a[1])[0]
            rb = cw.reference(steps[b[0]], b[1])[0]
            n = differing_pixels(ra, rb)
            assert n >= 8, f"{name}: steps {a[0]} {steps[a[0]]} and {b[0]} {steps[b[0]]} differ in {sorted(must)} " \
                           f"but their oracle bands in {n} pixels"
            for m in must:
                checked[m] += 1
    assert all(checked[m] > 0 for m in ("scene", "camera direction", "camera origin", "shadows", "fixed_face", "seed")), \
        dict(checked)


def test_shadows_and_hits_show_in_every_view(walks):
    seen = set()
    for steps in walks.values():
        for i, scene, cam, size, band, o in cw.frame_states(steps):
            if o.shadows:
                seen.add((scene, cam, size))
    assert {(s, c) for s, c, _ in seen} >= {(s, "A") for s in cw.SCENES}
    for scene, cam, size in sorted(seen):
        on, _, cnt = cw.oracle_frame(cw.frame_key(scene, cam, size, cw.DEFAULT))
        off, _, _ = cw.oracle_frame(cw.frame_key(scene, cam, size, cw.DEFAULT._replace(shadows=0)))
        assert int(cnt[:, 1].sum()) >= 8, f"{scene} {cam} {size}: {int(cnt[:, 1].sum())} hit pixels"
        n = differing_pixels(on, off)
        assert n >= 8, f"{scene} {cam} {size}: shadows change {n} pixels"


def test_faces_lights_and_the_far_camera():
    P = cw.pool()
    f0 = cw.oracle_frame(cw.frame_key("mixed", "A", (67, 13), cw.DEFAULT))[0]
    f1 = cw.oracle_frame(cw.frame_key("mixed", "A", (67, 13), cw.DEFAULT._replace(fixed_face=1)))[0]
    assert differing_pixels(f0, f1) >= 8
    d = P["mesh"]["dict"]
    assert cw.n_listed(d, cw.FIXED) == 2 and cw.n_listed(d, cw.HASH) == 1
    assert cw.n_listed(P["mixed"]["dict"], cw.FIXED) == 2 and cw.n_listed(P["mixed"]["dict"], cw.HASH) == 0
    sc = ol.scene_to_product(P["spheres"]["dict"])
    assert sc.shadow_origins_inside(P["spheres"]["cams"]["A"][0])
    assert not sc.shadow_origins_inside(P["spheres"]["cams"]["D"][0])
    # B keeps A's origin, C keeps A's look-at; E lies inside the scene's box
    for name, e in P.items():
        c = e["cams"]
        assert c["B"][0] == c["A"][0] and c["B"][1] != c["A"][1] and c["C"][1] == c["A"][1] and c["C"][0] != c["A"][0]
        hdr = ol.scene_to_product(e["dict"]).table("header").view(np.float32)
        assert np.all(hdr[4:7] < c["E"][0]) and np.all(np.array(c["E"][0]) < hdr[7:10]), name


def test_ray_sets():
    o, p = cw.ray_set("spheres", "B")
    assert o.shape == p.shape == (cw.RAY_GRID[0] * cw.RAY_GRID[1], 3) and o.dtype == p.dtype == np.float32
    assert len(o) <= 67 * 13 and np.all(o == o[0]) and len(np.unique(p, axis=0)) == len(p)
