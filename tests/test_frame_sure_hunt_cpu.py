"""CPU: a hunt for statement (I) of DESIGN.md 3.9 "Frames that need no fallback" over all rays and odd scenes
(tests/frame_sure_cases.py: the scenes, cameras and rays; numpy and the host library only).

 a. soundness: for every scene and every camera Scene.shadow_origins_inside accepts -- the last accepted eye
    along eight directions, the lowest accepted eye at five places along a floor's plane, an eye inside, eyes
    4 box sizes out -- the shadow origin of EVERY accepted (ray, primitive) hit of a cube map of directions,
    of limb rays per sphere, of near-in-plane rays per triangle and of rays at the triangles' edges and corners
    lies in [scene_lo, scene_hi], fp32 compares.  Printed: cameras, rays, origins, and the worst distance of a
    hit from its primitive over e_sph and over the triangle's own 4.01 Q / D_min;
 b. teeth: the cameras the predicate refuses do produce origins outside the box, so (a) is not vacuous:
    on "tilted", the five eyes at height 0 and the five at 1e-7 over the floor's plane, 20,000 near-in-plane
    rays each, leave at least 10 origins outside per height (measured with the restated arithmetic alone:
    201 and 200); on "touching", eight eyes 512 box sizes out leave at least 100 outside each with 4,000 limb
    rays (19,547 and more: there b * b - c is rounding noise for every ray that meets a sphere).  With a
    verdict that accepts every camera the check of (a) fails on both;
 c. not empty: yes 4 box sizes out along all eight directions of every scene but "sliver" and "far 1e6", yes
    0.1 over the tilted floor, no for "sliver" at every camera."""
import pytest

import frame_sure_cases as fc


def always(eye):
    return True


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_accepted_cameras_keep_every_origin_inside(name):
    rep = fc.hunt(name)
    print(f"{name}: predicate yes for {rep['yes']} cameras, no for {rep['no']}; {rep['rays']} rays, {rep['origins']} "
          f"accepted hits; {fc.n_escaped(rep)} origins outside the box; worst distance from the primitive: "
          f"{rep['worst_sph']:.4f} e_sph, {rep['worst_tri']:.4f} of the triangle's 4.01 Q / D_min")
    fc.assert_sound(rep)
    if name == "sliver":
        assert rep["yes"] == 0
    else:
        assert rep["yes"] >= 10 and rep["origins"] > 100000, f"{name}: the hunt is nearly empty"


@pytest.mark.parametrize("kind", ["plane 0", "plane +1e-7"])
def test_teeth_camera_in_the_tilted_floors_plane(kind):
    case = fc.scene("tilted")
    cams = fc.pick("tilted", kind)
    assert len(cams) == len(fc.IN_PLANE)
    for c in cams:
        assert abs(fc.height_of(case, c["eye"])) < 1e-6
        assert not case["sc"].shadow_origins_inside(c["eye"]), f"accepted: {c}"
    assert fc.hunt("tilted", cams=cams)["yes"] == 0
    rep = fc.hunt("tilted", always, cams, ("grazing",), total=20000)
    n = fc.n_escaped(rep)
    print(f"tilted, {kind}: {rep['rays']} near-in-plane rays from {rep['yes']} refused cameras, {rep['origins']} accepted "
          f"hits, {n} origins outside the box, by up to {max(e[3] for e in rep['escaped']):.3g}")
    assert n >= 10
    with pytest.raises(AssertionError):
        fc.assert_sound(rep)


def test_teeth_far_camera_on_touching_spheres():
    case = fc.scene("touching")
    cams = fc.pick("touching", "far 512")
    assert len(cams) == len(case["directions"])
    total = 0
    for c in cams:
        assert not case["sc"].shadow_origins_inside(c["eye"]), f"accepted: {c}"
        rep = fc.hunt("touching", always, [c], ("limb",))
        n = fc.n_escaped(rep)
        total += n
        assert n >= 100, f"direction {c['where']}: {n} origins outside"
        with pytest.raises(AssertionError):
            fc.assert_sound(rep)
    print(f"touching, 512 box sizes out: {total} origins outside the box from {len(cams)} refused cameras")


def test_predicate_is_not_empty():
    for name in fc.SCENES:
        case = fc.scene(name)
        said = [case["sc"].shadow_origins_inside(c["eye"]) for c in fc.pick(name, "at 4")]
        assert len(said) >= 6
        if name == "sliver":
            assert not any(case["sc"].shadow_origins_inside(c["eye"]) for c in fc.cameras(name))
        elif name not in fc.NEVER:
            assert all(said), f"{name}: refused 4 box sizes out: {said}"
            assert len(fc.pick(name, "last yes")) == len(case["directions"])
            assert not any(case["sc"].shadow_origins_inside(c["eye"]) for c in fc.pick(name, "first no"))
    tilted = fc.scene("tilted")
    for ab in fc.IN_PLANE:
        eye = fc.over_floor(tilted, ab, 0.1)
        assert abs(fc.height_of(tilted, eye) - 0.1) < 1e-5
        assert tilted["sc"].shadow_origins_inside(eye), f"refused 0.1 over the tilted floor at {ab}"
        assert len(fc.pick("tilted", "lowest", ab)) == 1
