"""GPU: k_frame's SURE instantiation at the boundary of the predicate that admits it, and the vote kernel where
shadow origins really leave the scene box (csrc/rt_kernels.hip k_frame / shadow_wave_lists, DESIGN.md 3.9
"Frames that need no fallback"; tests/frame_sure_cases.py: the scenes, cameras and views).  Every frame is
96 x 24 and is compared with the oracle, fp32 bit for bit and bytes.

 a. the scenes the predicate can accept (tilted floor, its 1e3 and 1e5 translates, slab, big sphere, touching
    spheres), from the last accepted eye along each of the eight directions, from an eye inside the box (inside
    the big sphere: the second root), and over a floor from the lowest accepted eye at each of the five places
    along its plane: a frame at 60 degrees towards the box's middle, one that the box just fills, a narrow
    frame centred on the limb (on the light's side) of the nearest sphere and as tall as its angular radius,
    and, where there is a floor, a narrow frame along it towards its far edge.  The launch takes SURE, the
    tripwire reads 0, the frame is the oracle's and, over each scene's frames, not black (from ten box sizes
    out a frame at 60 degrees is: the others carry the comparison);
 b. "touching" from 512 and from 256 box sizes, a narrow frame on a sphere that touches the box's face: the
    predicate refuses the eye, the oracle's own record of its shadow rays has 336 and 648 pixels whose origin
    lies outside [scene_lo, scene_hi] (at least 8 are asserted), the launch takes the vote kernel, and the
    frame is the oracle's under the default flags and under ESC_RENDER_NO_PACKED_LIGHT_LISTS.  The triangle
    twin yielded no qualifying frame: the ten eyes of frame_sure_cases at height 0 and 1e-7 in the tilted
    floor's plane, fields of 1e-4, 1e-3, 1e-2, 0.1 and 1 degree along the floor, gave no pixel with a shadow
    origin outside the box on the oracle, so the sphere case stands alone;
 c. the 1e3 and 1e5 translates from the synthetic-style view moved with the scene: whichever kernel the launch
    picks, the frame is the oracle's and the tripwire 0; where it picks SURE, the predicate holds."""
import numpy as np
import pytest

import frame_sure_cases as fc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 96, 24
BOUNDARY_SCENES = list(fc.SOUND)


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
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_as_oracle(esc, renderer, case, eye, look, vfov, what, flags=0):
    """render and compare with the oracle -> (kernel, tripwire, lit pixels)"""
    cam = esc.Camera.for_image(eye, look, W, H, vfov=vfov)
    img, u8 = renderer.render(cam, W, H, want_u8=True, flags=flags)
    kern, trip = renderer.last_frame_kernel(), renderer.frame_tripwire()
    ref = ol.oracle_render(case["d"], eye, look, W, H, vfov=vfov, threads=4)
    lit = int((ref.sum(axis=2) > 0).sum())
    print(f"{what}: eye {eye}, vfov {vfov:.3g}: {kern}, tripwire {trip}, {lit} lit pixels")
    bad = bits(img) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.any(axis=2).sum())} pixels differ from the oracle in fp32"
    assert np.array_equal(u8, ol.oracle_quantise(ref)), f"{what}: bytes differ from the oracle's"
    return kern, trip, lit


def boundary_cameras(name):
    cams = fc.pick(name, "last yes") + fc.pick(name, "inside")
    if fc.scene(name)["floor"] is not None:
        cams += fc.pick(name, "lowest")
    return cams


@pytest.mark.parametrize("name", BOUNDARY_SCENES)
def test_sure_at_the_boundary_equals_the_oracle(esc, renderer, name):
    case = fc.scene(name)
    renderer.upload(case["sc"])
    lit_total = 0
    for c in boundary_cameras(name):
        eye = c["eye"]
        assert case["sc"].shadow_origins_inside(eye)
        views = [("60 degrees", fc.eye32(case["mid"]), 60.0), ("whole scene",) + fc.whole_view(case, eye),
                 ("limb",) + fc.limb_view(case, eye)]
        if case["floor"] is not None:
            views.append(("along the floor",) + fc.floor_view(case, eye))
        for view, look, vfov in views:
            what = f"{name}, {c['kind']} {c['where']}, {view}"
            kern, trip, lit = same_as_oracle(esc, renderer, case, eye, look, vfov, what)
            assert kern["fused"] and kern["sure"], f"{what}: {kern}"
            assert trip == 0, f"{what}: the tripwire is set"
            lit_total += lit
    assert lit_total > 500, f"{name}: the frames are (nearly) black"


@pytest.mark.parametrize("which", list(fc.FALLBACK_FRAMES))
def test_origins_that_leave_the_box_take_the_vote_kernel(esc, renderer, which):
    case = fc.scene("touching")
    eye, look, vfov = fc.far_sphere_view(case, *fc.FALLBACK_FRAMES[which])
    assert not case["sc"].shadow_origins_inside(eye)
    rec = ol.oracle_shadow_rays(case["d"], eye, look, W, H, vfov=vfov)[:, 0]
    n_out = int((fc.outside(case, rec[:, :3]) & (rec[:, 7] > 0)).sum())
    print(f"touching, {which}: {int((rec[:, 7] > 0).sum())} shadow rays, {n_out} origins outside the box")
    assert n_out >= 8
    renderer.upload(case["sc"])
    for label, flags in (("default", 0), ("no packed light lists", esc.ESC_RENDER_NO_PACKED_LIGHT_LISTS)):
        what = f"touching, {which}, {label}"
        kern, trip, lit = same_as_oracle(esc, renderer, case, eye, look, vfov, what, flags=flags)
        assert kern["fused"] and not kern["sure"], f"{what}: {kern}"
        assert trip == 0, f"{what}: the tripwire is set"
        assert lit > 100, f"{what}: the frame is (nearly) black"


@pytest.mark.parametrize("name", ["far 1e3", "far 1e5"])
def test_far_translates_equal_the_oracle(esc, renderer, name):
    case = fc.scene(name)
    renderer.upload(case["sc"])
    f = case["floor"]
    # the synthetic view's place relative to its scene -- over one edge of the floor, looking down across it
    eye = fc.eye32(f["p0"] + f["half"] * (0.2 * f["u"] + 1.2 * f["v"]) + 1.4 * f["half"] * f["n"])
    look = fc.eye32(f["p0"] + 0.1 * f["half"] * f["n"])
    kern, trip, lit = same_as_oracle(esc, renderer, case, eye, look, 60.0, name)
    assert kern["fused"], f"{name}: {kern}"
    assert trip == 0, f"{name}: the tripwire is set"
    assert lit > 100, f"{name}: the frame is (nearly) black"
    if kern["sure"]:
        assert case["sc"].shadow_origins_inside(eye)
