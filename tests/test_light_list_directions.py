"""GPU: shadow rays over every direction of the light lists' cube map, both kinds of pair record.

The binning kernels of csrc/rt_lists.h (k_bin_light_pairs, k_bin_light_tri_pairs, k_bin_light_tri_escape,
k_sort_light_cells) are device-only geometry: face axes, "in front of the face's plane" against "cut by
it", the corner rule, `around`, cone entries, caps.  The scenes of tests/light_list_cases.py put the light
in the middle of a closed room with sparse occluders all around it, so that every face of the cube is
used and a record missing from a cell changes a pixel (tests/test_light_list_cases_cpu.py shows that on
the reference alone), and add one scene per geometry class.  Every frame is compared as
test_gpu_lists.py::both_ways compares: lists == sweep (lists off) == oracle, bit for bit on fp32.
"""
import numpy as np
import pytest

import light_list_cases as lc
import oracle_lib as ol

pytestmark = pytest.mark.gpu


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


_refs = {}


def reference(key, d, view, **kw):
    """one oracle frame per (scene, view, options), shared by the tests that compare with it"""
    k = (key, view, tuple(sorted(kw.items())))
    if k not in _refs:
        _refs[k] = lc.frame(d, view, **kw)
        _refs[k].setflags(write=False)
    return _refs[k]


def both_ways(esc, renderer, key, c, flags=0, upload=True, **kw):
    """the case's scene, uploaded once; per view: default (lists) == sweep (lists off) == oracle, and the
    same ray counts.  -> the list statistics after the first view (the lists are per scene).
    kw: fixed_face, for the renderer (ESC_FACE_FIXED is its default) and the oracle alike"""
    d = lc.build(c)
    if upload:
        renderer.upload(ol.scene_to_product(d))
    off = esc.ESC_RENDER_NO_TILE_LISTS | esc.ESC_RENDER_NO_LIGHT_LISTS
    stats = None
    for i, view in enumerate(c["views"]):
        cam = esc.Camera.for_image(view[0], view[1], lc.W, lc.H)
        ref = reference(key, d, view, **kw)
        renderer.reset_counters()
        gpu = renderer.render(cam, lc.W, lc.H, flags=flags, **kw)
        c_lists = renderer.counters()
        if stats is None:
            stats = [renderer.tile_lists(w) for w in (0, 1, 2, 3)]
        assert_bit_equal(gpu, ref, f"{key}/view {i}/lists")
        renderer.reset_counters()
        sweep = renderer.render(cam, lc.W, lc.H, flags=flags | off, **kw)
        c_sweep = renderer.counters()
        assert_bit_equal(sweep, ref, f"{key}/view {i}/sweep")
        for k in ("primary_rays", "hit_pixels", "shadow_rays"):
            assert c_lists[k] == c_sweep[k], (key, i, k)
        assert c_lists["shadow_rays"] > 0
    return stats


def assert_lists(st, sph, tri, what):
    assert (st[2] is not None) == sph, f"{what}: light lists of sphere pair records"
    assert (st[3] is not None) == tri, f"{what}: light lists of triangle pair records"


def assert_served(st, what):
    """no cell and no face list over its cap, nothing switched off: the lists served every ray"""
    for s in st[2:]:
        if s is not None:
            assert s["off"] == 0 and s["global"] <= s["global_cap"], what
            assert int(s["counts"].max()) <= s["cap"], f"{what}: a cell holds {int(s['counts'].max())} records"
            assert int((s["counts"] > 0).sum()) > 0


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_every_direction(esc, renderer, variant):
    """the six views of the room: every face of the cube map serves shadow rays, from its own lists"""
    c = lc.room(variant)
    n_tri, n_sph = lc.ROOMS[variant]
    st = both_ways(esc, renderer, variant, c)
    assert_lists(st, n_sph > 0, n_tri > 0, variant)  # (the 13 triangles of room and light alone: not grouped)
    assert_served(st, variant)
    for s, n in ((st[2], n_sph), (st[3], n_tri)):
        if n:  # every face of the light's cube has cells with records
            per_face = s["counts"].reshape(6, -1)
            assert (per_face.max(axis=1) > 0).all(), variant


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_two_kernels(esc, renderer, variant):
    """the same views with the frame split into k_primary and k_shade"""
    st = both_ways(esc, renderer, variant, lc.room(variant), flags=esc.ESC_RENDER_TWO_KERNELS)
    assert_served(st, variant)


@pytest.mark.parametrize("variant", list(lc.ROOMS))
def test_room_bvh(esc, renderer, variant, bvh_tree):
    """ESC_STAGE_BVH: no lists, but light-space bins with the same blind spot; bit equality with the oracle"""
    c = lc.room(variant)
    d = lc.build(c)
    renderer.upload(ol.scene_to_product(d))
    for i, view in enumerate(c["views"]):
        cam = esc.Camera.for_image(view[0], view[1], lc.W, lc.H)
        gpu = renderer.render(cam, lc.W, lc.H, stage=esc.ESC_STAGE_BVH)
        assert_bit_equal(gpu, reference(variant, d, view), f"bvh/{variant}/view {i}")


@pytest.mark.parametrize("name", list(lc.CASES))
def test_geometry_class(esc, renderer, name):
    """one scene per class of the binning kernels' geometry (light_list_cases.CASES)"""
    c = lc.case(name)
    want = lc.EXPECT[name]
    st = both_ways(esc, renderer, name, c)
    assert_lists(st, want["sph"], want["tri"], name)
    s = st[3] if want["tri"] and not want["sph"] else st[2]  # the kind the case is about
    if want["over"] == "cell":
        assert int(s["counts"].max()) > s["cap"], f"{name}: no cell overflowed ({int(s['counts'].max())})"
    elif want["over"] == "global":
        assert s["global"] > s["global_cap"], f"{name}: no face list overflowed ({s['global']})"
    else:
        assert_served(st, name)
    if name == "P nearly in triangles' planes":
        assert st[3]["cones"] > 0, "no cone entries"
    if name in ("P inside a sphere's reach", "P inside a sphere", "P beside a small triangle"):
        assert s["global"] >= 1, "nothing listed for every direction"
    # both kinds of pixel where the case's own primitives matter (oracle frames only)
    if len(c["extra_tris"]) or len(c["extra_spheres"]):
        m = np.array(lc.extras_matter(c))
        assert m[:, 1].sum() > 0 and (m[:, 2].sum() > 0 or not lc.EXPECT[name]["seen"]), (name, m.tolist())


def test_fixed_face_of_a_two_face_light_in_the_room(esc, renderer):
    """ESC_FACE_FIXED, faces 0, 1, 0 of a two-face light at the room's middle: the lists are rebuilt for
    the other sample point and back"""
    c = lc.fixed_face_case()
    seen = []
    for n, face in enumerate((0, 1, 0)):
        st = both_ways(esc, renderer, "fixed face", c, upload=n == 0, fixed_face=face)
        assert_lists(st, True, True, f"fixed face {face}")
        assert_served(st, f"fixed face {face}")
        seen.append(st[3]["counts"].copy())
    assert np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[0], seen[1])
