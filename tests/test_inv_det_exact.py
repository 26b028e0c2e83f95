"""GPU: the exact tail of the triangle test takes ray_triangle.h:26's `1.0 / det` from inv_det_exact
(csrc/rt_math.h: v_rcp_f64 and two Newton steps) instead of the compiler's f64 division ("The
reciprocal of the exact tail").

 1. every float: esc_check_inv_det_exact runs the helper on the device over ALL 2^32 bit patterns and compares
    it, as 64-bit integers, with 1.0 / (double)x wherever x passes the range test in front of the division --
    every finite |x| >= FLT_EPSILON, the infinities, the NaNs.  Zero mismatches.
 2. every caller: scenes whose frames run the exact tail for every pair (ESC_RENDER_EXACT_ONLY: no filters in
    front of it) and for the survivors of the filters (the default path) give the oracle's bits both ways.
"""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as esc
    return esc


@pytest.fixture(scope="module")
def renderer(esc):
    r = esc.Renderer(0)
    yield r
    r.close()


def test_every_float_pattern(renderer):
    chunk = 1 << 28
    total, firsts = 0, []
    for first in range(0, 1 << 32, chunk):
        bad, lowest = renderer.check_inv_det_exact(first, chunk)
        print(f"patterns 0x{first:08x} .. 0x{first + chunk - 1:08x}: {bad} mismatches"
              + (f", the first 0x{lowest:08x}" if bad else ""))
        total += bad
        if bad:
            firsts.append(lowest)
    assert total == 0, f"{total} float patterns differ from 1.0 / (double)x, the first 0x{min(firsts):08x}"


def test_check_ranges(renderer):
    """the hook's own plumbing: an empty range reports nothing, a range of patterns that all fail the range
    test (|x| < FLT_EPSILON) compares nothing, and a bad argument is refused"""
    assert renderer.check_inv_det_exact(0x3f800000, 0) == (0, 0)
    assert renderer.check_inv_det_exact(0, 1 << 20) == (0, 0)
    import esctp1raytracer_amd as esc
    with pytest.raises(esc.EscError):
        renderer.check_inv_det_exact(0, (1 << 32) + 1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", ["two", "spheres on a floor"])
def test_every_caller(esc, renderer, name):
    if name == "two":  # triangles only, two lights, smooth normals
        d = ol.load_dump("two")
        sc, eye, look = ol.scene_to_product(d), (0.0, 1.0, 3.0), (0.0, 1.0, 0.0)
    else:  # the floor's and the light's triangles among 300 spheres
        sc = esc.Scene.synthetic("c4", 300)
        d = ol.scene_from_product(sc)
        eye, look = esc.synthetic_view()
    w, h = 96, 54
    renderer.upload(sc)
    cam = esc.Camera.for_image(eye, look, w, h)
    ref = ol.oracle_render(d, eye, look, w, h, threads=4)
    assert np.any(ref)
    for what, kw in (("default path", {}), ("exact only", {"flags": esc.ESC_RENDER_EXACT_ONLY}),
                     ("exact only, two kernels", {"flags": esc.ESC_RENDER_EXACT_ONLY | esc.ESC_RENDER_TWO_KERNELS}),
                     ("tree", {"stage": esc.ESC_STAGE_BVH})):
        img = renderer.render(cam, w, h, **kw)
        assert np.array_equal(bits(img), bits(ref)), f"{name}, {what}: differs from the oracle"
