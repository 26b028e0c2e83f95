"""GPU: what esc_lens_rays and esc_render_lens do to the CALLER'S buffers -- which bytes they write, which
they leave alone, what they do around them and to their inputs, and at which addresses they work -- the way
tests/test_caller_buffers.py asks it of the other device entry points.

Every device buffer of every call is an arena of tests/buffer_lib.py: poisoned, between two 64 KiB guards of
its own allocation, at a chosen offset from a 256-byte boundary, and every case runs with both poisons, so an
element that is never written cannot pass by holding its expected value.  After a call every output equals
its expected value byte for byte, an output the call is to leave alone (an empty band, a NULL neighbour)
still holds its poison, the offsets array is byte-identical to what was uploaded, and all guards and pads
stand.

Expected values: the rays are the numpy restatement's (tests/lens_lib.py).  The frame is the SAME call into a
plain, aligned torch buffer; its bits are held by tests/test_lens.py::test_frames_equal_the_composition.

Alignment: 4-byte types run at offsets 0, 4, 8, 12, the byte image at 0, 1, 2, 3."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
import buffer_lib as bl
import lens_cases as lc
import lens_lib as ll
import oracle_lib as ol
from ray_oracle import F32

pytestmark = pytest.mark.gpu

OFFSETS = ((0, 0), (4, 1), (8, 2), (12, 3))  # (4-byte types, bytes) from a 256-byte boundary
SCENE = "c2_200"
S, K = 3, 16


class Keep:
    """an output buffer that is handed to the call and must come back untouched"""

    def __init__(self, nbytes, byte=False):
        self.nbytes, self.byte = int(nbytes), byte


def _is_byte(v):
    return v.byte if isinstance(v, Keep) else v.dtype == np.uint8


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    rr.upload(ol.scene_to_product(ac.scene(SCENE)[0]))
    rr.set_lens_table(lc.table(S, K))
    yield rr
    rr.close()


def run_call(r, what, call, ins, outs, off):
    """call(p) -> rc, p(name) the device pointer of buffer `name`.  ins: {name: array}; outs: {name: expected
    array | Keep}"""
    for poison in bl.POISONS:
        at = lambda v: off[1] if _is_byte(v) else off[0]  # noqa: E731
        A = {k: bl.arena_of(v, at(v), poison) for k, v in ins.items()}
        for k, v in outs.items():
            A[k] = bl.arena(v.nbytes, at(v), poison)
        bl.settle()
        rc = call(lambda k: C.c_void_p(A[k].ptr) if k in A else None)
        r.synchronize()
        tag = f"{what} [poison {poison:#x}, offsets {off}]"
        assert rc == 0, f"{tag}: rc {rc}: {r._lib.esc_last_error().decode('utf-8', 'replace')}"
        for k in ins:
            A[k].check_input(f"{tag}: input {k}")
        for k, v in outs.items():
            if isinstance(v, Keep):
                A[k].check_untouched(f"{tag}: {k}")
            else:
                A[k].check_equals(v, f"{tag}: output {k}")


def lens_options(esc, name, W, H, aperture_share=0.1, seed=lc.LENS_SEED):
    from esctp1raytracer_amd import _capi
    _, ext, dist = lc.camera(name, W, H)
    return _capi.esc_lens_options(float(F32(aperture_share * ext)), dist, seed)


@pytest.mark.parametrize("k_off", range(4))
def test_lens_rays(esc, r, k_off):
    """exactly the band's 24 bytes per ray are written, with the restatement's values; an empty band writes nothing"""
    W, H = 33, 9
    cam = lc.camera(SCENE, W, H)[0]
    lib, h, cc, off = r._lib, r._h, C.byref(cam.c), OFFSETS[k_off]
    tab = lc.table(S, K)
    for share in (0.1, 0.0):
        lo = lens_options(esc, SCENE, W, H, share)
        for r0, r1 in ((0, H), (2, 7), (8, 9), (4, 4)):
            pix = lc.pixels(W, H, (r0, r1))
            n = len(pix)
            for with_offsets in (False, True):
                ins = {"offsets": lc.offsets(n)} if with_offsets and n else {}
                if n:
                    o, d = ll.lens_rays(cam.vectors(), W, H, pix, lo.aperture, lo.focus_dist, tab, K - 1, lc.LENS_SEED,
                                        ins.get("offsets"))
                    assert np.isfinite(o).all() and np.isfinite(d).all()
                    outs = {"o": o, "d": d}
                else:
                    outs = {"o": Keep(48), "d": Keep(48)}
                run_call(r, f"lens_rays aperture {lo.aperture} rows {r0}..{r1} offsets {with_offsets}",
                         lambda p: lib.esc_lens_rays(h, cc, W, H, r0, r1, p("offsets"), C.byref(lo), K - 1, p("o"), p("d")),
                         ins, outs, off)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("W,H", [(33, 9), (64, 8)])
def test_render_lens(esc, r, W, H, k_off):
    """W*H*3 floats and, when asked for, W*H*3 bytes are written, nothing else; NULL for the bytes leaves them alone"""
    import torch
    from esctp1raytracer_amd import _capi
    cam = lc.camera(SCENE, W, H)[0]
    lib, h, cc, off = r._lib, r._h, C.byref(cam.c), OFFSETS[k_off]
    o = esc._options(True, esc.ESC_FACE_FIXED, 0, 77, esc.ESC_STAGE_AUTO)
    to = _capi.esc_trace_options(1, 1e-3, _capi.ESC_TRANSMIT_OFF, 0)
    lo = lens_options(esc, SCENE, W, H)
    call = lambda p: lib.esc_render_lens(h, cc, W, H, 4, C.byref(o), C.byref(to), C.byref(lo), p("f32"), p("u8"))  # noqa: E731
    # the same call into plain aligned buffers (module docstring)
    f32 = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda:0")
    u8 = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda:0")
    bl.settle()
    T = {"f32": f32, "u8": u8}
    assert call(lambda k: C.c_void_p(T[k].data_ptr())) == 0
    r.synchronize()
    want, want8 = f32.cpu().numpy(), u8.cpu().numpy()
    assert np.array_equal(want8, esc.quantise(want).reshape(-1)) and want.any(), "the plain call's own outputs disagree"
    run_call(r, f"render_lens {W}x{H}", call, {}, {"f32": want, "u8": want8}, off)
    run_call(r, f"render_lens {W}x{H}, no u8", lambda p: call(lambda k: None if k == "u8" else p(k)), {},
             {"f32": want, "u8": Keep(want8.nbytes, byte=True)}, off)
