"""GPU: what every device entry point does to the CALLER'S buffers -- which bytes it writes, which it leaves
alone, what it does around them and to its inputs, and at which addresses it works.

Every device buffer of every call here is an arena of tests/buffer_lib.py: poisoned, between two 64 KiB
guards of its own allocation, at a chosen offset from a 256-byte boundary.  Every case runs with both poisons
(0xCD and 0x32), so an element that is never written cannot pass by holding its expected value: not 0 (a
pixel that misses, or whose light is occluded), not -1 (a miss's geom / prim), not 205.  After a call

  - every output equals its expected value byte for byte;
  - an output the header says is left alone (NULL neighbours, n == 0, an empty band, a refused call) still
    holds its poison;
  - every input is byte-identical to what was uploaded;
  - all guards and pads stand: nothing within 64 KiB of any buffer was written.

Expected values are CPU restatements, never a second GPU render: the oracle's frame (oracle_lib) for every
frame call, ray_oracle / ambient_lib / skylight_lib / environment_lib / filter_lib / temporal_lib for the ray
batches and images.  Three calls have no restatement that a few lines can invoke; their expected value is the
SAME call into a plain, aligned torch buffer, and the bits themselves are held by the test named:
  - esc_camera_rays with offsets     tests/test_shade_rays.py::test_camera_rays_pinned
  - esc_trace_rays (depth 2)         tests/test_trace_rays.py::test_bounces_against_the_oracle
  - esc_trace_rays_ex (refraction)   tests/test_transmission.py::test_refraction_against_the_restatement
  - esc_render_supersampled, spp 4   tests/test_shade_rays.py::test_supersampling
(spp 1, depth 0 and the plain camera rays are held to the oracle here.)

Frames: 33 x 9 (one full tile column plus one pixel; H no multiple of 4), 36 x 8 (W % 4 == 0 with a partial
tile), 64 x 8 (full tiles only: the dword path of the u8 store) and 130 x 22, each as the whole frame, rows 6..22,
rows 8..20 and strips of 8 rows for rank 1 of 2 and rank 2 of 3, clipped to the frame -- at H = 8 or 9 some of
these are one short row or no row at all, and an empty piece must write nothing.  Every scene is viewed so that
at least a quarter of the reference's pixels are exactly black (asserted on the oracle's frame): those are the
pixels a zero-filled buffer cannot see.

Alignment: 4-byte types run at offsets 0, 4, 8, 12, byte outputs at 0, 1, 2, 3 (d_rgb_u8 may sit anywhere: the
dword path of write_tile is taken only for an aligned pointer).  A 4-byte pointer at +1 or +2 is refused with
ESC_ERR_INVALID before anything is launched.

Streams: the renderer launches on its own stream and does not wait for torch's: buffer_lib.settle() after the
fills, Renderer.synchronize() before the read-backs.

Not covered here (DESIGN.md 4e lists them): the multi-device calls (their device buffers are the library's
own), esc_render_frame_host and trace() (host pointers), the viewer.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ambient_lib
import buffer_lib as bl
import environment_lib as envl
import filter_lib
import oracle_lib as ol
import ray_oracle as ro
import skylight_lib
import temporal_lib
import tile_list_cases as tc
import tile_tri_mask_cases as mc

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
OFFSETS = ((0, 0), (4, 1), (8, 2), (12, 3))  # (4-byte types, bytes) from a 256-byte boundary
RUNS = {"cases": 0, "calls": 0}


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as esc
    return esc


@pytest.fixture(scope="module")
def r(esc):
    r = esc.Renderer(0)
    yield r
    r.close()
    print(f"\ntest_caller_buffers: {RUNS['cases']} cases, {RUNS['calls']} device calls, each case under both poisons")


@pytest.fixture(scope="module")
def r_env(esc):
    """a context of its own for the calls that need an environment (it changes what traced rays see)"""
    r = esc.Renderer(0)
    yield r
    r.close()


def last_error(r):
    return r._lib.esc_last_error().decode("utf-8", "replace")


# ---- the harness around one call -----------------------------------------------------------------------
class Keep:
    """an output buffer that is handed to the call and must come back untouched"""

    def __init__(self, nbytes, byte=False):
        self.nbytes, self.byte = int(nbytes), byte


def _is_byte(v):
    return v.byte if isinstance(v, Keep) else v.dtype == np.uint8


def run_call(r, what, call, ins, outs, off=(0, 0), alias=None, misplace=None, refused=False):
    """call(p) -> rc, p(name) the device pointer of buffer `name` (None when the call gets NULL for it).
    ins: {name: array}; outs: {name: expected array | Keep}; alias: {output: the input it overwrites};
    misplace: {name: byte offset} overriding `off`; refused: the call must answer ESC_ERR_INVALID with a
    message about alignment, and write nothing."""
    alias = alias or {}
    RUNS["cases"] += 1
    for poison in bl.POISONS:
        at = lambda k, v: (misplace or {}).get(k, off[1] if _is_byte(v) else off[0])  # noqa: E731
        A = {k: bl.arena_of(v, at(k, v), poison) for k, v in ins.items()}
        for k, v in outs.items():
            if k not in alias:
                A[k] = bl.arena(v.nbytes, at(k, v), poison)
        bl.settle()
        rc = call(lambda k: C.c_void_p(A[alias.get(k, k)].ptr) if alias.get(k, k) in A else None)
        RUNS["calls"] += 1
        r.synchronize()
        tag = f"{what} [poison {poison:#x}, offsets {off}]"
        if refused:
            assert rc == -1 and "align" in last_error(r), f"{tag}: rc {rc}, {last_error(r)!r}"
        else:
            assert rc == 0, f"{tag}: rc {rc}: {last_error(r)}"
        for k, v in ins.items():
            if k not in alias.values():
                A[k].check_input(f"{tag}: input {k}")
        for k, v in outs.items():
            a = A[alias.get(k, k)]
            if refused or isinstance(v, Keep):
                if k in alias:
                    a.check_input(f"{tag}: {k}")
                else:
                    a.check_untouched(f"{tag}: {k}")
            else:
                a.check_equals(v, f"{tag}: output {k}")


def plain_call(r, call, ins, shapes):
    """the same call into plain aligned torch buffers -> {name: numpy}; shapes: {name: (dtype, n)}"""
    import torch
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in ins.items()}
    for k, (dt, n) in shapes.items():
        T[k] = torch.zeros(n, dtype=getattr(torch, np.dtype(dt).name), device="cuda:0")
    bl.settle()
    rc = call(lambda k: C.c_void_p(T[k].data_ptr()) if k in T else None)
    r.synchronize()
    assert rc == 0, last_error(r)
    return {k: T[k].cpu().numpy() for k in shapes}


# ---- frames ---------------------------------------------------------------------------------------------
SIZES = ((33, 9), (36, 8), (64, 8), (130, 22))
SCENES = ("masks", "spheres", "mesh")


def pieces_of(H):
    """the issue's pieces clipped to the frame"""
    return (("rows", 0, H), ("rows", min(6, H), min(22, H)), ("rows", min(8, H), min(20, H)),
            ("strips", 8, 1, 2), ("strips", 8, 2, 3))


@functools.lru_cache(maxsize=None)
def frame_scene(name, W, H):
    import esctp1raytracer_amd as esc
    eye, look = mc.EYE, mc.LOOK
    if name == "masks":  # 2 floor triangles, the light's, 5 spheres: a directly swept table with tile masks
        c = mc._c3_layout(f"caller buffers {W}x{H}", W=W, H=H)
        d, cam = c["scene"], c["cam"]
    elif name == "spheres":  # sphere groups, tile lists, light lists
        cam = tc.camera(eye, look, W, H)
        d = ol.scene_from_product(esc.Scene.synthetic("c3", 300))
    else:  # 100 triangles of a patch: triangle groups
        cam = tc.camera(eye, look, W, H)
        d = tc.scene(cam, tc.patch_triangles(cam, 10, 5))
    ref = ol.oracle_render(d, eye, look, W, H, threads=4)
    black = float((ref.view(np.uint32) == 0).all(axis=-1).mean())
    print(f"frame scene {name} {W}x{H}: {black:.3f} of the reference's pixels are exactly black")
    # the condition that makes these tests mean something: pixels whose correct value is what a zeroed buffer holds
    assert 0.25 <= black <= 0.97, f"{name} {W}x{H}: black share {black}"
    return {"d": d, "cam": cam, "eye": eye, "look": look, "product": ol.scene_to_product(d), "key": (name, W, H)}


@functools.lru_cache(maxsize=None)
def frame_ref(name, W, H, piece, shadows=True):
    s = frame_scene(name, W, H)
    rows = tc.local_rows(piece, H).tolist()
    if not rows:
        return np.zeros((0, W, 3), F32), np.zeros((0, W, 3), np.uint8)
    ref, _ = ol.oracle_render_rows(s["d"], s["eye"], s["look"], W, H, rows, shadows=shadows, threads=4)
    return ref, ol.oracle_quantise(ref)


def use_scene(r, s):
    if getattr(r, "_caller_buffers_scene", None) != s["key"]:
        r.upload(s["product"])
        r._caller_buffers_scene = s["key"]


def forms_of(esc):
    return {"default": {}, "two kernels": {"flags": esc.ESC_RENDER_TWO_KERNELS},
            "queue": {"flags": esc.ESC_RENDER_SHADE_QUEUE}, "px1": {"px": 1}, "px2": {"px": 2}, "px4": {"px": 4},
            "lds": {"stage": esc.ESC_STAGE_LDS}, "lds px1": {"stage": esc.ESC_STAGE_LDS, "px": 1},
            "lds px4": {"stage": esc.ESC_STAGE_LDS, "px": 4}, "bvh": {"stage": esc.ESC_STAGE_BVH},
            "no shadows": {"shadows": False}}


FORM_NAMES = ("default", "two kernels", "queue", "px1", "px2", "px4", "lds", "lds px1", "lds px4", "bvh", "no shadows")


def options(esc, shadows=True, stage=0, px=0, flags=0):
    return esc._options(shadows, esc.ESC_FACE_FIXED, 0, 0, stage, px, flags)


def frame_outs(name, W, H, piece, want, shadows=True):
    ref, ref8 = frame_ref(name, W, H, piece, shadows)
    outs = {}
    if want in ("both", "f32"):
        outs["f32"] = ref if len(ref) else Keep(W * 12)
    if want in ("both", "u8"):
        outs["u8"] = ref8 if len(ref8) else Keep(W * 3, byte=True)
    return outs


def render_call(esc, r, s, W, H, piece, o):
    cam = C.byref(s["cam"].c)
    if piece[0] == "rows":
        return lambda p: r._lib.esc_render_rows(r._h, cam, W, H, piece[1], piece[2], C.byref(o), p("f32"), p("u8"))
    return lambda p: r._lib.esc_render_strips(r._h, cam, W, H, piece[1], piece[2], piece[3], C.byref(o), p("f32"),
                                              p("u8"))


def frame_cases():
    out = []
    for W, H in SIZES:  # every size meets every piece and every scene
        for k in range(5):
            for name in SCENES:
                out.append((name, W, H, k, "default", "both", 0))
    for W, H in ((33, 9), (64, 8)):  # every form meets these two sizes
        for form in FORM_NAMES[1:]:
            for name in SCENES:
                out.append((name, W, H, 0, form, "both", 0))
        for form in ("default", "two kernels", "queue", "lds", "bvh"):
            for want in ("f32", "u8"):
                out.append(("masks", W, H, 0, form, want, 0))
                out.append(("spheres", W, H, 3, form, want, 0))
        for form in ("default", "two kernels"):  # every offset, bytes at 1, 2, 3
            for k_off in (1, 2, 3):
                for name in ("masks", "spheres"):
                    for want in ("both", "u8"):
                        out.append((name, W, H, 0, form, want, k_off))
    return out


@pytest.mark.parametrize("name,W,H,k,form,want,k_off", frame_cases(),
                         ids=lambda v: str(v).replace(" ", "_"))
def test_render_rows_and_strips(esc, r, name, W, H, k, form, want, k_off):
    """esc_render_rows (the row pieces) and esc_render_strips (the strip pieces) against the oracle's frame"""
    s, piece, f = frame_scene(name, W, H), pieces_of(H)[k], forms_of(esc)[form]
    use_scene(r, s)
    o = options(esc, **f)
    outs = frame_outs(name, W, H, piece, want, f.get("shadows", True))
    run_call(r, f"{name} {W}x{H} {piece} {form} {want}", render_call(esc, r, s, W, H, piece, o), {}, outs,
             OFFSETS[k_off])
    if form == "default" and k == 0 and want == "both" and k_off == 0:
        kernel = r.last_frame_kernel()
        assert kernel["fused"] and kernel["tgrp"] == (name == "mesh"), kernel
    assert r.frame_tripwire() == 0


def record_cases():
    out = []
    for W, H in SIZES:
        for piece in (("strips", 8, 0, 1), ("strips", 8, 1, 2), ("strips", 8, 2, 3)):
            if len(tc.local_rows(piece, H)):  # (a rank without a strip has nothing to record)
                for name in ("masks", "spheres"):
                    out.append((name, W, H, piece, "default", 0))
    for W, H in ((33, 9), (64, 8)):
        for form in ("two kernels", "queue", "px4"):
            out.append(("spheres", W, H, ("strips", 8, 0, 1), form, 0))
        out.append(("masks", W, H, ("strips", 8, 0, 1), "default", 3))
        out.append(("masks", W, H, ("strips", 8, 0, 1), "two kernels", 1))
    return out


@pytest.mark.parametrize("name,W,H,piece,form,k_off", record_cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_record_strips_and_three_replays(esc, r, name, W, H, piece, form, k_off):
    """esc_frame_record writes the frame (twice: the plain frame and the captured one), and each of three
    esc_frame_launch replays writes all of it again into re-poisoned buffers, and nothing else"""
    s, f = frame_scene(name, W, H), forms_of(esc)[form]
    use_scene(r, s)
    o = options(esc, **f)
    ref, ref8 = frame_ref(name, W, H, piece)
    off = OFFSETS[k_off]
    RUNS["cases"] += 1
    for poison in bl.POISONS:
        a32, a8 = bl.arena(ref.nbytes, off[0], poison), bl.arena(ref8.nbytes, off[1], poison)
        bl.settle()
        h = C.c_void_p()
        rc = r._lib.esc_frame_record(r._h, C.byref(s["cam"].c), W, H, piece[1], piece[2], piece[3], C.byref(o),
                                     C.c_void_p(a32.ptr), C.c_void_p(a8.ptr), C.byref(h))
        assert rc == 0, last_error(r)
        try:
            for replay in range(4):  # 0: what the recording itself left
                if replay:
                    a32.fill()
                    a8.fill()
                    bl.settle()
                    assert r._lib.esc_frame_valid(h) == 1 and r._lib.esc_frame_launch(h) == 0, last_error(r)
                    RUNS["calls"] += 1
                r.synchronize()
                tag = f"{name} {W}x{H} {piece} {form} replay {replay} [poison {poison:#x}]"
                a32.check_equals(ref, tag + ": f32")
                a8.check_equals(ref8, tag + ": u8")
        finally:
            r._lib.esc_frame_destroy(h)


# ---- supersampled, adaptive and traced frames through their device-buffer forms --------------------------
def vectors(cam):
    """the camera's four vectors as temporal_lib takes them"""
    return {k: list(getattr(cam.c, k)) for k in ("origin", "lower_left_corner", "horizontal", "vertical")}


def edge_mask(B, threshold):
    """esc_render_adaptive's M: some 4-neighbour and channel with !(|B - B'| <= threshold)"""
    H, W = B.shape[:2]
    M = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        dv = ~(np.abs(B[1:] - B[:-1]) <= F32(threshold)).all(axis=-1)
        dh = ~(np.abs(B[:, 1:] - B[:, :-1]) <= F32(threshold)).all(axis=-1)
    M[1:] |= dv
    M[:-1] |= dv
    M[:, 1:] |= dh
    M[:, :-1] |= dh
    return M.astype(np.uint8)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("W,H", [(33, 9), (64, 8)])
@pytest.mark.parametrize("name", ["masks", "spheres"])
def test_frames_built_on_shade_rays(esc, r, name, W, H, k_off):
    """spp 1 (and depth 0, and a refinement of one sample) is the frame itself, bit for bit: the oracle's"""
    s = frame_scene(name, W, H)
    use_scene(r, s)
    o, cam, off = options(esc), C.byref(s["cam"].c), OFFSETS[k_off]
    ref, ref8 = frame_ref(name, W, H, ("rows", 0, H))
    lib, h = r._lib, r._h
    run_call(r, f"supersampled {name} {W}x{H}",
             lambda p: lib.esc_render_supersampled(h, cam, W, H, 1, C.byref(o), p("f32"), p("u8")), {},
             {"f32": ref, "u8": ref8}, off)
    run_call(r, f"supersampled, no u8 {name} {W}x{H}",
             lambda p: lib.esc_render_supersampled(h, cam, W, H, 1, C.byref(o), p("f32"), None), {},
             {"f32": ref, "u8": Keep(ref8.nbytes, byte=True)}, off)
    run_call(r, f"traced {name} {W}x{H}",
             lambda p: lib.esc_render_traced(h, cam, W, H, 1, 0, 1e-3, C.byref(o), p("f32"), p("u8")), {},
             {"f32": ref, "u8": ref8}, off)
    from esctp1raytracer_amd import _capi
    ao = _capi.esc_adaptive_options(1, 0.05, 0, 0)
    run_call(r, f"adaptive {name} {W}x{H}",
             lambda p: lib.esc_render_adaptive(h, cam, W, H, C.byref(o), C.byref(ao), p("f32"), p("u8"), p("mask")), {},
             {"f32": ref, "u8": ref8, "mask": edge_mask(ref, 0.05)}, off)
    run_call(r, f"adaptive, image only {name} {W}x{H}",
             lambda p: lib.esc_render_adaptive(h, cam, W, H, C.byref(o), C.byref(ao), p("f32"), None, None), {},
             {"f32": ref, "u8": Keep(ref8.nbytes, byte=True), "mask": Keep(W * H, byte=True)}, off)
    if k_off == 0:  # four samples per pixel: the same call into plain buffers (module docstring)
        call = lambda p: lib.esc_render_supersampled(h, cam, W, H, 4, C.byref(o), p("f32"), p("u8"))  # noqa: E731
        want = plain_call(r, call, {}, {"f32": (F32, W * H * 3), "u8": (np.uint8, W * H * 3)})
        for off4 in OFFSETS:
            run_call(r, f"supersampled x4 {name} {W}x{H}", call, {}, want, off4)


# ---- ray batches ----------------------------------------------------------------------------------------
NS = (0, 1, 63, 64, 65, 257)
RW, RH = 33, 9
PIXEL_BASE = 1234


@functools.lru_cache(maxsize=None)
def ray_set():
    """257 of the masks scene's 297 camera rays, shuffled so that every prefix holds floor hits, sphere hits and
    misses; and everything the restatements say about them"""
    s = frame_scene("masks", RW, RH)
    d, cam = s["d"], s["cam"]
    rng = np.random.default_rng(11)
    pick = rng.permutation(RW * RH)[:NS[-1]]
    dirs = np.ascontiguousarray(tc.ref_dirs(cam.c, RW, RH).reshape(-1, 3)[pick], F32)
    o = np.ascontiguousarray(np.tile(np.array(cam.c.origin, F32), (len(pick), 1)))
    with np.errstate(all="ignore"):
        hit, occ = ro.ref_queries(d, o, dirs)
        tmax = np.where(rng.random(len(pick)) < 0.5, hit["t"] * F32(0.5), F32(50.0)).astype(F32)
        hit_m, occ_m = ro.ref_queries(d, o, dirs, tmax)
    kinds = (hit["geom"][:63] >= 0).any() and ((hit["geom"][:63] < 0) & (hit["prim"][:63] >= 0)).any() and \
        (hit["prim"][:63] < 0).any()
    assert kinds, "the first 63 rays hold no triangle hit, sphere hit or miss"
    assert (hit["uv"][hit["geom"] < 0] == 0).all() and (hit["t"][hit["prim"] < 0] == F32(FLT_MAX)).all()
    ref, _ = ol.oracle_render_rows(d, s["eye"], s["look"], RW, RH, list(range(RH)), threads=4)
    rgb = np.ascontiguousarray(ref.reshape(-1, 3)[pick])
    return {"s": s, "d": d, "o": o, "dirs": dirs, "pick": pick, "hit": hit, "occ": occ, "tmax": tmax, "hit_m": hit_m,
            "occ_m": occ_m, "rgb": rgb, "rgb8": ol.oracle_quantise(rgb)}


def first(x, n):
    return np.ascontiguousarray(x[:n])


def keeps(n_items, names):
    """outputs for an n == 0 call: room for n_items elements each, all to be left alone"""
    return {k: Keep(n_items * (1 if b else 4), byte=b) for k, b in names.items()}


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_intersect_and_occluded_rays(esc, r, n, k_off):
    R = ray_set()
    use_scene(r, R["s"])
    lib, h, off = r._lib, r._h, OFFSETS[k_off]
    for with_tmax in (False, True):
        hit, occ = (R["hit_m"], R["occ_m"]) if with_tmax else (R["hit"], R["occ"])
        ins = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
        if with_tmax:
            ins["tmax"] = first(R["tmax"], n)
        for with_uv in (False, True):
            if n == 0:
                outs = keeps(4, {"t": 0, "geom": 0, "prim": 0, "uv": 0})
            else:
                outs = {"t": first(hit["t"], n), "geom": first(hit["geom"], n), "prim": first(hit["prim"], n),
                        "uv": first(hit["uv"], n) if with_uv else Keep(8 * n)}
            run_call(r, f"intersect n={n} tmax={with_tmax} uv={with_uv}",
                     lambda p: lib.esc_intersect_rays(h, n, p("o"), p("d"), p("tmax"), p("t"), p("geom"), p("prim"),
                                                      p("uv") if with_uv else None, 0), ins, outs, off)
        run_call(r, f"occluded n={n} tmax={with_tmax}",
                 lambda p: lib.esc_occluded_rays(h, n, p("o"), p("d"), p("tmax"), p("occ"), 0), ins,
                 {"occ": first(occ, n)} if n else keeps(4, {"occ": 1}), off)


@pytest.mark.parametrize("k_off", range(4))
def test_camera_rays(esc, r, k_off):
    """with rows: the reference's rays (tile_list_cases.ref_dirs); with offsets: module docstring"""
    s = frame_scene("masks", RW, RH)
    use_scene(r, s)
    lib, h, cam, off = r._lib, r._h, C.byref(s["cam"].c), OFFSETS[k_off]
    dirs = tc.ref_dirs(s["cam"].c, RW, RH)
    for r0, r1 in ((0, RH), (2, 7), (8, 9), (4, 4)):
        n = (r1 - r0) * RW
        d = np.ascontiguousarray(dirs[r0:r1].reshape(-1, 3))
        o = np.ascontiguousarray(np.tile(np.array(s["cam"].c.origin, F32), (n, 1)))
        outs = {"o": o, "d": d} if n else keeps(12, {"o": 0, "d": 0})
        run_call(r, f"camera_rays rows {r0}..{r1}",
                 lambda p: lib.esc_camera_rays(h, cam, RW, RH, r0, r1, None, p("o"), p("d")), {}, outs, off)
    r0, r1 = 3, 6
    n = (r1 - r0) * RW
    offs = np.random.default_rng(5).uniform(-0.5, 0.5, (n, 2)).astype(F32)
    call = lambda p: lib.esc_camera_rays(h, cam, RW, RH, r0, r1, p("offsets"), p("o"), p("d"))  # noqa: E731
    want = plain_call(r, call, {"offsets": offs}, {"o": (F32, 3 * n), "d": (F32, 3 * n)})
    assert not np.array_equal(want["d"], dirs[r0:r1].reshape(-1)), "the offsets moved nothing"
    run_call(r, "camera_rays with offsets", call, {"offsets": offs}, want, off)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_shade_rays(esc, r, n, k_off):
    """the frame's rays shaded are the frame's pixels (the oracle's); t, geom, prim are esc_intersect_rays'"""
    R = ray_set()
    use_scene(r, R["s"])
    lib, h, off, o = r._lib, r._h, OFFSETS[k_off], options(esc)
    ins = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
    full = {"rgb": first(R["rgb"], n), "rgb8": first(R["rgb8"], n), "t": first(R["hit"]["t"], n),
            "geom": first(R["hit"]["geom"], n), "prim": first(R["hit"]["prim"], n)}
    if n == 0:
        full = keeps(4, {"rgb": 0, "rgb8": 1, "t": 0, "geom": 0, "prim": 0})
    for given in (("rgb", "rgb8", "t", "geom", "prim"), ("rgb",), ("rgb", "rgb8"), ("rgb", "prim")):
        outs = {k: (v if k in given else Keep(v.nbytes, byte=(k == "rgb8"))) for k, v in full.items()}
        g = lambda p, k: p(k) if k in given else None  # noqa: E731
        run_call(r, f"shade_rays n={n} {given}",
                 lambda p: lib.esc_shade_rays(h, n, p("o"), p("d"), PIXEL_BASE, C.byref(o), g(p, "rgb"), g(p, "rgb8"),
                                              g(p, "t"), g(p, "geom"), g(p, "prim")), ins, outs, off)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_trace_rays(esc, r, n, k_off):
    """depth 0 is esc_shade_rays (the oracle's colours); depth 2 and refraction: module docstring"""
    from esctp1raytracer_amd import _capi
    R = ray_set()
    d = dict(R["d"])
    glass = ol.scene_to_product(d)
    on_sphere = (R["hit"]["geom"] < 0) & (R["hit"]["prim"] >= 0)
    k_glass = int(np.bincount(R["hit"]["prim"][on_sphere]).argmax())  # the sphere most rays see
    glass.set_sphere_transmission(k_glass, [(0.9, 0.9, 0.9)], [1.5])  # one transmissive material
    r.upload(glass)
    r._caller_buffers_scene = None
    lib, h, off, o = r._lib, r._h, OFFSETS[k_off], options(esc)
    ins = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
    empty = keeps(4, {"rgb": 0, "rgb8": 1})
    depth0 = lambda p: lib.esc_trace_rays(h, n, p("o"), p("d"), PIXEL_BASE, C.byref(o), 0, 1e-3, p("rgb"), p("rgb8"))  # noqa: E731
    run_call(r, f"trace_rays depth 0 n={n}", depth0, ins,
             {"rgb": first(R["rgb"], n), "rgb8": first(R["rgb8"], n)} if n else empty, off)
    depth2 = lambda p: lib.esc_trace_rays(h, n, p("o"), p("d"), PIXEL_BASE, C.byref(o), 2, 1e-3, p("rgb"), p("rgb8"))  # noqa: E731
    to = _capi.esc_trace_options(3, 1e-3, _capi.ESC_TRANSMIT_REFRACT, 0)
    ex = lambda p: lib.esc_trace_rays_ex(h, n, p("o"), p("d"), PIXEL_BASE, C.byref(o), C.byref(to), p("rgb"), p("rgb8"))  # noqa: E731
    for what, call in (("trace_rays depth 2", depth2), ("trace_rays_ex refract", ex)):
        want = plain_call(r, call, ins, {"rgb": (F32, 3 * n), "rgb8": (np.uint8, 3 * n)}) if n else empty
        run_call(r, f"{what} n={n}", call, ins, want, off)
        if n:
            run_call(r, f"{what} n={n}, no rgb8", lambda p: call(lambda k: None if k == "rgb8" else p(k)), ins,
                     {"rgb": want["rgb"], "rgb8": Keep(3 * n, byte=True)}, off)
    if n == NS[-1] and k_off == 0:
        st = r.transmit_stats()
        assert st["refracted"] > 0, f"no ray was refracted: {st}"


SETS, SAMPLES = 3, 4


@functools.lru_cache(maxsize=None)
def ambient_ref():
    import esctp1raytracer_amd as esc
    R = ray_set()
    table = esc.ambient_table(SETS, SAMPLES, seed=7)
    cube = envl.random_cube(4, seed=3)
    with np.errstate(all="ignore"):
        w = ambient_lib.ambient(R["d"], R["o"], R["dirs"], table, radius=2.5, bias=1e-3, seed=9, pixel_base=PIXEL_BASE)
        sk = skylight_lib.skylight(R["d"], w, cube, SAMPLES)
    assert (w["count"][~w["has"]] == SAMPLES).all() and (w["count"][w["has"]] < SAMPLES).any()
    return table, cube, w, sk


def ambient_options(flags=0, pixel_base=PIXEL_BASE):
    from esctp1raytracer_amd import _capi
    return _capi.esc_ambient_options(SAMPLES, SETS, 2.5, 1e-3, 9, pixel_base, flags)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_ambient_and_skylight_rays(esc, r_env, n, k_off):
    r = r_env
    R = ray_set()
    table, cube, w, sk = ambient_ref()
    use_scene(r, R["s"])
    r.set_ambient_table(table)
    r.set_environment(cube)
    lib, h, off, ao = r._lib, r._h, OFFSETS[k_off], ambient_options()
    ins = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
    full = {"vis": first(w["vis"], n), "count": first(w["count"], n), "t": first(w["t"], n),
            "geom": first(w["geom"], n), "prim": first(w["prim"], n)}
    sky = {"sky": first(sk["sky"], n), "light": first(sk["light"], n)}
    if n == 0:
        full, sky = keeps(4, dict.fromkeys(full, 0)), keeps(12, dict.fromkeys(sky, 0))
    for given in (tuple(full), ("vis",), ("vis", "count")):
        outs = {k: (v if k in given else Keep(v.nbytes)) for k, v in full.items()}
        g = lambda p, k: p(k) if k in given else None  # noqa: E731
        run_call(r, f"ambient_rays n={n} {given}",
                 lambda p: lib.esc_ambient_rays(h, n, p("o"), p("d"), C.byref(ao), g(p, "vis"), g(p, "count"), g(p, "t"),
                                                g(p, "geom"), g(p, "prim")), ins, outs, off)
    both = {**sky, **full}
    for given in (tuple(both), ("sky",), ("light",), ("light", "vis", "prim")):
        outs = {k: (v if k in given else Keep(v.nbytes)) for k, v in both.items()}
        g = lambda p, k: p(k) if k in given else None  # noqa: E731
        run_call(r, f"skylight_rays n={n} {given}",
                 lambda p: lib.esc_skylight_rays(h, n, p("o"), p("d"), C.byref(ao), g(p, "sky"), g(p, "light"),
                                                 g(p, "vis"), g(p, "count"), g(p, "t"), g(p, "geom"), g(p, "prim")),
                 ins, outs, off)
    # the environment's own lookup
    env = envl.env_ref(cube, first(R["dirs"], n))
    outs = {"rgb": env, "rgb8": ol.oracle_quantise(env)} if n else keeps(12, {"rgb": 0, "rgb8": 1})
    for given in (("rgb", "rgb8"), ("rgb",), ("rgb8",)):
        o2 = {k: (v if k in given else Keep(v.nbytes, byte=(k == "rgb8"))) for k, v in outs.items()}
        g = lambda p, k: p(k) if k in given else None  # noqa: E731
        run_call(r, f"environment_rays n={n} {given}",
                 lambda p: lib.esc_environment_rays(h, n, p("d"), g(p, "rgb"), g(p, "rgb8")), {"d": ins["d"]}, o2, off)


GB = ("normal", "position", "albedo", "t", "geom", "prim")


@functools.lru_cache(maxsize=None)
def gbuffer_ref():
    R = ray_set()
    return filter_lib.gbuffer(R["d"], R["o"], R["dirs"])


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_gbuffer_rays(esc, r, n, k_off):
    R, g = ray_set(), gbuffer_ref()
    use_scene(r, R["s"])
    lib, h, off = r._lib, r._h, OFFSETS[k_off]
    ins = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
    full = {k: first(np.ascontiguousarray(g[k]), n) for k in GB}
    if n == 0:
        full = keeps(12, dict.fromkeys(GB, 0))
    for given in (GB,) + tuple((k,) for k in GB):  # all six, and each output alone
        outs = {k: (v if k in given else Keep(v.nbytes)) for k, v in full.items()}
        run_call(r, f"gbuffer_rays n={n} {given}",
                 lambda p: lib.esc_gbuffer_rays(h, n, p("o"), p("d"), 0, *[p(k) if k in given else None for k in GB]),
                 ins, outs, off)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("n", NS)
def test_modulate_and_add_light(esc, r, n, k_off):
    """out of place, and with d_out aliasing d_rgb as the header allows; fl(rgb * vis) and fl(rgb + light)"""
    rng = np.random.default_rng(n + 1)
    rgb = rng.uniform(0, 1.4, (n, 3)).astype(F32)
    vis = (rng.integers(0, 5, n) / F32(4)).astype(F32)
    light = rng.uniform(0, 0.5, (n, 3)).astype(F32)
    lib, h, off = r._lib, r._h, OFFSETS[k_off]
    for fn, second, b, want in ((lib.esc_modulate, "vis", vis, (rgb * vis[:, None]).astype(F32)),
                                (lib.esc_add_light, "light", light, (rgb + light).astype(F32))):
        ins = {"rgb": rgb, second: b}
        call = lambda p, fn=fn, second=second: fn(h, n, p("rgb"), p(second), p("out"), p("out8"))  # noqa: E731
        outs = {"out": want, "out8": ol.oracle_quantise(want)} if n else keeps(12, {"out": 0, "out8": 1})
        run_call(r, f"{second} n={n}", call, ins, outs, off)
        if n:
            run_call(r, f"{second} n={n} in place", call, ins, outs, off, alias={"out": "rgb"})
            run_call(r, f"{second} n={n} bytes only", lambda p: call(lambda k: None if k == "out" else p(k)), ins,
                     {"out": Keep(want.nbytes), "out8": outs["out8"]}, off)
            run_call(r, f"{second} n={n} floats only", lambda p: call(lambda k: None if k == "out8" else p(k)), ins,
                     {"out": want, "out8": Keep(3 * n, byte=True)}, off)


# ---- images ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image_ref(W, H):
    """the masks scene's frame rays, their G-buffer, ambient and sky values, and a second (previous) camera"""
    s = frame_scene("masks", W, H)
    cam = s["cam"]
    dirs = np.ascontiguousarray(tc.ref_dirs(cam.c, W, H).reshape(-1, 3))
    o = np.ascontiguousarray(np.tile(np.array(cam.c.origin, F32), (W * H, 1)))
    table, cube, _, _ = ambient_ref()
    with np.errstate(all="ignore"):
        g = filter_lib.gbuffer(s["d"], o, dirs)
        w = ambient_lib.ambient(s["d"], o, dirs, table, radius=2.5, bias=1e-3, seed=9, pixel_base=0)
        sk = skylight_lib.skylight(s["d"], w, cube, SAMPLES)
        prev_cam = tc.camera((0.25, 3.0, 6.0), mc.LOOK, W, H)
        gp = filter_lib.gbuffer(s["d"], np.ascontiguousarray(np.tile(np.array(prev_cam.c.origin, F32), (W * H, 1))),
                                np.ascontiguousarray(tc.ref_dirs(prev_cam.c, W, H).reshape(-1, 3)))
    return {"s": s, "g": g, "w": w, "sk": sk, "prev_cam": prev_cam, "gp": gp}


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("W,H", [(33, 9), (64, 8)])
def test_render_gbuffer_ambient_skylight(esc, r_env, W, H, k_off):
    r = r_env
    I = image_ref(W, H)
    table, cube, _, _ = ambient_ref()
    use_scene(r, I["s"])
    r.set_ambient_table(table)
    r.set_environment(cube)
    lib, h, off, cam, ao = r._lib, r._h, OFFSETS[k_off], C.byref(I["s"]["cam"].c), ambient_options(pixel_base=0)
    g = {k: np.ascontiguousarray(I["g"][k]) for k in GB}
    for given in (GB, ("normal", "prim"), ("t",)):
        outs = {k: (v if k in given else Keep(v.nbytes)) for k, v in g.items()}
        run_call(r, f"render_gbuffer {W}x{H} {given}",
                 lambda p: lib.esc_render_gbuffer(h, cam, W, H, 0, *[p(k) if k in given else None for k in GB]), {}, outs,
                 off)
    w, sk = I["w"], I["sk"]
    run_call(r, f"render_ambient {W}x{H}", lambda p: lib.esc_render_ambient(h, cam, W, H, C.byref(ao), p("vis"), p("count")),
             {}, {"vis": w["vis"], "count": w["count"]}, off)
    run_call(r, f"render_ambient {W}x{H}, no count",
             lambda p: lib.esc_render_ambient(h, cam, W, H, C.byref(ao), p("vis"), None), {},
             {"vis": w["vis"], "count": Keep(W * H * 4)}, off)
    full = {"sky": sk["sky"], "light": sk["light"], "vis": w["vis"], "count": w["count"]}
    for given in (tuple(full), ("sky",), ("light", "count")):
        outs = {k: (v if k in given else Keep(v.nbytes)) for k, v in full.items()}
        run_call(r, f"render_skylight {W}x{H} {given}",
                 lambda p: lib.esc_render_skylight(h, cam, W, H, C.byref(ao), *[p(k) if k in given else None
                                                                               for k in full]), {}, outs, off)


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("W,H", [(33, 9), (64, 8)])
def test_filter_guided_and_temporal_accumulate(esc, r, W, H, k_off):
    from esctp1raytracer_amd import _capi
    I = image_ref(W, H)
    lib, h, off = r._lib, r._h, OFFSETS[k_off]
    rng = np.random.default_rng(W)
    guides = {k: np.ascontiguousarray(I["g"][k]) for k in ("normal", "position", "geom", "prim")}
    prev = {"p_" + k: np.ascontiguousarray(I["gp"][k]) for k in ("normal", "position", "geom", "prim")}
    assert I["g"]["has"].any() and not I["g"]["has"].all()
    for ch in (1, 3):
        img = rng.uniform(0, 1, (H, W, ch)).astype(F32)
        for L in (1, 3):
            fo = _capi.esc_filter_options(L, 0.9, 0.5, 1, (C.c_int32 * 2)(0, 0))
            want, _ = filter_lib.atrous(img.reshape(H, W) if ch == 1 else img, guides, L, 0.9, 0.5, True)
            run_call(r, f"filter_guided {W}x{H} ch={ch} L={L}",
                     lambda p: lib.esc_filter_guided(h, W, H, ch, p("in"), p("normal"), p("position"), p("geom"),
                                                     p("prim"), C.byref(fo), p("out")),
                     {"in": img, **guides}, {"out": np.ascontiguousarray(want, F32)}, off)
        hist = rng.uniform(0, 1, (H, W, ch)).astype(F32)
        hist_n = rng.integers(0, 6, (H, W)).astype(np.int32)
        for taps in (1, 4):
            to = _capi.esc_temporal_options(taps, 8, 0.9, 0.5, 1, (C.c_int32 * 3)(0, 0, 0))
            shape = (lambda x: x.reshape(H, W)) if ch == 1 else (lambda x: x)
            want, want_n, st = temporal_lib.accumulate(shape(img), guides, vectors(I["prev_cam"]), shape(hist), hist_n,
                                                       {k[2:]: v for k, v in prev.items()}, taps=taps, max_history=8,
                                                       normal_cos=0.9, plane_dist=0.5, same_object=True)
            assert st["taps_accepted"] > 0, "no history tap was accepted: nothing but copies"

            def call(p, to=to):
                gc = _capi.esc_guides(p("normal"), p("position"), p("geom"), p("prim"))
                gp = _capi.esc_guides(p("p_normal"), p("p_position"), p("p_geom"), p("p_prim"))
                return lib.esc_temporal_accumulate(h, C.byref(I["prev_cam"].c), W, H, ch, p("cur"), C.byref(gc),
                                                   p("hist"), p("hist_n"), C.byref(gp), C.byref(to), p("out"),
                                                   p("out_n"))
            ins = {"cur": img, "hist": hist, "hist_n": hist_n, **guides, **prev}
            outs = {"out": np.ascontiguousarray(want, F32), "out_n": np.ascontiguousarray(want_n, np.int32)}
            run_call(r, f"temporal_accumulate {W}x{H} ch={ch} taps={taps}", call, ins, outs, off)
            run_call(r, f"temporal_accumulate {W}x{H} ch={ch} taps={taps}, out = current", call, ins, outs, off,
                     alias={"out": "cur"})


@pytest.mark.parametrize("k_off", range(4))
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("W,H", [(33, 9), (64, 8), (36, 22)])
@pytest.mark.parametrize("bpp", [12, 3])
def test_assemble_strips(esc, r, W, H, bpp, world, k_off):
    """the oracle's frame cut into the ranks' blocks, each block padded and the padding poisoned: the frame comes
    back whole, the padding neither reaches it nor changes.  H is no multiple of the strip height (8)"""
    if (W, H) in SIZES:
        ref, ref8 = frame_ref("masks", W, H, ("rows", 0, H))
    else:  # 36 x 22: any image will do for a copy; three strips, the last one short
        ref = np.random.default_rng(3).uniform(0, 1, (H, W, 3)).astype(F32)
        ref8 = ol.oracle_quantise(ref)
    frame = ref if bpp == 12 else ref8
    rows = [tc.local_rows(("strips", 8, k, world), H) for k in range(world)]
    row_bytes = W * bpp
    pitch = max(len(x) for x in rows) * row_bytes + 64  # 64 bytes of padding behind the longest block
    off = OFFSETS[k_off]
    at = off[0] if bpp == 12 else off[1]
    RUNS["cases"] += 1
    for poison in bl.POISONS:
        gathered = np.full(world * pitch, poison, np.uint8)
        for k, x in enumerate(rows):
            gathered[k * pitch:k * pitch + len(x) * row_bytes] = frame[x].reshape(-1).view(np.uint8)
        a_in, a_out = bl.arena_of(gathered, at, poison), bl.arena(frame.nbytes, at, poison)
        bl.settle()
        rc = r._lib.esc_assemble_strips(r._h, C.c_void_p(a_in.ptr), world, pitch, W, H, 8, bpp, C.c_void_p(a_out.ptr))
        RUNS["calls"] += 1
        r.synchronize()
        assert rc == 0, last_error(r)
        a_in.check_input(f"assemble {W}x{H} bpp {bpp} world {world}: gathered")
        a_out.check_equals(frame, f"assemble {W}x{H} bpp {bpp} world {world}: frame")
    if bpp == 12 and k_off == 0:  # the Python layer sizes both buffers
        a_in, a_out = bl.arena_of(gathered, 0), bl.arena(frame.nbytes, 0)
        need = max(k * pitch + len(x) * row_bytes for k, x in enumerate(rows) if len(x))  # (a rank without rows is not read)
        bl.settle()
        r.assemble_strips(a_in.payload[:need], world, pitch, W, H, a_out.payload, bytes_per_pixel=bpp)
        r.synchronize()
        a_out.check_equals(frame, "assemble through the Python layer")
        a_out.fill()
        bl.settle()
        for g, f in ((a_in.payload[:need - 1], a_out.payload), (a_in.payload, a_out.payload[:-1])):
            with pytest.raises(ValueError, match="device buffer too small"):
                r.assemble_strips(g, world, pitch, W, H, f, bytes_per_pixel=bpp)
        r.synchronize()
        a_out.check_untouched("assemble refused by the Python layer")


# ---- refusals -------------------------------------------------------------------------------------------
def test_misaligned_pointers_are_refused_and_nothing_is_written(esc, r, r_env):
    """every 4-byte device pointer parameter at +1 and +2 bytes: ESC_ERR_INVALID, a message that names the
    alignment, nothing launched (every buffer keeps its poison), and a recorded frame stays valid"""
    from esctp1raytracer_amd import _capi
    R = ray_set()
    s, n, W, H = R["s"], 5, 64, 8
    table, cube, _, _ = ambient_ref()
    for rr in (r, r_env):
        use_scene(rr, frame_scene("masks", W, H))
    r_env.set_ambient_table(table)
    r_env.set_environment(cube)
    fs = frame_scene("masks", W, H)
    cam, o, lib = C.byref(fs["cam"].c), options(esc), r._lib
    # a recorded frame of the context, to be replayed after all the refusals
    ref, ref8 = frame_ref("masks", W, H, ("rows", 0, H))
    a32, a8 = bl.arena(ref.nbytes), bl.arena(ref8.nbytes)
    bl.settle()
    frame = C.c_void_p()
    assert lib.esc_frame_record(r._h, cam, W, H, 8, 0, 1, C.byref(o), C.c_void_p(a32.ptr), C.c_void_p(a8.ptr),
                                C.byref(frame)) == 0, last_error(r)
    rays = {"o": first(R["o"], n), "d": first(R["dirs"], n)}
    f4 = lambda k: Keep(4 * k)  # noqa: E731
    px = W * H
    ao, ad = ambient_options(), _capi.esc_adaptive_options(4, 0.05, 0, 0)
    to = _capi.esc_trace_options(2, 1e-3, 1, 0)
    fo = _capi.esc_filter_options(2, 0.9, 0.5, 1, (C.c_int32 * 2)(0, 0))
    tp = _capi.esc_temporal_options(4, 8, 0.9, 0.5, 1, (C.c_int32 * 3)(0, 0, 0))
    img = np.zeros((px, 3), F32)
    gd = {"normal": img, "position": img, "geom": np.zeros(px, np.int32), "prim": np.zeros(px, np.int32)}
    gp = {"p_" + k: v for k, v in gd.items()}

    def temporal(p):
        gc = _capi.esc_guides(p("normal"), p("position"), p("geom"), p("prim"))
        gq = _capi.esc_guides(p("p_normal"), p("p_position"), p("p_geom"), p("p_prim"))
        return lib.esc_temporal_accumulate(r._h, cam, W, H, 3, p("cur"), C.byref(gc), p("hist"), p("hist_n"), C.byref(gq),
                                           C.byref(tp), p("out"), p("out_n"))
    frames = {"f32": f4(3 * px), "u8": Keep(3 * px, byte=True)}
    calls = [  # (context, name, call, inputs, outputs): every 4-byte pointer among them is misplaced in turn
        (r, "esc_render_rows", lambda p: lib.esc_render_rows(r._h, cam, W, H, 0, H, C.byref(o), p("f32"), p("u8")), {}, frames),
        (r, "esc_render_rows, empty band", lambda p: lib.esc_render_rows(r._h, cam, W, H, 4, 4, C.byref(o), p("f32"), p("u8")), {}, frames),
        (r, "esc_render_strips", lambda p: lib.esc_render_strips(r._h, cam, W, H, 8, 0, 1, C.byref(o), p("f32"), p("u8")), {}, frames),
        (r, "esc_frame_record", lambda p: lib.esc_frame_record(r._h, cam, W, H, 8, 0, 1, C.byref(o), p("f32"), p("u8"), C.byref(C.c_void_p())), {}, frames),
        (r, "esc_render_supersampled", lambda p: lib.esc_render_supersampled(r._h, cam, W, H, 4, C.byref(o), p("f32"), p("u8")), {}, frames),
        (r, "esc_render_adaptive", lambda p: lib.esc_render_adaptive(r._h, cam, W, H, C.byref(o), C.byref(ad), p("f32"), p("u8"), None), {}, frames),
        (r, "esc_render_traced", lambda p: lib.esc_render_traced(r._h, cam, W, H, 1, 2, 1e-3, C.byref(o), p("f32"), p("u8")), {}, frames),
        (r, "esc_render_traced_ex", lambda p: lib.esc_render_traced_ex(r._h, cam, W, H, 1, C.byref(o), C.byref(to), p("f32"), p("u8")), {}, frames),
        (r, "esc_assemble_strips", lambda p: lib.esc_assemble_strips(r._h, p("g"), 1, px * 12, W, H, 8, 12, p("f32")), {"g": img}, {"f32": f4(3 * px)}),
        (r, "esc_intersect_rays", lambda p: lib.esc_intersect_rays(r._h, n, p("o"), p("d"), p("tmax"), p("t"), p("geom"), p("prim"), p("uv"), 0),
         {**rays, "tmax": first(R["tmax"], n)}, {"t": f4(n), "geom": f4(n), "prim": f4(n), "uv": f4(2 * n)}),
        (r, "esc_occluded_rays", lambda p: lib.esc_occluded_rays(r._h, n, p("o"), p("d"), p("tmax"), p("occ"), 0),
         {**rays, "tmax": first(R["tmax"], n)}, {"occ": Keep(n, byte=True)}),
        (r, "esc_camera_rays", lambda p: lib.esc_camera_rays(r._h, cam, W, H, 0, 1, p("offsets"), p("o"), p("d")),
         {"offsets": np.zeros((W, 2), F32)}, {"o": f4(3 * W), "d": f4(3 * W)}),
        (r, "esc_shade_rays", lambda p: lib.esc_shade_rays(r._h, n, p("o"), p("d"), 0, C.byref(o), p("rgb"), p("rgb8"), p("t"), p("geom"), p("prim")),
         rays, {"rgb": f4(3 * n), "rgb8": Keep(3 * n, byte=True), "t": f4(n), "geom": f4(n), "prim": f4(n)}),
        (r, "esc_trace_rays", lambda p: lib.esc_trace_rays(r._h, n, p("o"), p("d"), 0, C.byref(o), 2, 1e-3, p("rgb"), p("rgb8")),
         rays, {"rgb": f4(3 * n), "rgb8": Keep(3 * n, byte=True)}),
        (r, "esc_trace_rays_ex", lambda p: lib.esc_trace_rays_ex(r._h, n, p("o"), p("d"), 0, C.byref(o), C.byref(to), p("rgb"), p("rgb8")),
         rays, {"rgb": f4(3 * n), "rgb8": Keep(3 * n, byte=True)}),
        (r_env, "esc_ambient_rays", lambda p: lib.esc_ambient_rays(r_env._h, n, p("o"), p("d"), C.byref(ao), p("vis"), p("count"), p("t"), p("geom"), p("prim")),
         rays, {k: f4(n) for k in ("vis", "count", "t", "geom", "prim")}),
        (r_env, "esc_skylight_rays", lambda p: lib.esc_skylight_rays(r_env._h, n, p("o"), p("d"), C.byref(ao), p("sky"), p("light"), p("vis"), p("count"), p("t"), p("geom"), p("prim")),
         rays, {"sky": f4(3 * n), "light": f4(3 * n), **{k: f4(n) for k in ("vis", "count", "t", "geom", "prim")}}),
        (r_env, "esc_environment_rays", lambda p: lib.esc_environment_rays(r_env._h, n, p("d"), p("rgb"), p("rgb8")),
         {"d": rays["d"]}, {"rgb": f4(3 * n), "rgb8": Keep(3 * n, byte=True)}),
        (r, "esc_gbuffer_rays", lambda p: lib.esc_gbuffer_rays(r._h, n, p("o"), p("d"), 0, *[p(k) for k in GB]),
         rays, {"normal": f4(3 * n), "position": f4(3 * n), "albedo": f4(3 * n), "t": f4(n), "geom": f4(n), "prim": f4(n)}),
        (r, "esc_modulate", lambda p: lib.esc_modulate(r._h, n, p("rgb"), p("vis"), p("out"), p("out8")),
         {"rgb": np.ones((n, 3), F32), "vis": np.ones(n, F32)}, {"out": f4(3 * n), "out8": Keep(3 * n, byte=True)}),
        (r, "esc_add_light", lambda p: lib.esc_add_light(r._h, n, p("rgb"), p("light"), p("out"), p("out8")),
         {"rgb": np.ones((n, 3), F32), "light": np.ones((n, 3), F32)}, {"out": f4(3 * n), "out8": Keep(3 * n, byte=True)}),
        (r, "esc_render_gbuffer", lambda p: lib.esc_render_gbuffer(r._h, cam, W, H, 0, *[p(k) for k in GB]), {},
         {"normal": f4(3 * px), "position": f4(3 * px), "albedo": f4(3 * px), "t": f4(px), "geom": f4(px), "prim": f4(px)}),
        (r_env, "esc_render_ambient", lambda p: lib.esc_render_ambient(r_env._h, cam, W, H, C.byref(ao), p("vis"), p("count")), {},
         {"vis": f4(px), "count": f4(px)}),
        (r_env, "esc_render_skylight", lambda p: lib.esc_render_skylight(r_env._h, cam, W, H, C.byref(ao), p("sky"), p("light"), p("vis"), p("count")), {},
         {"sky": f4(3 * px), "light": f4(3 * px), "vis": f4(px), "count": f4(px)}),
        (r, "esc_filter_guided", lambda p: lib.esc_filter_guided(r._h, W, H, 3, p("in"), p("normal"), p("position"), p("geom"), p("prim"), C.byref(fo), p("out")),
         {"in": img, **gd}, {"out": f4(3 * px)}),
        (r, "esc_temporal_accumulate", temporal, {"cur": img, "hist": img, "hist_n": gd["geom"], **gd, **gp},
         {"out": f4(3 * px), "out_n": f4(px)}),
    ]
    refused = 0
    for ctx, what, call, ins, outs in calls:
        for k in list(ins) + [k for k, v in outs.items() if not v.byte]:
            for delta in (1, 2):
                run_call(ctx, f"{what}: {k} at +{delta}", call, ins, outs, misplace={k: delta}, refused=True)
                refused += 1
    print(f"{refused} misplaced pointers refused")
    # the frame recorded before all this replays as if nothing had happened
    assert lib.esc_frame_valid(frame) == 1
    a32.fill()
    a8.fill()
    bl.settle()
    assert lib.esc_frame_launch(frame) == 0, last_error(r)
    r.synchronize()
    a32.check_equals(ref, "the recorded frame after the refusals: f32")
    a8.check_equals(ref8, "the recorded frame after the refusals: u8")
    lib.esc_frame_destroy(frame)


def test_python_layer_refuses_short_tensors(esc, r):
    """a tensor one element short: ValueError before anything reaches the library, nothing written"""
    import torch
    W, H = 33, 9
    s = frame_scene("masks", W, H)
    use_scene(r, s)
    n = W * H * 3
    a32, a8 = bl.arena(n * 4), bl.arena(n)
    bl.settle()
    f32, u8 = a32.view(torch.float32), a8.payload
    cam = s["cam"]
    for what, fn in (("render_rows f32", lambda: r.render_rows(cam, W, H, 0, H, out_f32=f32[:-1], out_u8=u8)),
                     ("render_rows u8", lambda: r.render_rows(cam, W, H, 0, H, out_f32=f32, out_u8=u8[:-1])),
                     ("render_strips f32", lambda: r.render_strips(cam, W, H, 0, 1, out_f32=f32[:-1], out_u8=u8)),
                     ("render_strips u8", lambda: r.render_strips(cam, W, H, 0, 1, out_f32=f32, out_u8=u8[:-1])),
                     ("record_strips f32", lambda: r.record_strips(cam, W, H, 0, 1, out_f32=f32[:-1], out_u8=u8)),
                     ("record_strips u8", lambda: r.record_strips(cam, W, H, 0, 1, out_f32=f32, out_u8=u8[:-1]))):
        with pytest.raises(ValueError, match="device buffer too small"):
            fn()
    # the ray and image methods take tensors of an exact shape: one element short is no such shape
    R = ray_set()
    k = 7
    ao, ad = bl.arena_of(first(R["o"], k)), bl.arena_of(first(R["dirs"], k))
    outs = {name: bl.arena(k * 4 * c) for name, c in (("t", 1), ("geom", 1), ("prim", 1), ("rgb", 3), ("vis", 1))}
    bl.settle()
    to, td = ao.view(torch.float32, k, 3), ad.view(torch.float32, k, 3)
    t, geom, prim = outs["t"].view(torch.float32), outs["geom"].view(torch.int32), outs["prim"].view(torch.int32)
    rgb, vis = outs["rgb"].view(torch.float32, k, 3), outs["vis"].view(torch.float32)
    for what, fn in (("intersect_rays", lambda: r.intersect_rays(to, td, t[:-1], geom, prim)),
                     ("intersect_rays dirs", lambda: r.intersect_rays(to, td[:-1], t, geom, prim)),
                     ("occluded_rays", lambda: r.occluded_rays(to, td, a8.payload[:k - 1])),
                     ("shade_rays", lambda: r.shade_rays(to, td, rgb[:-1])),
                     ("trace_rays", lambda: r.trace_rays(to, td, rgb[:-1], max_depth=1, bias=1e-3)),
                     ("ambient_rays", lambda: r.ambient_rays(to, td, vis[:-1])),
                     ("gbuffer_rays", lambda: r.gbuffer_rays(to, td, t=t[:-1]))):
        with pytest.raises(ValueError, match="must have shape"):
            fn()
    r.synchronize()
    for a in (a32, a8, *outs.values()):
        a.check_untouched("a call the Python layer refused")
    ao.check_input()
    ad.check_input()


# ---- host read-backs with a capacity --------------------------------------------------------------------
def test_host_readbacks_respect_their_capacity(esc, r):
    """each read-back into a numpy array longer than the stated capacity, and with a capacity below the real
    size: the elements past the capacity keep their fill, the return value and info are the header's"""
    lib, h = r._lib, r._h
    I32 = C.POINTER(C.c_int32)
    ptr = lambda a: a.ctypes.data_as(I32)  # noqa: E731
    for fill in (-0x32323233, 0x32323232):  # 0xCDCDCDCD as int32, 0x32323232
        mk = lambda n: np.full(n, fill, np.int32)  # noqa: E731
        # sphere tile lists and light lists: the grouped sphere scene
        W, H = 130, 22
        s = frame_scene("spheres", W, H)
        use_scene(r, s)
        a32 = bl.arena(W * H * 12)
        bl.settle()
        assert lib.esc_render_rows(h, C.byref(s["cam"].c), W, H, 0, H, C.byref(options(esc)), C.c_void_p(a32.ptr), None) == 0
        hdr = mk(8)
        n_tiles = lib.esc_tile_list_counts(h, 0, ptr(hdr), None, 0)
        assert n_tiles == ((W + 31) // 32) * ((H + 3) // 4) and hdr[3] == (W + 31) // 32 and hdr[4] == (H + 3) // 4
        whole = mk(n_tiles + 8)
        assert lib.esc_tile_list_counts(h, 0, ptr(mk(8)), ptr(whole), n_tiles) == n_tiles
        assert (whole[n_tiles:] == fill).all() and (whole[:n_tiles] >= 0).all()
        part = mk(n_tiles + 8)
        assert lib.esc_tile_list_counts(h, 0, ptr(mk(8)), ptr(part), 3) == n_tiles
        assert np.array_equal(part[:3], whole[:3]) and (part[3:] == fill).all()
        tile = int(np.argmax(whole[:n_tiles]))
        cnt = int(whole[tile])
        assert cnt >= 2, "no tile with two spheres"
        ids = mk(cnt + 8)
        assert lib.esc_tile_list_ids(h, 0, tile, ptr(ids), cnt + 8) == cnt
        m = min(cnt, int(hdr[5]))
        assert (ids[m:] == fill).all() and (ids[:m] >= 0).all()
        short = mk(cnt + 8)
        assert lib.esc_tile_list_ids(h, 0, tile, ptr(short), 1) == cnt
        assert short[0] == ids[0] and (short[1:] == fill).all()
        # the light lists: face counts, a range of cells, and the arrays behind the range untouched
        info = mk(8)
        total = lib.esc_light_list_read(h, 2, ptr(info), None, None, 0, 0, None)
        assert total > 0 and info[0] >= 1 and total == info[0] * 6 * info[1] * info[1]
        cap, faces = int(info[2]), int(info[0]) * 6
        fc, cells = mk(faces + 4), mk(3 * cap + 16)
        assert lib.esc_light_list_read(h, 2, ptr(mk(8)), ptr(fc), None, 5, 3, ptr(cells)) == total
        assert (fc[faces:] == fill).all() and (fc[:faces] >= 0).all()
        assert (cells[3 * cap:] == fill).all() and (cells[:3 * cap] >= -1).all()
        none = mk(cap)
        assert lib.esc_light_list_read(h, 2, ptr(mk(8)), None, None, 5, 0, ptr(none)) == total and (none == fill).all()
        assert lib.esc_light_list_read(h, 2, ptr(mk(8)), None, None, total, 1, ptr(none)) == -1 and (none == fill).all()
        pinfo = mk(8)
        assert lib.esc_light_list_packed_read(h, ptr(pinfo), 0, 0, None, None) == total
        per = int(pinfo[2])
        assert per == 2 * cap and pinfo[3] == 4
        steps, slots = mk(3 + 4), mk(3 * per + 16)
        assert lib.esc_light_list_packed_read(h, ptr(mk(8)), 5, 3, ptr(steps), ptr(slots)) == total
        assert (steps[3:] == fill).all() and (steps[:3] >= -1).all()
        assert (slots[3 * per:] == fill).all() and (slots[:3 * per] >= -1).all()
        # the triangle masks: the masks scene
        W, H = 130, 22
        s = frame_scene("masks", W, H)
        use_scene(r, s)
        assert lib.esc_render_rows(h, C.byref(s["cam"].c), W, H, 0, H, C.byref(options(esc)), C.c_void_p(a32.ptr), None) == 0
        minfo = mk(8)
        n_tiles = lib.esc_tile_tri_masks(h, ptr(minfo), None, 0)
        assert n_tiles == ((W + 31) // 32) * ((H + 3) // 4) and minfo[4] == 3
        U32 = C.POINTER(C.c_uint32)
        whole, part = mk(n_tiles + 8), mk(n_tiles + 8)
        assert lib.esc_tile_tri_masks(h, ptr(mk(8)), whole.ctypes.data_as(U32), n_tiles) == n_tiles
        assert lib.esc_tile_tri_masks(h, ptr(mk(8)), part.ctypes.data_as(U32), 2) == n_tiles
        assert (whole[n_tiles:] == fill).all() and np.array_equal(part[:2], whole[:2]) and (part[2:] == fill).all()
        assert ((whole[:n_tiles] >> 3) == 0).all(), "a bit past the three triangles"
        r.synchronize()
