"""GPU: the per-tile triangle masks of a directly swept triangle table (csrc/rt_lists.h "Per-tile triangle
masks") hold every triangle the reference accepts per tile, and the frames rendered through them are the
frames rendered without them.

A table of 1 to 32 triangles has no groups and no lists; k_bin_tri_masks runs k_bin_triangles' own rule
(bin_triangle) per triangle and leaves one 32-bit word per 32 x 4 pixel tile, which the primary pass walks
instead of testing every triangle.  The masks of a rendered frame are read back (Renderer.tile_tri_masks)
and held to tests/tile_list_cases.py's `needed` for the scenes of tests/tile_tri_mask_cases.py: every (tile,
triangle) pair some pixel's reference test accepts with t carried from FLT_MAX, hidden or not.  The other
direction is bounded too, so that "all bits everywhere" cannot pass: a non-global triangle's bits lie in the
tile box of its 12 corners at the largest dilation, grown by one ring.  tests/test_tile_tri_mask_cases_cpu.py
shows on the reference alone that the cases are not vacuous.

Strips: strip_rows must be a multiple of 8 (the frame kernels' workgroup tile is 8 rows high), so the cyclic
strips here are 8 and 16 rows high, and test_strips_of_4_rows_are_refused pins the refusal of 4.

Streams: the renderer runs on a stream of its own and render_rows / render_strips do not wait for torch's, so
render_piece waits for the zero-fill of its fresh buffers before it renders into them.
"""
import numpy as np
import pytest

import oracle_lib as ol
import tile_list_cases as tc
import tile_tri_mask_cases as mc

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


def render_piece(renderer, c, piece, flags=0, px=0):
    """the piece's rows -> ([n_local_rows, W, 3] fp32, the same as uint8)"""
    import torch
    W, H = c["W"], c["H"]
    n = len(tc.local_rows(piece, H))
    buf = torch.zeros(n * W * 3, dtype=torch.float32, device="cuda:0")
    u8 = torch.zeros(n * W * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.current_stream().synchronize()  # the buffers were zeroed on torch's stream, the frame is not on it
    if piece[0] == "rows":
        renderer.render_rows(c["cam"], W, H, piece[1], piece[2], out_f32=buf, out_u8=u8, flags=flags, px=px)
    else:
        got = renderer.render_strips(c["cam"], W, H, piece[2], piece[3], out_f32=buf, out_u8=u8, strip_rows=piece[1],
                                     flags=flags, px=px)
        assert got == n, "the library's restatement of the strip partition"
    renderer.synchronize()
    return buf.cpu().numpy().reshape(n, W, 3), u8.cpu().numpy().reshape(n, W, 3)


def gpu_rays(renderer, c, piece):
    """Renderer.camera_rays of the piece's rows, run by run of consecutive image rows"""
    rows = tc.local_rows(piece, c["H"])
    cuts = [0] + [i for i in range(1, len(rows)) if rows[i] != rows[i - 1] + 1] + [len(rows)]
    o, d = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        to, td = renderer.camera_rays(c["cam"], c["W"], c["H"], rows=(int(rows[a]), int(rows[b - 1]) + 1))
        renderer.synchronize()
        o.append(to.cpu().numpy())
        d.append(td.cpu().numpy())
    return np.concatenate(o).reshape(len(rows), c["W"], 3), np.concatenate(d).reshape(len(rows), c["W"], 3)


def counted(renderer, c, piece, flags):
    renderer.reset_counters()
    render_piece(renderer, c, piece, flags)
    return renderer.counters()


@pytest.mark.parametrize("name", list(mc.CASES))
def test_masks_hold_every_needed_triangle(esc, renderer, name):
    c = mc.case(name)
    d, W, H, n_tri = c["scene"], c["W"], c["H"], c["n_tri"]
    renderer.upload(ol.scene_to_product(d))
    forms = {"default": 0, "vote": esc.ESC_RENDER_VOTE, "idl": esc.ESC_RENDER_NO_PACKED_LIGHT_LISTS,
             "two kernels": esc.ESC_RENDER_TWO_KERNELS}
    for k, piece in enumerate(c["pieces"]):
        what = f"{name}/piece {k} {piece}"
        frame, frame8 = render_piece(renderer, c, piece)
        kernel = renderer.last_frame_kernel()
        st = renderer.tile_tri_masks()
        assert renderer.tile_lists(1) is None, f"{what}: triangle LISTS for a table without groups"
        # ---- 4. the frame: the same without lists and masks, and the oracle's; fp32 and u8; every form
        sweep, sweep8 = render_piece(renderer, c, piece, flags=esc.ESC_RENDER_NO_TILE_LISTS)
        assert renderer.tile_tri_masks() is None, f"{what}: masks under ESC_RENDER_NO_TILE_LISTS"
        nb = int((bits(frame) != bits(sweep)).sum())
        assert nb == 0 and np.array_equal(frame8, sweep8), f"{what}: {nb} fp32 values differ between masks and sweep"
        ref, _ = ol.oracle_render_rows(d, c["eye"], c["look"], W, H, tc.local_rows(piece, H).tolist(), threads=4)
        nb = int((bits(frame) != bits(ref)).sum())
        assert nb == 0, f"{what}: {nb} fp32 values differ from the oracle"
        assert np.array_equal(frame8, ol.oracle_quantise(ref)), f"{what}: u8 differs from the oracle"
        assert np.isfinite(frame).all()
        for form, flags in forms.items():
            if form == "default":
                continue
            img, img8 = render_piece(renderer, c, piece, flags=flags)
            kf = renderer.last_frame_kernel()
            assert (renderer.tile_tri_masks() is not None) == c["masks"][k], f"{what}: {form}: masks"
            assert kf["fused"] == (form != "two kernels"), f"{what}: {form}: {kf}"
            if "80 spheres" in name:  # the forms by name: no fallback sweep / the vote / the id lists
                assert kernel["sure"] and not kernel["idl"], f"{what}: default frame took {kernel}"
                assert (form != "vote" or not kf["sure"]) and (form != "idl" or kf["idl"]), f"{what}: {form}: {kf}"
            nb = int((bits(img) != bits(frame)).sum())
            assert nb == 0 and np.array_equal(img8, frame8), f"{what}: {form}: {nb} fp32 values differ"
        for px in (1, 4):  # kernels that never read a mask: none is built for them, the frame is the same
            img, img8 = render_piece(renderer, c, piece, px=px)
            assert renderer.tile_tri_masks() is None, f"{what}: masks built for {px} pixels per lane"
            nb = int((bits(img) != bits(frame)).sum())
            assert nb == 0 and np.array_equal(img8, frame8), f"{what}: {px} pixels per lane: {nb} fp32 values differ"
        assert renderer.frame_tripwire() == 0, f"{what}: the tripwire"
        # ---- 5. the ray counters
        with_masks = counted(renderer, c, piece, 0)
        without = counted(renderer, c, piece, esc.ESC_RENDER_NO_TILE_LISTS)
        assert with_masks == without and with_masks["primary_rays"] == len(tc.local_rows(piece, H)) * W, \
            f"{what}: counters {with_masks} with masks, {without} without"
        # ---- 2. the rays `needed` was computed for are the rays the frame traces
        o_ref, d_ref = tc.rays(c, piece)
        o_gpu, d_gpu = gpu_rays(renderer, c, piece)
        assert np.array_equal(bits(o_gpu), bits(o_ref)) and np.array_equal(bits(d_gpu), bits(d_ref)), f"{what}: rays"
        if not c["masks"][k]:
            assert st is None, f"{what}: masks where none are due ({n_tri} triangles, band from row {piece[1]})"
            continue
        assert st is not None, f"{what}: no masks"
        assert (st["tiles_x"], st["tile_rows"]) == tc.tile_grid(piece, W, H) and st["n_tri"] == n_tri, what
        assert st["off"] == 0, f"{what}: the masks switched themselves off"
        words = st["masks"].reshape(-1)
        words = words.astype(np.int64)
        assert not ((words | st["global"]) >> n_tri).any(), f"{what}: a bit past the table"
        present = ((words[:, None] >> np.arange(n_tri)[None, :]) & 1).astype(bool)
        is_global = ((st["global"] >> np.arange(n_tri)) & 1).astype(bool)
        nd = mc.needed(c, k)
        print(f"{what}: {int(nd.sum())} needed pairs, {int(present.sum())} bits of {present.size}, "
              f"global {np.flatnonzero(is_global).tolist()}, kernel {kernel}")
        # ---- 1. completeness
        missing = nd & ~present & ~is_global[None, :]
        if missing.any():
            tile, prim = (int(x) for x in np.argwhere(missing)[0])
            pw, ph = tc.first_needed_pixel(c, k, 1, tile, prim)
            raise AssertionError(
                f"{what}: {int(missing.sum())} needed (tile, triangle) pairs have no bit; first: tile {tile} (column "
                f"{tile % st['tiles_x']}, local tile row {tile // st['tiles_x']}), triangle {prim}, needed by pixel "
                f"(w={pw}, h={ph})")
        declared = np.zeros(n_tri, bool)
        declared[list(c["global"])] = True
        assert not (is_global & ~declared).any(), \
            f"{what}: global but not declared: {np.flatnonzero(is_global & ~declared).tolist()}"
        for q in c["zero"]:
            assert not is_global[q] and not present[:, q].any(), f"{what}: zero triangle {q} has a bit"
        # ---- 3. tightness
        bounded = 0
        for q in range(n_tri):
            if is_global[q] or q in c["zero"]:
                continue
            box = mc.corner_box(c, k, q)
            if box is None:
                continue
            bounded += 1
            assert not (present[:, q] & ~box).any(), \
                f"{what}: triangle {q}: tiles {np.flatnonzero(present[:, q] & ~box).tolist()} outside its corners' box"
        print(f"{what}: {bounded} of {int((~is_global).sum())} non-global triangles held to their box")
        if c.get("c3"):
            # (the floor's corners at the LARGEST dilation reach behind the camera: no box for those two)
            assert not is_global.any() and bounded >= 1, what
            clear = (~present).mean(axis=0)
            assert (clear >= 0.5).any(), f"{what}: every triangle has its bit in more than half of the tiles: {clear.tolist()}"
        if "off" in c:
            assert not present[:, c["off"]].any() and not is_global[c["off"]], f"{what}: off screen, yet tested"
            assert present[:, c["cover"]].all() or is_global[c["cover"]], what


def test_tiles_shared_over_several_workgroups(esc, renderer):
    """2048 x 516: 8,256 tiles, so k_bin_tri_masks runs two workgroups per triangle and every wave strides over
    its share of the tiles.  Completeness against the reference, the c3 layout's tightness, and the frame
    against the frame without masks"""
    c = mc.case(mc.LARGE)
    piece, n_tri = c["pieces"][0], c["n_tri"]
    assert mc.mask_workgroups(int(np.prod(tc.tile_grid(piece, c["W"], c["H"])))) == 2
    renderer.upload(ol.scene_to_product(c["scene"]))
    frame, frame8 = render_piece(renderer, c, piece)
    st = renderer.tile_tri_masks()
    sweep, sweep8 = render_piece(renderer, c, piece, flags=esc.ESC_RENDER_NO_TILE_LISTS)
    nb = int((bits(frame) != bits(sweep)).sum())
    assert nb == 0 and np.array_equal(frame8, sweep8), f"{nb} fp32 values differ between masks and sweep"
    o_ref, d_ref = tc.rays(c, piece)
    o_gpu, d_gpu = gpu_rays(renderer, c, piece)
    assert np.array_equal(bits(o_gpu), bits(o_ref)) and np.array_equal(bits(d_gpu), bits(d_ref)), "rays"
    assert st is not None and st["off"] == 0 and st["global"] == 0
    assert (st["tiles_x"], st["tile_rows"]) == tc.tile_grid(piece, c["W"], c["H"])
    words = st["masks"].reshape(-1).astype(np.int64)
    assert not (words >> n_tri).any()
    present = ((words[:, None] >> np.arange(n_tri)[None, :]) & 1).astype(bool)
    nd = mc.needed(c)
    missing = nd & ~present
    assert not missing.any(), f"{int(missing.sum())} needed pairs have no bit; first (tile, triangle) {np.argwhere(missing)[0].tolist()}"
    box = mc.corner_box(c, 0, 2)  # the light's triangle: all 12 corners in front
    assert box is not None and not (present[:, 2] & ~box).any()
    clear = (~present).mean(axis=0)
    print(f"{mc.LARGE}: {int(nd.sum())} needed pairs, {int(present.sum())} bits, clear share per triangle {clear.tolist()}")
    assert (clear >= 0.5).any() and (present.sum(axis=1) == 0).mean() >= 0.2  # (the sky's tiles test nothing)


def test_strips_of_4_rows_are_refused(esc, renderer):
    """strip_rows must be a multiple of 8: esc_strip_local_rows answers ESC_ERR_INVALID and says so"""
    import torch
    from esctp1raytracer_amd import _capi
    c = mc.case("strips of 8")
    renderer.upload(ol.scene_to_product(c["scene"]))
    buf = torch.zeros(c["W"] * c["H"] * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    with pytest.raises(_capi.EscError) as err:
        renderer.render_strips(c["cam"], c["W"], c["H"], 0, 2, out_f32=buf, strip_rows=4)
    assert err.value.code == _capi.ESC_ERR_INVALID and "multiple of 8" in str(err.value)


def test_readback_without_masks(esc, renderer):
    """a grouped triangle table has lists and no masks; the read-back says so and refuses a null info"""
    c = tc.case("triangles/synthetic view")
    renderer.upload(ol.scene_to_product(c["scene"]))
    render_piece(renderer, c, c["pieces"][0])
    assert renderer.tile_tri_masks() is None and renderer.tile_lists(1) is not None
    from esctp1raytracer_amd import _capi
    assert renderer._lib.esc_tile_tri_masks(renderer._h, None, None, 0) == _capi.ESC_ERR_INVALID
