"""CPU: the lens table generator (esc_lens_disk_table runs on the host) and the numpy restatement of the
thin-lens rule (tests/lens_lib.py) on the cases of tests/lens_cases.py.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
import lens_cases as lc
import lens_lib as ll
from ray_oracle import F32, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(c, W, H) for c in lc.CAMERAS for W, H in lc.FRAMES]
IDS = [f"{c}-{W}x{H}" for c, W, H in PAIRS]


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


# ---- the table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,K", [(1, 1), (1, 4), (3, 16), (2, 7), (64, 64), (5, 9), (4, 60)])
def test_lens_table_shape_determinism_and_disk(esc, S, K):
    t = esc.lens_table(S, K, 3)
    assert t.shape == (S, K, 2) and t.dtype == np.float32
    assert np.array_equal(t.view(np.uint32), esc.lens_table(S, K, 3).view(np.uint32)), "not deterministic"
    t64 = t.astype(np.float64)
    r2 = t64[..., 0] ** 2 + t64[..., 1] ** 2
    assert np.isfinite(t).all() and (r2 <= 1.0).all(), f"a point outside the unit disk: max r^2 = {r2.max()!r}"
    assert not np.array_equal(t, esc.lens_table(S, K, 4)), "two seeds give one table"
    if S > 1:
        assert not np.array_equal(t[0], t[1]), "two sets are the same"


def test_lens_table_covers_the_disk(esc):
    """a square K is stratified: every quadrant of the disk holds its quarter of a 16-point set; the mean
    radius squared of many points is that of a uniform disk, 1/2 (64 * 64 points: standard error 0.0045)"""
    t = esc.lens_table(64, 16, 11)
    for s in range(64):
        q = (t[s, :, 0] >= 0).astype(int) * 2 + (t[s, :, 1] >= 0).astype(int)
        assert np.bincount(q, minlength=4).tolist() == [4, 4, 4, 4], (s, q.tolist())
    big = esc.lens_table(64, 64, 1).astype(np.float64)
    assert abs((big ** 2).sum(axis=-1).mean() - 0.5) < 0.03
    # the order inside a set is shuffled: sample k is not cell k of the grid in every set
    first_quadrant = {int((t[s, 0, 0] >= 0) * 2 + (t[s, 0, 1] >= 0)) for s in range(64)}
    assert len(first_quadrant) > 1


def test_lens_table_refuses_bad_arguments(esc):
    from esctp1raytracer_amd import _capi
    lib = _capi.load()
    out = np.zeros(2 * 64 * 64, np.float32)
    for S, K in ((0, 4), (4, 0), (-1, 4), (65, 4), (4, 65)):
        assert lib.esc_lens_disk_table(S, K, 0, esc._fp(out)) == _capi.ESC_ERR_INVALID, (S, K)
        assert b"esc_lens_disk_table" in lib.esc_last_error()
        with pytest.raises(esc.EscError):
            esc.lens_table(S, K)
    assert lib.esc_lens_disk_table(2, 4, 0, None) == _capi.ESC_ERR_INVALID
    assert b"esc_lens_disk_table" in lib.esc_last_error()
    assert not out.any(), "a refused call wrote"


# ---- the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", PAIRS, ids=IDS)
def test_aperture_zero_is_the_pinhole_camera(name, W, H):
    cam = lc.camera(name, W, H)[0]
    o0, d0 = ac.camera_rays(cam, W, H)
    for fd in (1.0, 0.37):
        o, d = ll.lens_rays(cam.vectors(), W, H, lc.pixels(W, H, None), 0.0, fd, None, 0, lc.LENS_SEED)
        assert_same(o, o0, f"{name} {W}x{H} origins")
        assert_same(d, d0, f"{name} {W}x{H} dirs")
    n = 0
    for c in lc.cases(name, W, H):
        if c["aperture"] == 0 and not c["offsets"]:
            r0, r1 = c["rows"] or (0, H)
            o, d = lc.want(c)
            assert_same(o, o0[r0 * W:r1 * W], "rows")
            assert_same(d, d0[r0 * W:r1 * W], "rows")
            n += 1
    assert n == 16


@pytest.mark.parametrize("name,W,H", PAIRS, ids=IDS)
def test_most_rays_of_every_lens_case_leave_the_pinhole_ray(name, W, H):
    """the condition on the inputs: an aperture > 0 case moves at least 90 % of its rays"""
    cs = lc.cases(name, W, H)
    assert len(cs) == 96
    low = 1.0
    for c in cs:
        lc.check_condition(c)
        if c["aperture"] > 0:
            low = min(low, lc.moved_share(c))
        o, d = lc.want(c)
        assert np.isfinite(o).all() and np.isfinite(d).all(), lc.key(c)
    print(f"{name} {W}x{H}: the least share of moved rays over the aperture > 0 cases is {low:.3f}")


@pytest.mark.parametrize("name,W,H", PAIRS, ids=IDS)
def test_every_ray_passes_its_point_of_the_focus_plane(name, W, H):
    """In float64, the line of every ray (o', d') passes F = origin + p*focus_dist.  The allowed distance,
    from the roundings of the written operations, with u = 2^-24 and every |fl(x) - x| <= u |x|:

      off is computed with some error e1:  off = off* + e1  (off* exact in the fp32 inputs)
      o'  = fl(origin + off)     = origin + off + e2,                       |e2| <= u |o'|
      x   = fl(fl(p*fd) - off)   = p*fd - off + e3 + e4,    |e3| <= u |p*fd|, |e4| <= u |x|
      d'  = x / len componentwise: d'_i = (x_i / len)(1 + eps_i), so d' is parallel to g = x + eta,
                                                                            |eta| <= u |x|
    (len is common to the three components and does not turn the direction.)  Then
      F - o' = p*fd - off - e2 = x - e2 - e3 - e4 = g - (eta + e2 + e3 + e4):
    e1 cancels, g lies along the line, and the distance from F to the line is at most
      |eta + e2 + e3 + e4| <= u (|o'| + |p*fd| + 2 |x|)
    in Euclidean norms.  |x| is taken as |F - o'| here, which differs from it by that same small amount; the
    factor 1 + 2^-10 covers this, the second-order terms and the float64 evaluation of the check itself."""
    cam = lc.camera(name, W, H)[0]
    v = cam.vectors()
    u = 2.0 ** -24
    worst = 0.0
    for c in lc.cases(name, W, H):
        pix = lc.pixels(W, H, c["rows"])
        p = ll.pinhole_points(v, W, H, pix, lc.case_offsets(c)).astype(np.float64)
        pf = p * float(F32(c["focus_dist"]))
        if c["aperture"] == 0:  # the rounding of p*fd is not part of a pinhole ray: only eta is
            pf = p
        F = v["origin"].astype(np.float64) + pf
        o, d = (a.astype(np.float64) for a in lc.want(c))
        r = F - o
        dn = d / np.linalg.norm(d, axis=1)[:, None]
        dist = np.linalg.norm(r - (r * dn).sum(axis=1)[:, None] * dn, axis=1)
        allowed = u * (np.linalg.norm(o, axis=1) + np.linalg.norm(pf, axis=1) + 2 * np.linalg.norm(r, axis=1)) * (1 + 2.0 ** -10)
        assert (dist <= allowed).all(), (lc.key(c), float((dist / allowed).max()))
        worst = max(worst, float((dist / allowed).max()))
        # the rays point towards the focus plane, not away from it
        assert ((r * dn).sum(axis=1) > 0).all()
    print(f"{name} {W}x{H}: the largest distance is {worst:.3f} of the allowed one")


def test_declarations_and_struct_layout():
    from esctp1raytracer_amd import _capi
    header = open(os.path.join(ROOT, "include", "esctp1_rt.h")).read()
    for name in ("esc_set_lens_table", "esc_get_lens_table_shape", "esc_lens_disk_table", "esc_lens_rays", "esc_render_lens"):
        assert name + "(" in header and name in _capi.SIGNATURES
    assert C.sizeof(_capi.esc_lens_options) == 24
    assert [f[0] for f in _capi.esc_lens_options._fields_] == ["aperture", "focus_dist", "seed", "reserved"]
    assert _capi.esc_lens_options.seed.offset == 8 and _capi.esc_lens_options.reserved.offset == 16
    for line in ("set = mix(lens.seed, q, 0xFFFFFFFD) mod S", "off = U*(l.x*aperture) + V*(l.y*aperture)",
                 "d'  = normalize(p*focus_dist - off)"):
        assert line in header, line
    lib = _capi.load()  # a null context is refused by name, without a device
    s, k = C.c_int32(), C.c_int32()
    lo = _capi.esc_lens_options(0.0, 1.0, 0)
    assert lib.esc_set_lens_table(None, 1, 1, None) == _capi.ESC_ERR_INVALID and b"esc_set_lens_table" in lib.esc_last_error()
    assert lib.esc_get_lens_table_shape(None, C.byref(s), C.byref(k)) == _capi.ESC_ERR_INVALID
    assert lib.esc_lens_rays(None, None, 4, 4, 0, 4, None, C.byref(lo), 0, None, None) == _capi.ESC_ERR_INVALID
    assert b"esc_lens_rays" in lib.esc_last_error()
    assert lib.esc_render_lens(None, None, 4, 4, 1, None, None, C.byref(lo), None, None) == _capi.ESC_ERR_INVALID
    assert b"esc_render_lens" in lib.esc_last_error()


@pytest.mark.parametrize("args,message", [
    (["--aperture", "0.1"], "--aperture needs --spp"),
    (["--spp", "4", "--aperture", "-1"], "--aperture must be a finite number >= 0"),
    (["--spp", "4", "--aperture", "nan"], "--aperture must be a finite number >= 0"),
    (["--spp", "4", "--aperture", "0.1", "--focus", "0"], "--focus must be a finite number > 0"),
    (["--spp", "4", "--focus", "2"], "--focus and --lens-seed need --aperture"),
    (["--spp", "4", "--lens-seed", "2"], "--focus and --lens-seed need --aperture"),
    (["--spp", "4", "--aperture", "0.1", "--lens-seed", "x"], "--lens-seed must be a whole number"),
    (["--spp", "4", "--aperture", "0.1", "--adaptive", "0.1"], "not with --adaptive or --ao"),
    (["--spp", "4", "--aperture", "0.1", "--ao", "4", "--ao-radius", "1"], "not with --adaptive or --ao"),
    (["--spp", "4", "--aperture", "0.1", "--gpus", "2"], "--spp renders on one GPU"),
    (["--spp", "4", "--aperture", "0.1", "--ispc"], "--spp renders on one GPU"),
])
def test_viewer_refuses_bad_lens_flags(args, message):
    exe = os.path.join(ROOT, "bin", "ESCViewer2021")
    res = subprocess.run([exe] + args, capture_output=True, text=True)
    assert res.returncode != 0 and message in res.stderr, res.stderr
    help_ = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert help_.returncode == 0 and "--aperture A" in help_.stdout and "--focus D --lens-seed S" in help_.stdout


def test_set_does_not_depend_on_the_sample_and_lens_points_are_the_tables():
    """o' - origin of sample k is U*(l.x*a) + V*(l.y*a) with l = table[set(q)][k]: the sets of k = 0 and
    k = K - 1 are the same, and with S = 3 every set is drawn by some pixel of a 33 x 9 frame"""
    sets = ll.lens_sets(lc.LENS_SEED, lc.pixels(33, 9, None), 3)
    assert sorted(set(sets.tolist())) == [0, 1, 2]
    assert np.array_equal(ll.lens_sets(lc.LENS_SEED, lc.pixels(33, 9, (4, 9)), 3), sets[4 * 33:])
    assert not np.array_equal(ll.lens_sets(lc.LENS_SEED + 1, lc.pixels(33, 9, None), 3), sets)
    # sub-pixel grid of spp 4, as esc_render_supersampled writes it
    assert [tuple(float(x) for x in ll.grid_offset(k, 2)) for k in range(4)] == \
        [(-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25)]
