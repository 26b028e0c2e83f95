"""The environment cube map on the GPU (esc_set_environment, k_environment_rays, the ENV instantiations of
k_trace), bit for bit against the CPU restatements of tests/environment_lib.py: the lookup in numpy fp32, and
ray_oracle.oracle_trace with a `colours` callable that gives every ray that misses the colour env(d).

The cases and their conditions are tests/environment_cases.py's: decided on the CPU, asserted by
test_environment_cpu.py and again here before anything is compared.  Only Ns == 0 cases are used, so that no
tolerance is needed anywhere (ray_cases.py's docstring says what powf costs otherwise).

Misses per level of the trace cases at depth 5, of the rays per level (levels 0, 1, 2):
rand3 25 of 160, 62 of 103, 17 of 36; rand5 32 of 159, 65 of 114, 23 of 47; cornell_mixed 128 of 192, 11 of
40, 7 of 20; mirror_floor_camera 0 of 192, 20 of 43, 8 of 8.  glass_open: 41 of 192 rays meet glass, and 41
(REFRACT) / 36 (FRESNEL) refracted rays reach the environment."""
import os
import subprocess

import numpy as np
import pytest

import environment_cases as ec
import environment_lib as el
import oracle_lib as ol
from ray_cases import product
from ray_oracle import F32, FRESNEL, MODE_NAME, REFRACT, assert_same, same_bits, stats_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, PIXEL_BASE = 77, 1234  # oracle_trace's defaults


@pytest.fixture(scope="module")
def esc():
    import esctp1raytracer_amd as m
    return m


@pytest.fixture(scope="module")
def r(esc):
    rr = esc.Renderer(0)
    yield rr
    rr.close()


# ---- 1. the lookup kernel ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("res", ec.LOOKUP_RES)
def test_lookup_kernel_equals_the_restatement(esc, r, res):
    ec.check_directions(res)
    cube = el.random_cube(res)
    r.set_environment(cube)
    assert r.environment_res == res
    want = el.env_ref(cube, ec.DIRECTIONS)
    for n in (0, 1, 63, 64, 65, 257, 4099, len(ec.DIRECTIONS)):
        got = r.environment(ec.DIRECTIONS[:n])
        assert got["rgb"].shape == (n, 3) and got["rgb8"].shape == (n, 3)
        assert_same(got["rgb"], want[:n], f"R = {res}, n = {n}")
        assert np.array_equal(got["rgb8"], ol.oracle_quantise(want[:n]))
    assert_same(esc.environment_lookup_host(cube, ec.DIRECTIONS), got["rgb"], "host build of the same code")
    r.set_environment(None)


@pytest.mark.gpu
def test_lookup_kernel_outputs_are_optional_one_at_a_time(esc, r):
    import torch
    cube = el.random_cube(8)
    r.set_environment(cube)
    dev = torch.device("cuda", r.device)
    n = 1000
    d = torch.from_numpy(ec.DIRECTIONS[:n].copy()).to(dev)
    rgb = torch.full((n + 1, 3), -7.0, device=dev)
    u8 = torch.full((n + 1, 3), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    r.environment_rays(d, rgb[:n], None)
    r.environment_rays(d, None, u8[:n])
    r.synchronize()
    want = el.env_ref(cube, ec.DIRECTIONS[:n])
    assert_same(rgb[:n].cpu().numpy(), want, "rgb alone")
    assert np.array_equal(u8[:n].cpu().numpy(), ol.oracle_quantise(want))
    assert (rgb[n].cpu().numpy() == -7).all() and (u8[n].cpu().numpy() == 9).all()  # nothing past n
    with pytest.raises(esc.EscError) as e:
        r.environment_rays(d, None, None)
    assert e.value.code == -1 and "esc_environment_rays" in str(e.value)
    r.set_environment(None)


# ---- 2. trace cases ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,max_depth,bias,shadows", ec.TRACE_CASES)
def test_traces_against_the_oracle(esc, r, name, max_depth, bias, shadows):
    ec.check_trace_case(name)
    d, o, _ = ec.case_rays(name)
    bias = float(F32(bias))
    w = ec.want(name, max_depth, bias, shadows)
    assert w["usable"].all()  # every ray is compared
    r.upload(ol.scene_to_product(d))
    kw = dict(max_depth=max_depth, bias=bias, shadows=shadows, face_mode=esc.ESC_FACE_FIXED, seed=SEED,
              pixel_base=PIXEL_BASE)
    r.set_environment(None)
    r.trace(o, w["dirs"], **kw)
    plain = r.trace_stats()
    r.set_environment(ec.TRACE_CUBE)
    for exact in (False, True):
        got = r.trace(o, w["dirs"], exact=exact, **kw)
        st = r.trace_stats()
        assert st["depth_rays"] == w["depth_rays"], (st["depth_rays"], w["depth_rays"])
        assert_same(got["rgb"], w["rgb"], f"{name} depth {max_depth} exact {exact}")
        assert np.array_equal(got["rgb8"], ol.oracle_quantise(w["rgb"]))
        if not exact:  # the environment does not change which rays bounce
            for k in ("depth_rays", "rays", "hit_rays"):
                assert st[k] == plain[k], (k, st[k], plain[k])
            assert st["hit_rays"] >= w["hit_rays0"]
    r.set_environment(None)


# ---- 3. refraction -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [REFRACT, FRESNEL], ids=["refract", "fresnel"])
def test_refracted_rays_reach_the_environment(esc, r, mode):
    ec.check_glass_case(mode)
    d, o, _ = ec.case_rays("glass_open")
    bias = float(F32(ec.GLASS_BIAS))
    w = ec.want("glass_open", ec.GLASS_DEPTH, ec.GLASS_BIAS, True, mode)
    r.upload(product(d))
    kw = dict(max_depth=ec.GLASS_DEPTH, bias=bias, seed=SEED, pixel_base=PIXEL_BASE, transmission=MODE_NAME[mode])
    r.set_environment(None)
    black = r.trace(o, w["dirs"], **kw)
    plain, plain_t = r.trace_stats(), r.transmit_stats()
    r.set_environment(ec.TRACE_CUBE)
    for exact in (False, True):
        got = r.trace(o, w["dirs"], exact=exact, **kw)
        st = r.trace_stats()
        assert st["depth_rays"] == w["depth_rays"]
        assert r.transmit_stats() == stats_of(w) == plain_t
        assert_same(got["rgb"], w["rgb"], f"glass_open {MODE_NAME[mode]} exact {exact}")
        assert np.array_equal(got["rgb8"], ol.oracle_quantise(w["rgb"]))
        if not exact:
            for k in ("depth_rays", "rays", "hit_rays"):
                assert st[k] == plain[k], k
    assert (~same_bits(got["rgb"], black["rgb"])).any()
    r.set_environment(None)


# ---- 4. off is off -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand5", "cornell_mixed"])
def test_off_is_off(esc, name):
    d, o, _ = ec.case_rays(name)
    want = ec.want(name, 5, cube=None)
    assert np.isfinite(want["rgb"]).all()  # `w * 0` added to a finite C changes nothing: finite cases only
    rr = esc.Renderer(0)
    rr.upload(ol.scene_to_product(d))
    kw = dict(max_depth=5, bias=float(F32(1e-4)), seed=SEED, pixel_base=PIXEL_BASE)
    assert rr.environment_res == 0
    before = rr.trace(o, want["dirs"], **kw)
    rr.set_environment(ec.TRACE_CUBE)
    lit = rr.trace(o, want["dirs"], **kw)
    rr.set_environment(None)
    assert rr.environment_res == 0
    after = rr.trace(o, want["dirs"], **kw)
    assert before["rgb"].tobytes() == after["rgb"].tobytes() and before["rgb8"].tobytes() == after["rgb8"].tobytes()
    assert_same(before["rgb"], want["rgb"], f"{name} without an environment")
    assert (~same_bits(lit["rgb"], before["rgb"])).any()
    rr.set_environment(np.zeros((6, 4, 4, 3), F32))
    zero = rr.trace(o, want["dirs"], **kw)
    assert_same(zero["rgb"], want["rgb"], f"{name} with a cube of zeros")
    assert np.array_equal(zero["rgb8"], before["rgb8"])
    rr.close()


# ---- 5. depth 0 ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_depth_zero_is_shade_with_the_environment_on_the_misses(esc, r):
    r.upload(esc.Scene.synthetic("c4", 500))
    W, H = 192, 108
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    o, d = r.camera_rays(cam, W, H)
    r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
    o, d = o.cpu().numpy(), d.cpu().numpy()
    cube = el.random_cube(8, 3)
    r.set_environment(cube)
    for mode in (esc.ESC_FACE_FIXED, esc.ESC_FACE_HASH):
        want = r.shade(o, d, face_mode=mode, seed=9, pixel_base=5)["rgb"]
        q = r.intersect(o, d)
        miss = (q["geom"] < 0) & (q["prim"] < 0)
        assert miss.sum() * 10 >= len(o) and (~miss).sum() * 10 >= len(o), miss.sum()
        assert not want[miss].view(np.uint32).any()  # shade_rays is unchanged: black where nothing is hit
        env = r.environment(d)["rgb"]
        assert_same(env, el.env_ref(cube, d), "camera directions")
        want[miss] = env[miss]
        got = r.trace(o, d, max_depth=0, bias=0.25, face_mode=mode, seed=9, pixel_base=5)
        assert_same(got["rgb"], want, f"mode {mode}")
        assert np.array_equal(got["rgb8"], ol.oracle_quantise(want))
        assert r.trace_stats()["depth_rays"][0] == len(o)
    r.set_environment(None)


# ---- 6. a traced frame ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_traced_frame_is_composed_of_camera_rays_and_trace(esc, r):
    import torch
    dev = torch.device("cuda", r.device)
    d, _, _ = ec.case_rays("cornell_mixed")
    r.upload(ol.scene_to_product(d))
    r.set_environment(ec.TRACE_CUBE)
    W, H, spp, depth, bias, seed = 33, 19, 4, 2, float(F32(1e-4)), 21
    cam = esc.Camera.for_image((0, 1, 3.5), (0.4, 1.2, 0), W, H)
    img, u8 = r.render_traced(cam, W, H, spp=spp, max_depth=depth, bias=bias, seed=seed, want_u8=True,
                              face_mode=esc.ESC_FACE_HASH)
    st = r.trace_stats()
    assert st["depth_rays"][2] > 0 and st["hit_rays"] < st["rays"], st
    nn = 2
    acc = np.zeros((W * H, 3), F32)
    rays = 0
    for j in range(spp):  # render_supersampled's sample offsets, in fp32
        dx = F32(F32(F32(j % nn) + F32(0.5)) / F32(nn)) - F32(0.5)
        dy = F32(F32(F32(j // nn) + F32(0.5)) / F32(nn)) - F32(0.5)
        off = torch.from_numpy(np.tile(np.array([dx, dy], F32), (W * H, 1))).to(dev)
        torch.cuda.synchronize()
        o, dd = r.camera_rays(cam, W, H, offsets=off)
        r.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
        got = r.trace(o.cpu().numpy(), dd.cpu().numpy(), max_depth=depth, bias=bias, seed=seed + j,
                      face_mode=esc.ESC_FACE_HASH)
        acc = (acc + got["rgb"]).astype(F32)  # from zeros: 0.f + rgb at sample 0, as k_ss_accumulate does
        rays += r.trace_stats()["rays"]
    want = (acc / F32(spp)).astype(F32)
    assert_same(img.reshape(-1, 3), want, "spp 4, depth 2")
    assert np.array_equal(u8.reshape(-1, 3), ol.oracle_quantise(want))
    assert st["rays"] == rays
    r.set_environment(None)
    assert (~same_bits(r.render_traced(cam, W, H, spp=spp, max_depth=depth, bias=bias, seed=seed,
                                       face_mode=esc.ESC_FACE_HASH), img)).any()


# ---- 7. context state ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_context_state_and_arguments(esc):
    from esctp1raytracer_amd import _capi
    import ctypes as C
    rr = esc.Renderer(0)
    dirs = ec.DIRECTIONS[:513]
    assert rr.environment_res == 0
    with pytest.raises(esc.EscError) as e:  # no environment yet (and no scene is needed for the message)
        rr.environment(dirs)
    assert e.value.code == -1 and "esc_environment_rays" in str(e.value) and "environment" in str(e.value)
    a, b = el.random_cube(3, 7), el.random_cube(8, 8)
    rr.set_environment(a)  # no scene is needed
    assert rr.environment_res == 3
    assert_same(rr.environment(dirs)["rgb"], el.env_ref(a, dirs), "first cube, no scene")
    d, o, _ = ec.case_rays("cornell_mixed")
    rr.upload(ol.scene_to_product(d))
    assert rr.environment_res == 3
    assert_same(rr.environment(dirs)["rgb"], el.env_ref(a, dirs), "after an upload")
    rr.set_environment(b)
    assert rr.environment_res == 8
    assert_same(rr.environment(dirs)["rgb"], el.env_ref(b, dirs), "second cube")
    rr.upload(esc.Scene.synthetic("c4", 100))
    assert rr.environment_res == 8
    # invalid arguments leave the environment as it is
    lib, h = rr._lib, rr._h
    fp = b.ctypes.data_as(C.POINTER(C.c_float))
    for res, ptr in ((-1, fp), (1025, fp), (0, fp), (8, None), (1 << 30, fp)):
        assert lib.esc_set_environment(h, res, ptr) == _capi.ESC_ERR_INVALID, res
        assert "esc_set_environment" in lib.esc_last_error().decode()
    assert lib.esc_get_environment_res(h, None) == _capi.ESC_ERR_INVALID
    for shape in ((5, 8, 8, 3), (6, 8, 4, 3), (6, 8, 8, 4), (6, 8, 8)):
        with pytest.raises(ValueError):
            rr.set_environment(np.zeros(shape, F32))
    import torch
    dev = torch.device("cuda", rr.device)
    td = torch.from_numpy(dirs.copy()).to(dev)
    rgb = torch.empty((len(dirs), 3), device=dev)
    torch.cuda.synchronize()
    assert lib.esc_environment_rays(h, -1, C.c_void_p(td.data_ptr()), C.c_void_p(rgb.data_ptr()), None) == \
        _capi.ESC_ERR_INVALID
    assert lib.esc_environment_rays(h, 4, None, C.c_void_p(rgb.data_ptr()), None) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_rays(h, 4, C.c_void_p(td.data_ptr()), None, None) == _capi.ESC_ERR_INVALID
    assert lib.esc_environment_rays(h, 4, C.c_void_p(td.data_ptr() + 2), C.c_void_p(rgb.data_ptr()), None) == \
        _capi.ESC_ERR_INVALID
    assert lib.esc_environment_rays(h, 0, None, None, None) == _capi.ESC_OK  # n == 0 launches nothing
    with pytest.raises((TypeError, ValueError)):
        rr.environment_rays(td.double(), rgb)
    assert rr.environment_res == 8
    assert_same(rr.environment(dirs)["rgb"], el.env_ref(b, dirs), "after the rejected calls")
    rr.set_environment(None)
    assert rr.environment_res == 0
    with pytest.raises(esc.EscError):
        rr.environment(dirs)
    rr.set_environment(el.random_cube(1, 2))  # R = 1, and a renderer closed with an environment set
    assert rr.environment_res == 1
    rr.close()


# ---- 8. nothing else moves -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_else_moves(esc):
    d, _, _ = ec.case_rays("cornell_mixed")
    W, H = 96, 54
    cam = esc.Camera.for_image((0, 1, 3.5), (0.4, 1.2, 0), W, H)

    def everything(rr):
        out = {}
        rr.reset_counters()
        out["render"] = rr.render(cam, W, H, want_u8=True)
        out["counters"] = rr.counters()
        o, dd = rr.camera_rays(cam, W, H)
        rr.synchronize()  # the rays are written on the renderer's stream, .cpu() copies on torch's
        o, dd = o.cpu().numpy(), dd.cpu().numpy()
        out["shade"] = rr.shade(o, dd, face_mode=esc.ESC_FACE_HASH, seed=3)
        out["shade_stats"] = rr.shade_stats()
        out["intersect"] = rr.intersect(o, dd)
        out["query_stats"] = rr.query_stats()
        out["occluded"] = rr.occluded(o, dd, np.full(len(o), 2.0, F32))
        out["ambient"] = rr.ambient(o, dd, radius=0.5, seed=4)
        out["ambient_stats"] = rr.ambient_stats()
        out["supersampled"] = rr.render_supersampled(cam, W, H, 4, want_u8=True)
        out["adaptive"] = rr.render_adaptive(cam, W, H, 4, 0.05, want_u8=True)
        out["adaptive_stats"] = rr.adaptive_stats()
        return out

    def flat(v):
        if isinstance(v, dict):
            return b"".join(k.encode() + flat(x) for k, x in sorted(v.items()))
        if isinstance(v, (tuple, list)):
            return b"".join(flat(x) for x in v)
        return v.tobytes() if isinstance(v, np.ndarray) else repr(v).encode()

    results = []
    for cube in (None, ec.TRACE_CUBE):
        rr = esc.Renderer(0)
        rr.upload(ol.scene_to_product(d))
        rr.set_ambient_table(esc.ambient_table(4, 8, 1))
        if cube is not None:
            rr.set_environment(cube)
        results.append(everything(rr))
        rr.close()
    assert (results[0]["render"][0] == 0).all(axis=-1).any()  # black where nothing is hit, with or without
    for k in results[0]:
        assert flat(results[0][k]) == flat(results[1][k]), k


# ---- 9. the viewer -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_viewer_sky(esc, tmp_path):
    viewer = os.path.join(ROOT, "bin", "ESCViewer2021")
    obj = os.path.join(ROOT, "tests", "golden", "scenes", "two.obj")
    w, h = 40, 30
    sky = ((0.1, 0.3, 0.9), (0.8, 0.8, 0.7), (0.2, 0.15, 0.1))
    arg = "/".join(",".join(repr(c) for c in col) for col in sky)
    r = esc.Renderer(0)
    r.upload(esc.Scene.load_obj(obj))
    cam = esc.Camera.for_image((0, 1, 3), (0, 1, 0), w, h)
    # the viewer's defaults: eye (0, 1, 3), look (0, 1, 0), hashed faces with seed 0, bias 1e-4, a 64-texel cube
    for extra, depth, res in ((["--bounces", "2"], 2, 64), ([], 0, 64), (["--bounces", "2", "--sky-res", "5"], 2, 5)):
        ppm = tmp_path / f"sky{depth}_{res}.ppm"
        p = subprocess.run([viewer, "-m", obj, "-w", f"{w},{h}", "--sky", arg, *extra, "-o", str(ppm)],
                           capture_output=True, text=True, timeout=300, cwd=os.path.dirname(obj))
        assert p.returncode == 0, p.stderr
        r.set_environment(esc.environment_sky(res, *sky))
        img = r.render_traced(cam, w, h, spp=1, max_depth=depth, bias=1e-4, face_mode=esc.ESC_FACE_HASH, seed=0)
        mine = tmp_path / "mine.ppm"
        esc.write_ppm(mine, img)
        assert ppm.read_bytes() == mine.read_bytes(), extra
    r.set_environment(None)
    plain = tmp_path / "plain.ppm"
    esc.write_ppm(plain, r.render_traced(cam, w, h, spp=1, max_depth=2, bias=1e-4, face_mode=esc.ESC_FACE_HASH, seed=0))
    assert ppm.read_bytes() != plain.read_bytes()  # the sky is in the picture
    r.close()
