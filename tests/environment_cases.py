"""The cases of the environment tests and the conditions they have to meet, all decided on the CPU by the
restatements (tests/environment_lib.py, tests/ray_oracle.py) before anything runs on the GPU.  The CPU test
asserts every condition; the GPU tests assert them again before they compare.

  - DIRECTIONS: the direction set of the lookup tests, about 20,000 directions in named classes;
  - TRACE_CASES: ray_cases.trace_case_rays' rays (Ns == 0 cases only: every bit is compared) traced with a
    random cube, R = 8, values in [0, 2);
  - "glass_open": glass spheres in the open under one light, for REFRACT and FRESNEL: refracted rays leave
    the scene (none does in the Cornell-box refraction cases)."""
import itertools

import numpy as np

import environment_lib as el
import oracle_lib as ol
import ray_cases as rc
from ray_cases import camera_targets, glass
from ray_oracle import F32, FRESNEL, OFF, REFRACT, oracle_trace, ray_colours

LOOKUP_RES = (1, 2, 3, 8, 64)
ODD_CLASSES = ("signs", "tie2", "tie3", "zeros", "huge", "tiny", "nan", "inf", "null")


def _directions():
    rng = np.random.default_rng(2024)
    parts = {"normal": rng.standard_normal((12000, 3))}
    parts["signs"] = np.array([v for v in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(v)])
    t2 = rng.standard_normal((2000, 3))  # |d[a]| == |d[b]| on a random pair of axes
    a = rng.integers(0, 3, 2000)
    t2[np.arange(2000), (a + 1) % 3] = t2[np.arange(2000), a] * rng.choice([-1.0, 1.0], 2000)
    parts["tie2"] = t2
    parts["tie3"] = rng.standard_normal((500, 1)) * rng.choice([-1.0, 1.0], (500, 3))
    z = rng.standard_normal((1500, 3))
    mask = rng.uniform(size=(1500, 3)) < 0.4
    mask[mask.all(axis=1), 0] = False
    z[mask] = 0.0
    z = np.where(mask & (rng.uniform(size=(1500, 3)) < 0.5), -0.0, z)
    parts["zeros"] = z
    with np.errstate(over="ignore"):
        scale = np.where(np.arange(1500) < 1000, F32(1e38), F32(3e38)).astype(F32)[:, None]  # 3e38: many overflow
        parts["huge"] = (rng.standard_normal((1500, 3)).astype(F32) * scale).astype(F32)
    parts["tiny"] = (rng.standard_normal((1500, 3)).astype(F32) * F32(1e-42)).astype(F32)  # subnormal
    nn = rng.standard_normal((120, 3))
    nn[np.arange(120), rng.integers(0, 3, 120)] = np.nan
    parts["nan"] = nn
    ii = rng.standard_normal((120, 3))
    ii[np.arange(120), rng.integers(0, 3, 120)] = rng.choice([-np.inf, np.inf], 120)
    ii[:10] = np.inf
    parts["inf"] = ii
    parts["null"] = np.array([v for v in itertools.product((-0.0, 0.0), repeat=3)] * 3)
    names, arrays = [], []
    for k, v in parts.items():
        names += [k] * len(v)
        arrays.append(np.ascontiguousarray(v, F32))
    dirs = np.concatenate(arrays)
    perm = rng.permutation(len(dirs))  # classes mixed within a wave
    return dirs[perm], np.array(names)[perm]


DIRECTIONS, DIRECTION_CLASS = _directions()


def check_directions(res, verbose=False):
    """the condition on the direction set for a cube of `res`: every face receives at least 10 % of the
    defined directions; for res <= 8 at least 5 % of the lookups are clamped at a face border; every odd
    class is present; u and v stay in [-1, 1], x in [-0.5, R - 0.5], fx in [0, 1]"""
    p = el.env_parts(el.random_cube(res), DIRECTIONS)
    ok = p["defined"]
    assert 19000 <= len(DIRECTIONS) <= 21000 and ok.sum() >= 15000
    share = np.bincount(p["face"][ok], minlength=6) / ok.sum()
    clamped = p["clamped"].sum() / ok.sum()
    if verbose:
        print(f"R = {res}: face shares {np.round(share, 3).tolist()}, clamped {clamped:.3f}, "
              f"undefined {int((~ok).sum())}")
    assert share.min() >= 0.10, share
    if res <= 8:
        assert clamped >= 0.05, clamped
    for name in ODD_CLASSES:
        assert (DIRECTION_CLASS == name).sum() >= 8, name
    for name in ("nan", "null"):
        assert not ok[DIRECTION_CLASS == name].any(), name
    assert (~ok[DIRECTION_CLASS == "inf"]).sum() >= 10 and (~ok[DIRECTION_CLASS == "huge"]).sum() >= 10
    assert ok[DIRECTION_CLASS == "tiny"].all() and ok[DIRECTION_CLASS == "huge"].sum() >= 900
    for k in ("u", "v"):
        assert np.abs(p[k][ok]).max() <= 1
    for k in ("x", "y"):
        assert p[k][ok].min() >= -0.5 and p[k][ok].max() <= res - 0.5
    for k, xk in (("fx", "x"), ("fy", "y")):  # f rounds to 1 only for x just under 0, where i0 == i1 == 0
        assert p[k][ok].min() >= 0 and p[k][ok].max() <= 1
        assert (p[xk][ok][p[k][ok] == 1] < 0).all()
    assert np.isfinite(p["rgb"]).all()
    return p


# ---- trace cases ---------------------------------------------------------------------------------------
TRACE_CUBE = el.random_cube(8, 1)
TRACE_NAMES = ("rand3", "rand5", "cornell_mixed", "mirror_floor_camera")
TRACE_SETTINGS = ((5, 1e-4, True), (2, 1e-4, True))
TRACE_CASES = [(n, *s) for n in TRACE_NAMES for s in TRACE_SETTINGS]
_WANT = {}


def want(name, max_depth, bias=1e-4, shadows=True, mode=OFF, cube=TRACE_CUBE, key="trace"):
    """oracle_trace of the case's rays: with the environment's rule (cube) or without (cube=None)"""
    k = (name, max_depth, bias, shadows, mode, key if cube is not None else None)
    if k not in _WANT:
        d, o, a = case_rays(name)
        _WANT[k] = oracle_trace(d, o, a, max_depth, float(F32(bias)), mode, shadows=shadows,
                                colours=el.env_colours(cube) if cube is not None else ray_colours)
    return _WANT[k]


def glass_open():
    """six glass spheres in the open under one light; the camera's rays are aimed at them"""
    light = {"vertex": np.array([(-0.5, 3, 0.5), (0.5, 3, 0.5), (0, 3, -0.5)], F32),
             "face_index": np.array([[0, 1, 2]]), "material": ol.LIGHT_A.copy()}
    sph = np.array([[x, y, 0.1 * x * y, 0.42] for y in (-0.5, 0.5) for x in (-1.0, 0.0, 1.0)], F32)
    d = ol.scene_dict([light], sph, np.stack([glass()] * len(sph)))
    d["transmission"] = {}
    d["sphere_transmission"] = {k: np.array([0.9, 0.8, 0.7 if k % 2 else 0.0, 1.5], F32) for k in range(len(sph))}
    o, a = camera_targets((0.2, 0.3, 3.0), (0, 0, 0), 16, 12)
    return d, o, a


GLASS_DEPTH, GLASS_BIAS = 5, 1e-4
_RAYS = {}


_PRIVATE, _CASES = {}, {}


def _shielded_trace_case_rays(name):
    """ray_cases.trace_case_rays built on copies of oracle_lib's shared material arrays.  random_scene puts
    ol.WHITE / ol.RED / ol.LIGHT_A themselves into its scenes and with_ks edits a scene's materials in place,
    so building rand3 changes those arrays for every later user in the process: scene_one's PPM pin, the
    pinned rand9, and rand5, whose patch then reflects.  `rand5` here is ray_cases.TRACE_CASES' sequence
    (rand3 built before rand5: 114 level-1 rays; built alone it has 14), reproduced on private copies that are
    swapped in for the build, so that oracle_lib's arrays and ray_cases' cache are left as they were found."""
    if name not in _CASES:
        if name == "rand5":
            _shielded_trace_case_rays("rand3")
        shared = {k: v for k, v in vars(ol).items() if isinstance(v, np.ndarray) and v.shape == (13,)}
        if not _PRIVATE:
            _PRIVATE.update({k: v.copy() for k, v in shared.items()})
        cache = dict(rc._TRACE_CACHE)
        try:
            rc._TRACE_CACHE.clear()
            for k in shared:
                setattr(ol, k, _PRIVATE[k])
            _CASES[name] = rc.trace_case_rays(name)
        finally:
            for k, v in shared.items():
                setattr(ol, k, v)
            rc._TRACE_CACHE.clear()
            rc._TRACE_CACHE.update(cache)
    return _CASES[name]


def case_rays(name):
    """-> (scene dict, origins, targets)"""
    if name != "glass_open":
        return _shielded_trace_case_rays(name)
    if name not in _RAYS:
        d, o, a = glass_open()
        keep = np.ones(len(o), bool)
        for mode in (REFRACT, FRESNEL):  # the hand-built camera reproduces every bounce direction
            keep &= oracle_trace(d, o, a, GLASS_DEPTH, float(F32(GLASS_BIAS)), mode)["usable"]
        _RAYS[name] = (d, o[keep], a[keep])
    return _RAYS[name]


def check_trace_case(name, verbose=False):
    """at least 10 misses at some level >= 1; for all but mirror_floor_camera (whose camera sees only the
    box) at least 10 % of the level-0 rays miss and at least 10 % hit"""
    d, o, _ = case_rays(name)
    w = want(name, 5)
    assert w["usable"].all()
    c = el.census(d, o, w["dirs"], 5, float(F32(1e-4)))
    if verbose:
        print(name, "misses of rays per level:", [f"{m} of {r}" for m, r in zip(c["misses"], c["rays"])])
    assert c["rays"] == [x for x in w["depth_rays"][:len(c["rays"])]], (c["rays"], w["depth_rays"])
    assert max(c["misses"][1:]) >= 10, c
    # and within depth 2, for the second setting
    assert max(c["misses"][1:3]) >= 10, c
    if name != "mirror_floor_camera":
        assert c["misses"][0] * 10 >= c["rays"][0] and (c["rays"][0] - c["misses"][0]) * 10 >= c["rays"][0], c
    return c


def check_glass_case(mode, verbose=False):
    """at least 10 rays that were refracted at least once reach the environment"""
    d, o, _ = case_rays("glass_open")
    w = want("glass_open", GLASS_DEPTH, GLASS_BIAS, True, mode)
    assert w["usable"].all() and len(o) >= 64
    c = el.census(d, o, w["dirs"], GLASS_DEPTH, float(F32(GLASS_BIAS)), mode)
    if verbose:
        print("glass_open mode", mode, c, {k: w[k] for k in ("refracted", "fresnel_reflected", "total_internal")})
    assert c["rays"] == w["depth_rays"][:len(c["rays"])], (c["rays"], w["depth_rays"])
    assert c["refracted_misses"] >= 10 and w["refracted"] >= 10, c
    if mode == FRESNEL:
        assert w["fresnel_reflected"] > 0
    return c
