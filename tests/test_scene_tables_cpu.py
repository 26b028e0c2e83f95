"""The per-scene tables of an upload (esctp1raytracer_amd/host/scene_tables.cpp), no GPU needed.

Every table `Scene.table` returns -- the staged records, the eighteen computed tables and the header
-- is pinned by its sha256 in tests/golden/scene_table_pins.json for scenes that take every branch of
the host code at its smallest size.  The digests were taken from the statements of commit() in
rt_capi.cpp as they stood BEFORE they moved into scene_tables.cpp (that function compiled with each
vector handed out instead of uploaded), so the test says: the move changed no byte.  Byte equality, no
tolerance.  tests/test_filter_bounds.py checks the same tables against its numpy restatements.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import esctp1raytracer_amd as esc
import oracle_lib as ol
import ray_cases as rc
from esctp1raytracer_amd._capi import ESC_TABLE_NAMES

F32 = np.float32
PINS = os.path.join(ol.GOLDEN_DIR, "scene_table_pins.json")


def _matte(n):
    return np.tile(ol.material13(ka=(0, 0, 0), kd=(0.5, 0.5, 0.5)), (n, 1))


def _spheres(n, seed):
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.uniform(-4, 4, (n, 3)), rng.uniform(0.05, 0.6, (n, 1))], axis=1).astype(F32)
    return s


def _empty():
    return esc.Scene()


def _spheres_overflowing():
    """Scene.add_spheres rejects a non-finite centre or radius, so the km = NaN -> +inf rule is entered
    the way a caller can: a finite radius whose square is +inf in fp32 makes the scene box infinite,
    g = NaN, and every km of the plain, sorted and group forms NaN; a centre at 3e38 overflows c - g"""
    s = _spheres(70, 3)
    s[17, 3] = 1e20
    s[40, :3] = (3e38, -3e38, 3e38)
    sc = esc.Scene()
    sc.add_spheres(s, _matte(70))
    return sc


def _spheres_huge_centre():
    """the same 70 spheres with only the far centre: g and rho_max stay finite, |c'|^2 is ~1e77"""
    s = _spheres(70, 3)
    s[40, :3] = (3e38, -3e38, 3e38)
    sc = esc.Scene()
    sc.add_spheres(s, _matte(70))
    return sc


def _degenerate_triangle():
    """70 triangles, one with e1 = 0 (no normal: g'' = 0, its group is `always`) and one that is a point
    (e1 = e2 = 0: the pre-filter's sliver path, the only way there with finite corners)"""
    rng = np.random.default_rng(5)
    v = rng.uniform(-3, 3, (70, 3, 3)).astype(F32)
    v[:, 1:] = v[:, :1] + rng.uniform(-0.4, 0.4, (70, 2, 3)).astype(F32)
    v[33, 1] = v[33, 0]
    v[50, 1] = v[50, 2] = v[50, 0]
    sc = esc.Scene()
    sc.add_geometry(v.reshape(-1, 3), np.arange(210, dtype=np.uint32).reshape(-1, 3),
                    ol.material13(ka=(0, 0, 0), kd=(0.5, 0.5, 0.5)))
    return sc


def _normals_and_transmission():
    """`two` (two lights, one geometry with vertex normals) under two sheets of water and a glass sphere"""
    d = ol.load_dump("two")
    d["transmission"], d["sphere_transmission"] = {}, {}
    rc.add_sheet(d, 1.2, (0.9, 0.8, 0.7, 0.75), 1)
    rc.add_sheet(d, 0.8, (0.6, 0.9, 0.0, 1.33), 2)
    d["spheres"] = np.array([[0.35, 1.05, 0.4, 0.35]], F32)
    d["sphere_materials"] = rc.glass()[None].copy()
    d["sphere_transmission"][0] = np.array([0.9, 0.7, 0.0, 1.5], F32)
    return rc.product(d)


SCENES = {
    "c2_63": lambda: esc.Scene.synthetic("c2", 63),    # below kSphGroupMinSpheres; odd: a pad half
    "c2_64": lambda: esc.Scene.synthetic("c2", 64),    # groups on, one hyper-group padded to the step
    "c2_65": lambda: esc.Scene.synthetic("c2", 65),    # ... a pad group and a pad half
    "c3_257": lambda: esc.Scene.synthetic("c3", 257),  # the last light's sweep order (>= 256), odd
    "c3_600": lambda: esc.Scene.synthetic("c3", 600),  # more than one hyper-group (512 spheres each)
    "c5_5": lambda: esc.Scene.synthetic("c5", 5),      # 51 triangles: no triangle groups
    "c5_6": lambda: esc.Scene.synthetic("c5", 6),      # 73 triangles: groups on, odd count
    "c5_40": lambda: esc.Scene.synthetic("c5", 40),    # 3,201 triangles: several super- / hyper-groups
    "empty": _empty,                                   # no primitives, no lights: empty box, g = 0
    "spheres_overflowing": _spheres_overflowing,
    "spheres_huge_centre": _spheres_huge_centre,
    "degenerate_triangle": _degenerate_triangle,
    "normals_and_transmission": _normals_and_transmission,
}


def digests(scene):
    return {name: hashlib.sha256(scene.table(name).tobytes()).hexdigest() for name in ESC_TABLE_NAMES}


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def test_every_scene_is_pinned(pins):
    assert set(pins) == set(SCENES)
    for name, p in pins.items():
        assert set(p) == set(ESC_TABLE_NAMES), name


@pytest.mark.parametrize("name", list(SCENES))
def test_tables_are_the_pinned_bytes(name, pins):
    got = digests(SCENES[name]())
    wrong = [t for t in ESC_TABLE_NAMES if got[t] != pins[name][t]]
    assert not wrong, f"{name}: {wrong} differ from the pinned bytes"


def _header(scene):
    h = scene.table("header")
    assert h.size == 72
    return h[:40].view(F32), h[40:].view(np.int32)


def test_the_scenes_take_the_branches_they_are_chosen_for():
    """sizes and header fields: what each scene is in the list for actually happens"""
    def size(sc, t):
        return sc.table(t).size
    sc = SCENES["c2_63"]()
    assert sc.info()["n_spheres"] == 63 and size(sc, "sph2") == 32 * 32 and size(sc, "sg_sorted") == 0
    assert list(_header(sc)[1][:6]) == [0] * 6 and size(sc, "sph2_ord") == 0
    assert sc.table("sph2").view(F32).reshape(-1, 4, 2)[-1, 3, 1] == -np.inf  # the pad half
    for n in (64, 65):
        sc = SCENES[f"c2_{n}"]()
        assert list(_header(sc)[1][:3]) == [512, 64, 8]  # one real hyper-group, padded to kSphGroupStep
        assert size(sc, "sg_sorted") == 4096 * 16 and size(sc, "sg_grp") == 584 * 16
        assert size(sc, "sg_grp2_f") == 292 * 32 and size(sc, "sg_orig") == 1024 * 16
        grp = sc.table("sg_grp").view(F32).reshape(-1, 4)
        assert (grp[:512, 3] >= 0).sum() == (n + 7) // 8 and (grp[512:576, 3] >= 0).sum() == (n + 63) // 64
    sc = SCENES["c3_257"]()
    assert size(sc, "sph2_ord") == size(sc, "sph2") == 129 * 32 and size(sc, "sph2_f_ord") == 129 * 32
    assert (SCENES["c3_600"]().table("sg_grp").view(F32).reshape(-1, 4)[512 + 64:, 3] >= 0).sum() == 2
    sc = SCENES["c5_5"]()
    assert sc.info()["n_triangles"] == 51 and size(sc, "tg_sorted") == 0 and size(sc, "tri2_f") == 26 * 128
    sc = SCENES["c5_6"]()
    assert sc.info()["n_triangles"] == 73 and list(_header(sc)[1][3:6]) == [512, 32, 4]
    assert size(sc, "tg_sorted") == 4096 * 48 and size(sc, "tg_grp2_pf") == 274 * 64
    sc = SCENES["c5_40"]()
    assert sc.info()["n_triangles"] == 3201
    grp = sc.table("tg_grp").view(F32).reshape(-1, 16)
    assert (grp[512:544, 3] >= 0).sum() == 26 and (grp[544:, 3] >= 0).sum() == 4
    f, i = _header(SCENES["empty"]())
    assert not f.any() and not i.any() and all(size(SCENES["empty"](), t) == 0 for t in ESC_TABLE_NAMES[:-1])
    sc = SCENES["spheres_overflowing"]()
    assert np.isnan(_header(sc)[0][:3]).all()
    for t in ("sph2_f", "sg_sorted2_f"):
        km = sc.table(t).view(F32).reshape(-1, 4, 2)[:, 3].ravel()
        assert (km == np.inf).sum() == 70 and (km == -np.inf).sum() == km.size - 70  # real: always; pads: never
    km = sc.table("sg_grp2_f").view(F32).reshape(-1, 4, 2)[:, 3].ravel()
    assert (km == np.inf).sum() == 9 + 2 + 1 and not np.isnan(km).any()
    sc = SCENES["degenerate_triangle"]()
    pf = sc.table("tri2_pf").view(F32).reshape(-1, 8, 2)
    assert np.isfinite(pf[16, 3, 1]) and not pf[16, 4:7, 1].any()  # triangle 33: a sphere, no normal
    assert pf[25, 3, 0] == np.inf and not pf[25, :3, 0].any() and not pf[25, 4:7, 0].any()  # 50: the sliver record
    order = sc.table("tg_orig").view(np.int32)
    for k in (33, 50):  # their groups are `always`
        assert sc.table("tg_grp").view(F32).reshape(-1, 16)[int(np.flatnonzero(order == k)[0]) // 8, 11] != 0
    sc = SCENES["normals_and_transmission"]()
    assert size(sc, "tri_n") == sc.info()["n_triangles"] * 36 and sc.table("tri_n").any()
    f, i = _header(sc)
    assert i[6] == 1 and i[7] >= 1 and sc.info()["n_lights"] == 2
    assert size(sc, "transmit") == (sc.info()["n_geometry"] + 1) * 16


def test_table_rejects_bad_arguments():
    sc = SCENES["c2_63"]()
    lib = sc._lib
    assert lib.esc_scene_table(sc._h, len(ESC_TABLE_NAMES), None, 0) < 0
    assert lib.esc_scene_table(sc._h, -1, None, 0) < 0
    assert lib.esc_scene_table(None, 0, None, 0) < 0
    out = np.full(8, 7, np.uint8)  # too small: the size comes back, nothing is written
    assert lib.esc_scene_table(sc._h, 2, out.ctypes.data, out.size) == 63 * 16 and (out == 7).all()
    with pytest.raises(ValueError):
        sc.table("no_such_table")
