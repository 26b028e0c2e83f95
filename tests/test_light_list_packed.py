"""GPU: the packed cells of the sphere light lists (csrc/rt_lists.h k_pack_light_cells, anyhit_sph_light_lists).

The shadow sweep reads, per cell of a light's cube map, only the spheres -- halves of the cell's stored pair
records -- whose own rectangle holds the cell, four per step, instead of the cell's pair records in batches of
four.  Per case (light_list_packed_rule.packed_cases: the slab and corner scenes of test_light_list_pairs.py, a pad
half, a cell and a face list over their caps, a sphere around P, spheres cut by face planes, two and five lights,
ESC_FACE_FIXED faces 0 and 1, one room):

 * frames: packed == id lists (ESC_RENDER_NO_PACKED_LIGHT_LISTS) == group sweep (ESC_RENDER_NO_LIGHT_LISTS) ==
   oracle, bit for bit, per view, as one kernel and with ESC_RENDER_TWO_KERNELS;
 * the read-back (Renderer.light_lists_packed) against the id lists (Renderer.light_lists): every slot a real
   half of a record among the cell's stored ids, no sphere twice in a cell, pads only at the tail of the last
   step, slots <= 2 cnt, a cell over the cap marked unserved -- and every stored record keeps at least one half (a
   record is appended only where a half's rectangle holds the cell);
 * membership, the direction that matters: every sphere a served reference shadow ray needs (light_list_cases
   shadow_rays / needed, as test_light_list_members.py uses them) is among the packed slots of its cell -- of
   both cells when it lies within 2^-12 cells of a border -- or its record is on the face's own list.  Served:
   the ray starts in the scene box, its light has lists, its cell and face list are within their caps.  All rays
   of the first light start in the box; of every later light at least a quarter do;
 * the packed path ran: with counters on, anyhit_tests with packing <= that of the id lists, and strictly below
   it on the far-apart scene.
"""
import numpy as np
import pytest

import light_list_cases as lc
import light_list_packed_rule as pr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD_SLOT = (2 ** 31 - 1) // 2  # what sg_orig holds for a pad slot
CASES = pr.packed_cases()


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


def check_structure(what, pk, ll, rec):
    """the packed read-back against the id lists -> (slots [n, cells, 2 cap], steps [n, cells])"""
    n, R, cap = ll["n_listed"], ll["R"], ll["cap"]
    assert pk["n_listed"] == n and pk["R"] == R and pk["per_step"] == 4, what
    cells = 6 * R * R
    ids = ll["ids"].reshape(n, cells, cap)
    cnt = ll["counts"].reshape(n, cells)
    steps = pk["steps"].reshape(n, cells)
    slots = pk["slots"].reshape(n, cells, -1)
    assert slots.shape[2] == 2 * cap
    over = cnt > cap
    assert np.array_equal(steps < 0, over), f"{what}: cells over the cap against cells marked unserved"
    assert int(steps[~over].sum()) == pk["total_steps"], f"{what}: the cells' steps against the stream's length"
    valid = slots >= 0
    k = valid.sum(axis=2)
    assert not k[over].any(), f"{what}: an unserved cell has slots"
    assert not (np.diff(valid.astype(np.int8), axis=2) > 0).any(), f"{what}: a slot after a pad"
    st = np.maximum(steps, 0)
    assert (k <= 4 * st).all() and (k > 4 * (st - 1))[st > 0].all(), f"{what}: pads elsewhere than the tail of the last step"
    assert (k <= 2 * np.minimum(cnt, cap)).all(), f"{what}: more slots than twice the stored records"
    assert int(slots.max(initial=-1)) < 2 * len(rec), f"{what}: a slot is no position of the sorted table"
    li, cell, q = np.nonzero(valid)
    pos = slots[li, cell, q]
    assert (rec[pos >> 1, 3, pos & 1] >= 0).all(), f"{what}: a slot holds a pad half"
    srt = np.sort(slots, axis=2)
    assert not ((np.diff(srt, axis=2) == 0) & (srt[:, :, 1:] >= 0)).any(), f"{what}: a sphere twice in a cell"
    # every slot's record is among the cell's stored ids, and every stored id keeps a half
    n_rec = len(rec)
    present = np.zeros((n, cells, n_rec), bool)
    a, b, c = np.nonzero(ids >= 0)
    present[a, b, ids[a, b, c]] = True
    assert present[li, cell, pos >> 1].all(), f"{what}: a slot's record is not among its cell's stored ids"
    kept = np.zeros((n, cells, n_rec), bool)
    kept[li, cell, pos >> 1] = True
    assert np.array_equal(kept[~over], present[~over]), f"{what}: a stored record keeps no half in its cell"
    return slots, steps


def run_case(esc, renderer, name, strict_fewer=False):
    d, views, (w, h), faces, key, over = CASES[name]
    sc = ol.scene_to_product(d)
    renderer.upload(sc)
    hdr = sc.table("header").view(F32)
    rec = sc.table("sg_sorted2").view(F32).reshape(-1, 4, 2)
    orig = sc.table("sg_orig").view(np.int32)
    slot_of = np.zeros(len(d["spheres"]), int)
    slot_of[orig[orig != PAD_SLOT]] = np.flatnonzero(orig != PAD_SLOT)
    nl = len(d["light_sources"])
    n_listed = min(nl, 4)
    for face in faces:
        tests = {"packed": 0, "ids": 0}
        inside, total = np.zeros(nl), np.zeros(nl)
        unserved_rays = 0
        read = None
        for vi, (eye, look) in enumerate(views):
            what = f"{name}/face {face}/view {vi}"
            cam = esc.Camera.for_image(eye, look, w, h)
            ref = ol.oracle_render(d, eye, look, w, h, threads=8, fixed_face=face)
            for two in (0, esc.ESC_RENDER_TWO_KERNELS):
                for mode, fl in (("packed", 0), ("ids", esc.ESC_RENDER_NO_PACKED_LIGHT_LISTS),
                                 ("sweep", esc.ESC_RENDER_NO_LIGHT_LISTS)):
                    renderer.reset_counters()
                    gpu = renderer.render(cam, w, h, fixed_face=face, flags=fl | two)
                    nb = int((bits(gpu) != bits(ref)).sum())
                    assert nb == 0, f"{what}/{mode}{'/two kernels' if two else ''}: {nb} fp32 values differ from the oracle's"
                    if not two and mode in tests:
                        tests[mode] += renderer.counters()["anyhit_tests"]
            if read is None:  # per scene and sample point: read once, after a default-path frame built them
                renderer.render(cam, w, h, fixed_face=face)
                pk, ll = renderer.light_lists_packed(), renderer.light_lists(2)
                assert pk is not None and ll is not None, f"{what}: no sphere light lists"
                P = lc.light_points(d)[ll["point"]]
                slots, steps = check_structure(what, pk, ll, rec)
                on_face = np.zeros((n_listed, 6, len(rec)), bool)
                a, f, c = np.nonzero(ll["face_ids"] >= 0)
                on_face[a, f, ll["face_ids"][a, f, c]] = True
                face_over = ll["face_counts"] > ll["global_cap"]
                read = True
                print(f"{name}/face {face}: {int(np.minimum(ll['counts'], ll['cap']).sum())} stored records, "
                      f"{int((slots >= 0).sum())} kept halves, {pk['total_steps']} steps, {int((steps < 0).sum())} cells "
                      f"over the cap, longest face list {int(ll['face_counts'].max())}")
            assert w == h == lc.W  # the frames lc.shadow_rays restates
            rays, nd = lc.members((key, vi, face), d, (eye, look), face)
            box = lc.in_box(hdr, rays["hitp"])
            inside += np.bincount(rays["light"], weights=box, minlength=nl)
            total += np.bincount(rays["light"], minlength=nl)
            for li in range(n_listed):
                assert np.array_equal(bits(P[li]), bits(rays["P"][li])), f"{what}: light {li}: lists for another point"
                sel = np.flatnonzero(box & (rays["light"] == li))
                if not len(sel):
                    continue
                fc, cells, _, _ = lc.cell_of(P[li], rays["hitp"][sel], 128)
                served = (steps[li][cells] >= 0).all(axis=1) & ~face_over[li, fc]
                unserved_rays += int((~served).sum())
                r, q = np.nonzero(nd["sph"][sel] & served[:, None])
                pos = slot_of[q]
                listed = on_face[li, fc[r], pos >> 1]
                for k in range(cells.shape[1]):
                    have = (slots[li][cells[r, k]] == pos[:, None]).any(axis=1)
                    bad = ~listed & ~have
                    assert not bad.any(), (f"{what}: light {li}: {int(bad.sum())} needed spheres are neither in their ray's "
                                           f"packed cell nor on its face list; first: original sphere {int(q[bad][0])}, "
                                           f"cell {int(cells[r, k][bad][0])}")
        if total.sum() > 0:
            share = inside / np.maximum(total, 1)
            assert share[0] == 1.0 and (share >= 0.25).all(), f"{name}: rays that start in the scene box, per light: {share}"
            if over is None:
                assert unserved_rays == 0, f"{name}: {unserved_rays} rays in the box are not served"
            else:
                assert unserved_rays > 0, f"{name}: no ray's {over} list is over its cap"
        print(f"{name}/face {face}: anyhit_tests packed {tests['packed']}, id lists {tests['ids']}")
        assert tests["packed"] <= tests["ids"], f"{name}: {tests}"
        if strict_fewer:
            assert tests["packed"] < tests["ids"], f"{name}: the packed sweep tested no less: {tests}"


@pytest.mark.parametrize("name", list(CASES))
def test_packed_cells(esc, renderer, name):
    run_case(esc, renderer, name, strict_fewer=name == "far apart")
