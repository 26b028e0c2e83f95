"""CPU only: the fixtures of test_light_list_packed.py are not vacuous.

The packed cells of the sphere light lists (csrc/rt_lists.h k_pack_light_cells) keep, per cell, only the halves
of its stored pair records whose own rectangle holds the cell.  From the rule restated per half
(light_list_packed_rule.HalfRects):

 * in far_apart_scene the packing has something to drop: a stored (cell, record) entry has two half slots, and
   fewer than 0.6 of them hold the cell (every entry keeps at least one half, so "0.6 halves per entry" can only
   be meant per half slot: kept / (2 entries) < 0.6);
 * in overlapping_scene more than half of the entries keep both halves;
 * every scene of the GPU test has shadowed pixels in some view, so its frames do run the shadow sweep's accepts.
"""
import pytest

import light_list_cases as lc
import light_list_packed_rule as pr


def test_far_apart_has_something_to_drop():
    entries, kept, both = pr.HalfRects(lc.far_apart_scene()).figures()
    print(f"far apart: {entries} entries, {kept} kept halves, {both} entries keep both")
    assert entries > 100
    assert kept / (2 * entries) < 0.6, (entries, kept)


def test_overlapping_keeps_both_halves():
    entries, kept, both = pr.HalfRects(lc.overlapping_scene()).figures()
    print(f"overlapping: {entries} entries, {kept} kept halves, {both} entries keep both")
    assert entries > 100
    assert both > 0.5 * entries, (entries, both)
    assert kept == entries + both


CASES = pr.packed_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_scene_has_shadowed_pixels(name):
    d, views, size, faces, _, _ = CASES[name]
    for face in faces:
        n = 0
        for v in views:
            n += pr.shadowed_pixels(d, v, size, fixed_face=face)
            if n:
                break
        assert n > 0, f"{name}, face {face}: no view has a shadowed pixel"
