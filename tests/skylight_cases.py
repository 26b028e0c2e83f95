"""Cubes and conditions of the sky-lighting tests.  The cases are those of tests/ambient_cases.py and the
visibility answer is ambient_cases.want, shared and cached: no ray is traced twice on the CPU.  What is new is
chosen here by the restatement of tests/skylight_lib.py alone, before anything runs on the GPU.

Three cubes: "random" (8 texels per side, values in [0, 2)), "ones" (every texel 1: sky == vis) and "faces"
(1 texel per side: one colour per face).  The conditions that make the comparison worth having:
  * ambient_cases.check_condition holds for the case;
  * in every case at least one hit ray's sky differs in some bit between ascending and descending summation,
    which pins the order;
  * over all cases together, the open samples fall on all six cube faces."""
import numpy as np

import ambient_cases as ac
import environment_lib as el
import skylight_lib as sl
from ray_oracle import F32

K = ac.TABLE_SAMPLES
CASES = ac.CASES
_CUBES, _WANT = {}, {}


def cube(name="random"):
    if name not in _CUBES:
        c = {"random": lambda: el.random_cube(8, 1), "ones": lambda: np.ones((6, 4, 4, 3), F32),
             "faces": lambda: el.random_cube(1, 2), "zeros": lambda: np.zeros((6, 2, 2, 3), F32)}[name]()
        c.setflags(write=False)
        _CUBES[name] = c
    return _CUBES[name]


def want(name, ray_set, k, cube_name="random", descending=False):
    """the restatement's sky lighting of a case (skylight_lib.skylight's dict), computed once"""
    key = (name, ray_set, k, cube_name, descending)
    if key not in _WANT:
        w = sl.skylight(ac.scene(name)[0], ac.want(name, ray_set, k), cube(cube_name), K, descending)
        for v in w.values():
            v.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def order_matters(name, ray_set, k):
    """how many hit rays' sky differs in some bit between ascending and descending summation"""
    a, b = want(name, ray_set, k)["sky"], want(name, ray_set, k, descending=True)["sky"]
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())


def check_condition(name, ray_set, k):
    ac.check_condition(name, ray_set, k)
    n = order_matters(name, ray_set, k)
    print(f"{name} {ray_set} setting {k}: the order of the sum shows in {n} rays' sky")
    assert n >= 1, (name, ray_set, k)


def open_faces():
    """over all cases: how many open samples look at each of the six faces"""
    faces = np.zeros(6, np.int64)
    for name, ray_set, k in CASES:
        w = ac.want(name, ray_set, k)
        parts = el.env_parts(cube(), w["sample_d"])
        sel = (w["sample_occ"] == 0) & parts["defined"]
        faces += np.bincount(parts["face"][sel], minlength=6)
    return faces
