"""The CPU restatement of sky lighting (include/esctp1_rt.h at esc_skylight_rays), steps 8 and 9, built on what
ambient_lib.ambient already returns (the hit, which rays have one, the sample directions and which of them
are occluded) and on environment_lib.env_ref: numpy fp32 with one rounding per operation.  No ray is traced
here, no scenes and no pytest; tests/skylight_cases.py chooses cubes with it.

The sum over the open samples runs in sample order, k ascending, as the definition says.  descending=True
runs it the other way round: the tests use it only to show that the order matters to the bits."""
import numpy as np

from environment_lib import env_ref
from ray_oracle import F32


def material_kd(d, geom, prim):
    """kd (material floats 3..5) of every hit: a triangle's from its geometry, a sphere's from its own
    material; rows of rays without a hit are zero"""
    kd = np.zeros((len(geom), 3), F32)
    for i, (g, p) in enumerate(zip(geom.tolist(), prim.tolist())):
        if g >= 0:
            kd[i] = d["geometry"][g]["material"][3:6]
        elif p >= 0:
            kd[i] = d["sphere_materials"][p][3:6]
    return kd


def skylight(d, w, cube, K, descending=False):
    """w: ambient_lib.ambient's dict for the rays, K its samples per ray.  -> {"sky", "light", "kd", "env",
    "open"}: sky and light (n, 3) float32 for every ray (zero for a miss), and for the rays WITH a hit, in
    ray order, env (n_hit, K, 3) = env(w_k) and open (n_hit, K)"""
    has = w["has"]
    n, nh = len(has), int(has.sum())
    e = env_ref(cube, w["sample_d"]).reshape(nh, K, 3)
    open_ = (w["sample_occ"].reshape(nh, K) == 0)
    s = np.zeros((nh, 3), F32)
    with np.errstate(all="ignore"):
        for k in (range(K - 1, -1, -1) if descending else range(K)):
            s = np.where(open_[:, k, None], (s + e[:, k]).astype(F32), s)
        sky = np.zeros((n, 3), F32)
        sky[has] = (s / F32(K)).astype(F32)
        kd = material_kd(d, w["geom"], w["prim"])
        light = np.zeros((n, 3), F32)
        light[has] = (kd[has] * sky[has]).astype(F32)
    return {"sky": sky, "light": light, "kd": kd, "env": e, "open": open_}
