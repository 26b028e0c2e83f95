"""The CPU restatement of ambient occlusion (include/esctp1_rt.h at esc_ambient_options) that the tests
compare the GPU with: numpy fp32 with one rounding per operation, built on ray_oracle.py's pieces (the closest
hit / occlusion loop, the normal of main.cpp:723-738, vec.h's dot and normalize, the hash's mixer).  No scenes
and no pytest here; tests/ambient_cases.py chooses scenes and rays with it.

Nothing here is transcendental: + - * / and sqrt, which numpy rounds correctly in float32, so counts are
compared exactly and vis bit for bit.  NaN results compare as NaN."""
import numpy as np

from ray_oracle import F32, FLT_MAX, dot, mix_hi32, normalize, normals_and_ks, ref_queries

AMBIENT_LIGHT = 0xFFFFFFFE  # the hash's light index of the set draw


def frame(Nf):
    """step 4: the branch-free tangent frame about Nf -> (T, B); |sg + Nf.z| >= 1"""
    x, y, z = Nf[..., 0], Nf[..., 1], Nf[..., 2]
    one = F32(1)
    with np.errstate(all="ignore"):
        sg = np.copysign(one, z).astype(F32)
        a = (-one / (sg + z).astype(F32)).astype(F32)
        b = ((x * y).astype(F32) * a).astype(F32)
        T = np.stack([(one + ((sg * (x * x).astype(F32)).astype(F32) * a).astype(F32)).astype(F32),
                      (sg * b).astype(F32), -((sg * x).astype(F32))], axis=-1).astype(F32)
        B = np.stack([b, (sg + ((y * y).astype(F32) * a).astype(F32)).astype(F32), -y], axis=-1).astype(F32)
    return T, B


def hit_frames(d, o, dirs, bias):
    """steps 1-4 -> (hit, has, Nf, P, T, B): the closest hit, which rays have one, and for every ray (values
    of rays without a hit mean nothing) the flipped normal, the sample origin and the frame"""
    o = np.ascontiguousarray(o, F32)
    dirs = np.ascontiguousarray(dirs, F32)
    with np.errstate(all="ignore"):
        hit, _ = ref_queries(d, o, dirs)
        N, _, has = normals_and_ks(d, hit, o, dirs)
        sn = dot(dirs, N)
        Nf = np.where((sn > 0)[:, None], -N, N).astype(F32)
        P = ((o + (dirs * hit["t"][:, None]).astype(F32)).astype(F32) + (Nf * F32(bias)).astype(F32)).astype(F32)
    T, B = frame(Nf)
    return hit, has, Nf, P, T, B


def ambient(d, o, dirs, table, radius=FLT_MAX, bias=1e-4, seed=0, pixel_base=0):
    """-> {"count", "vis", "t", "geom", "prim", "has", "set", "sample_o", "sample_d", "sample_occ"}: the
    definition for every ray.  table: (S, K, 3) float32.  sample_o / sample_d / sample_occ: the K sample rays
    of every ray WITH a hit, in ray order then sample order ((n_hit * K, 3) and (n_hit * K,)): the rays
    esc_occluded_rays is asked about with tmax = radius."""
    table = np.ascontiguousarray(table, F32)
    S, K = table.shape[0], table.shape[1]
    n = len(o)
    hit, has, Nf, P, T, B = hit_frames(d, o, dirs, bias)
    q = ((int(pixel_base) + np.arange(n, dtype=np.int64)) % (1 << 32)).astype(np.uint32)
    sets = (mix_hi32(seed, q, AMBIENT_LIGHT) % np.uint32(S)).astype(np.int64)
    count = np.full(n, K, np.int32)
    idx = np.nonzero(has)[0]
    so = np.zeros((0, 3), F32)
    sd = np.zeros((0, 3), F32)
    occ = np.zeros(0, np.uint8)
    if len(idx):
        l = table[sets[idx]]  # (nh, K, 3)
        Th, Bh, Nh = T[idx][:, None, :], B[idx][:, None, :], Nf[idx][:, None, :]
        with np.errstate(all="ignore"):
            x = (((Th * l[..., 0:1]).astype(F32) + (Bh * l[..., 1:2]).astype(F32)).astype(F32) +
                 (Nh * l[..., 2:3]).astype(F32)).astype(F32)
            sd = normalize(x.reshape(-1, 3))
            so = np.ascontiguousarray(np.repeat(P[idx], K, axis=0), F32)
            _, occ = ref_queries(d, so, sd, np.full(len(so), F32(radius), F32))
        count[idx] = K - occ.reshape(-1, K).astype(np.int32).sum(1)
    vis = (count.astype(F32) / F32(K)).astype(F32)
    return {"count": count, "vis": vis, "t": hit["t"], "geom": hit["geom"], "prim": hit["prim"], "has": has,
            "set": sets, "sample_o": so, "sample_d": sd, "sample_occ": occ}
