"""The CPU restatement of the G-buffer and of the edge-stopping a-trous filter (include/esctp1_rt.h at
esc_gbuffer_rays and esc_filter_options) that the tests compare the GPU with: numpy fp32 with one rounding per
operation (.astype(F32) after every one), built on ray_oracle.py's pieces.  No scenes and no pytest here;
tests/filter_cases.py chooses cases with it.

Nothing here is transcendental: + - * / and compares, so images are compared bit for bit and counts exactly.
descending=True sums the taps in the opposite order: the tests use it only to show that the order matters to
the bits."""
import numpy as np

from ray_oracle import F32, dot, normals_and_ks, ref_queries
from skylight_lib import material_kd

K1 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F32)
STOPS = ("missing", "object", "normal", "plane")


def gbuffer(d, o, dirs):
    """-> {"normal", "position", "albedo" (n, 3) float32, "t", "geom", "prim", "has"}: the definition for every
    ray; a miss has zeros, t = FLT_MAX and geom = prim = -1"""
    o = np.ascontiguousarray(o, F32)
    dirs = np.ascontiguousarray(dirs, F32)
    with np.errstate(all="ignore"):
        hit, _ = ref_queries(d, o, dirs)
        N, _, has = normals_and_ks(d, hit, o, dirs)
        P = (o + (dirs * hit["t"][:, None]).astype(F32)).astype(F32)
    P[~has] = 0
    N = np.ascontiguousarray(N, F32)
    N[~has] = 0
    return {"normal": N, "position": P, "albedo": material_kd(d, hit["geom"], hit["prim"]), "t": hit["t"],
            "geom": hit["geom"], "prim": hit["prim"], "has": has}


def atrous(image, guides, iterations, normal_cos, plane_dist, same_object=True, descending=False):
    """-> (out, stats): out has image's shape ((H, W) or (H, W, C)); stats holds pixels, hit_pixels, taps_tested,
    taps_accepted and, per stop of STOPS, how many tested taps it was the first to reject.  guides: "normal",
    "position" (H*W*3 values each), "geom", "prim" (H*W each), in any shape."""
    img = np.ascontiguousarray(image, F32)
    H, W = img.shape[:2]
    I = img.reshape(H, W, -1).copy()
    N = np.ascontiguousarray(guides["normal"], F32).reshape(H, W, 3)
    P = np.ascontiguousarray(guides["position"], F32).reshape(H, W, 3)
    G = np.asarray(guides["geom"], np.int32).reshape(H, W)
    R = np.asarray(guides["prim"], np.int32).reshape(H, W)
    nc, pd = F32(normal_cos), F32(plane_dist)
    hit = (G >= 0) | (R >= 0)
    hh, ww = np.mgrid[0:H, 0:W]
    order = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
    if descending:
        order.reverse()
    st = {"pixels": H * W, "hit_pixels": int(hit.sum()), "taps_tested": 0, "taps_accepted": 0}
    st.update({k: 0 for k in STOPS})
    with np.errstate(all="ignore"):
        for i in range(int(iterations)):
            s = 1 << i
            acc = np.zeros(I.shape, F32)
            ws = np.zeros((H, W), F32)
            for dy, dx in order:
                qh, qw = hh + dy * s, ww + dx * s
                take = hit & (qh >= 0) & (qh < H) & (qw >= 0) & (qw < W)
                qh, qw = np.clip(qh, 0, H - 1), np.clip(qw, 0, W - 1)
                if (dy, dx) != (0, 0):
                    st["taps_tested"] += int(take.sum())
                    checks = [("missing", hit[qh, qw])]
                    if same_object:
                        checks.append(("object", (G[qh, qw] == G) & ((G >= 0) | (R[qh, qw] == R))))
                    checks.append(("normal", dot(N, N[qh, qw]) >= nc))
                    checks.append(("plane", np.abs(dot((P[qh, qw] - P).astype(F32), N)) <= pd))
                    for name, ok in checks:
                        st[name] += int((take & ~ok).sum())
                        take = take & ok
                    st["taps_accepted"] += int(take.sum())
                k = F32(K1[dx + 2] * K1[dy + 2])
                acc = np.where(take[..., None], (acc + (k * I[qh, qw]).astype(F32)).astype(F32), acc)
                ws = np.where(take, (ws + k).astype(F32), ws)
            I = np.where(hit[..., None], (acc / ws[..., None]).astype(F32), I)
    return np.ascontiguousarray(I.reshape(img.shape), F32), st
