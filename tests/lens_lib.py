"""The thin-lens rule of include/esctp1_rt.h (at esc_lens_options) in numpy fp32, one rounding
per written operation: the yardstick of esc_lens_rays and, composed with Renderer.trace, of esc_render_lens.
No scenes and no pytest here; tests/lens_cases.py chooses the cases with it.

    is = (float(w) + dx) / float(W-1);   it = (float(h) + dy) / float(H-1)
    p  = ((llc + horizontal*is) + vertical*it) - origin
    aperture == 0:  o' = origin;  d' = normalize(p)
    else:           U = normalize(horizontal);  V = normalize(vertical)
                    set = mix_hi32(seed, q, 0xFFFFFFFD) mod S;   l = table[set][k]
                    off = U*(l.x*aperture) + V*(l.y*aperture)
                    o' = origin + off;   d' = normalize(p*focus_dist - off)

Every array below is float32 and every binary operation has two float32 operands, so numpy rounds once per
operation, as the kernel does (no contraction)."""
import numpy as np

from ray_oracle import F32, mix_hi32, normalize

LENS_LIGHT = 0xFFFFFFFD  # the hash's light index of the lens set


def _v(vectors, key):
    return np.ascontiguousarray(vectors[key], F32).reshape(3)


def _scaled(v, s):
    """vector x scalar, vec.h:127: v (3,) or (n, 3) float32 by s (n,) float32 -> (n, 3) float32"""
    return (v * s[:, None]).astype(F32)


def grid_offset(k, n):
    """esc_render_supersampled's sub-pixel offset of sample k of n*n, fp32 -> (dx, dy)"""
    n_ = F32(n)
    dx = F32(F32(F32(k % n) + F32(0.5)) / n_) - F32(0.5)
    dy = F32(F32(F32(k // n) + F32(0.5)) / n_) - F32(0.5)
    return F32(dx), F32(dy)


def pinhole_points(vectors, W, H, pix, offsets=None):
    """p of the rule for the pixels `pix` (ids h*W + w).  offsets: None, a pair (dx, dy) or an (n, 2) array"""
    pix = np.asarray(pix, np.int64)
    n = len(pix)
    if offsets is None:
        off = np.zeros((n, 2), F32)
    else:
        off = np.broadcast_to(np.asarray(offsets, F32), (n, 2))
    w, h = (pix % W).astype(F32), (pix // W).astype(F32)
    s = ((w + off[:, 0]).astype(F32) / F32(W - 1)).astype(F32)
    t = ((h + off[:, 1]).astype(F32) / F32(H - 1)).astype(F32)
    a = (_v(vectors, "lower_left_corner") + _scaled(_v(vectors, "horizontal"), s)).astype(F32)
    b = (a + _scaled(_v(vectors, "vertical"), t)).astype(F32)
    return (b - _v(vectors, "origin")).astype(F32)


def lens_sets(seed, pix, S):
    """the table's set of every pixel"""
    return (mix_hi32(int(seed), np.asarray(pix, np.int64).astype(np.uint32), LENS_LIGHT) % np.uint32(S)).astype(np.int64)


def lens_rays(vectors, W, H, pix, aperture, focus_dist, table=None, k=0, seed=0, offsets=None):
    """-> (origins, dirs), (n, 3) float32 each, for the pixels `pix`.  vectors: Camera.vectors().  table:
    (S, K, 2) float32, unused (and may be None) when aperture == 0"""
    origin = _v(vectors, "origin")
    p = pinhole_points(vectors, W, H, pix, offsets)
    n = len(p)
    ap, fd = F32(aperture), F32(focus_dist)
    with np.errstate(all="ignore"):
        if ap == 0:
            return np.tile(origin, (n, 1)).astype(F32), normalize(p)
        table = np.ascontiguousarray(table, F32)
        U, V = normalize(_v(vectors, "horizontal")), normalize(_v(vectors, "vertical"))
        l = table[lens_sets(seed, pix, table.shape[0]), int(k)]
        off = (_scaled(U, (l[:, 0] * ap).astype(F32)) + _scaled(V, (l[:, 1] * ap).astype(F32))).astype(F32)
        o = (origin + off).astype(F32)
        d = normalize(((p * fd).astype(F32) - off).astype(F32))
    return np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
