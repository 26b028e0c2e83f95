"""The environment cube map restated on the CPU (include/esctp1_rt.h at esc_set_environment): the lookup
env(d) in numpy fp32 with one rounding per operation, the sky generator in float64, a `colours` callable for
ray_oracle.oracle_trace that gives the rays that miss the environment's colour, and a census of where the
rays of a trace end.  No scenes and no pytest here; tests/environment_cases.py chooses scenes and rays."""
import numpy as np

from ray_oracle import (F32, FLT_MAX, OFF, bounce, normalize, normals_and_ks, ray_colours, ref_queries,
                        transmission_rows)

HALF = F32(0.5)


def _axis(u, R):
    """x = ((u * 0.5 + 0.5) * R) - 0.5 -> (i0, i1, f, clamped)"""
    x = (((u * HALF).astype(F32) + HALF).astype(F32) * F32(R)).astype(F32)
    x = (x - HALF).astype(F32)
    x0 = np.floor(x).astype(F32)
    f = (x - x0).astype(F32)
    k = x0.astype(np.int64)
    return np.clip(k, 0, R - 1), np.clip(k + 1, 0, R - 1), f, (k < 0) | (k + 1 > R - 1), x


def env_parts(cube, dirs):
    """every intermediate of env(d): {"defined", "face", "u", "v", "x", "y", "fx", "fy", "clamped", "rgb"}"""
    t = np.ascontiguousarray(cube, F32)
    R = t.shape[1]
    assert t.shape == (6, R, R, 3)
    d = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    n = np.arange(len(d))
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        ax, ay, az = ad[:, 0], ad[:, 1], ad[:, 2]
        axis = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
        c, a, b = d[n, axis], d[n, (axis + 1) % 3], d[n, (axis + 2) % 3]
        m = np.abs(c)
        ok = ~np.isnan(d).any(axis=1) & (m > 0) & (m <= FLT_MAX)
        m1 = np.where(ok, m, F32(1))
        u = (np.where(ok, a, F32(0)) / m1).astype(F32)
        v = (np.where(ok, b, F32(0)) / m1).astype(F32)
        i0, i1, fx, cx, x = _axis(u, R)
        j0, j1, fy, cy, y = _axis(v, R)
        face = 2 * axis + (c < 0)
        fx, fy = fx[:, None], fy[:, None]
        t00, t01, t10, t11 = t[face, j0, i0], t[face, j0, i1], t[face, j1, i0], t[face, j1, i1]
        c0 = (t00 + ((t01 - t00).astype(F32) * fx).astype(F32)).astype(F32)
        c1 = (t10 + ((t11 - t10).astype(F32) * fx).astype(F32)).astype(F32)
        rgb = (c0 + ((c1 - c0).astype(F32) * fy).astype(F32)).astype(F32)
    rgb[~ok] = 0
    return {"defined": ok, "face": face, "u": u, "v": v, "x": x, "y": y, "fx": fx[:, 0], "fy": fy[:, 0],
            "clamped": ok & (cx | cy), "rgb": rgb}


def env_ref(cube, dirs):
    """env(d): (n, 3) float32"""
    return env_parts(cube, dirs)["rgb"]


def sky_ref(res, zenith, horizon, ground):
    """esc_environment_sky in float64, in the header's operation order, cast to float32 at the end"""
    R = int(res)
    z, h, g = (np.asarray(v, F32).astype(np.float64) for v in (zenith, horizon, ground))
    out = np.zeros((6, R, R, 3), F32)
    s = ((np.arange(R, dtype=np.float64) + 0.5) / float(R)) * 2.0 - 1.0
    for face in range(6):
        axis = face // 2
        D = np.zeros((R, R, 3))
        D[..., axis] = -1.0 if face & 1 else 1.0
        D[..., (axis + 1) % 3] = s[None, :]  # i
        D[..., (axis + 2) % 3] = s[:, None]  # j
        e = D[..., 1] / np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])
        e = e[..., None]
        out[face] = np.where(e >= 0, h + (z - h) * e, h + (g - h) * (-e)).astype(F32)
    return out


def random_cube(res, seed=0):
    """values in [0, 2): above 1 too, so that the quantisation's clamp takes part"""
    return np.random.default_rng(1000 + seed).uniform(0.0, 2.0, (6, res, res, 3)).astype(F32)


def env_colours(cube):
    """ray_colours with the rule of the bounce loop added: the colour of every ray that ref_queries reports
    as a miss (exactly 0 from orc_render, asserted) is env(the direction ray_colours returns)"""
    def colours(d, origins, llc, fixed_face=0, shadows=True, horizontal=(1, 0, 0)):
        dirs, rgb = ray_colours(d, origins, llc, fixed_face, shadows, horizontal)
        hit, _ = ref_queries(d, origins, dirs)
        miss = (hit["geom"] < 0) & (hit["prim"] < 0)
        assert not rgb[miss].view(np.uint32).any(), "a miss whose colour is not +0"
        rgb[miss] = env_ref(cube, dirs[miss])
        return dirs, rgb
    return colours


def census(d, o, dirs, max_depth, bias, mode=OFF, seed=77, pixel_base=1234):
    """where the rays of oracle_trace's loop end: per level k <= max_depth (rays, misses), and how many of
    the misses belong to a path that was refracted at least once.  -> {"rays", "misses", "refracted_misses"}"""
    n = len(o)
    idx = np.arange(n)
    co, cd, w = np.ascontiguousarray(o, F32), np.ascontiguousarray(dirs, F32), np.ones((n, 3), F32)
    refr = np.zeros(n, bool)
    rays, misses, rm = [], [], 0
    with np.errstate(all="ignore"):
        for k in range(max_depth + 1):
            hit, _ = ref_queries(d, co, cd)
            N, ks, has = normals_and_ks(d, hit, co, cd)
            rays.append(len(idx))
            misses.append(int((~has).sum()))
            rm += int((~has & refr).sum())
            if k == max_depth or len(idx) == 0:
                break
            q = ((pixel_base + idx) % (1 << 32)).astype(np.uint32)
            go, o2, x, w, what = bounce(co, cd, hit["t"], N, ks, transmission_rows(d, hit), w, mode, seed + 64 * k,
                                        q, bias)
            go &= has
            refr = refr | (what == 1)
            d2 = normalize(x)
            idx, co, cd, w, refr = idx[go], o2[go], d2[go], w[go], refr[go]
            if len(idx) == 0:
                break
    return {"rays": rays, "misses": misses, "refracted_misses": rm}
