"""The CPU restatement of the temporal accumulation (include/esctp1_rt.h at esc_temporal_options) that the tests
compare the GPU with: numpy fp32 with one rounding per operation (.astype(F32) after every one), built on
ray_oracle.py's pieces, as filter_lib.py is.  No scenes and no pytest here; tests/temporal_cases.py chooses cases
with it.

Nothing here is transcendental: + - * /, floor and compares, so images are compared bit for bit and counts
exactly.  reverse=True visits the 4 taps in the opposite order: the tests use it only to show that the order
matters to the bits."""
import numpy as np

from ray_oracle import F32, cross, dot

STOPS = ("missing", "history", "object", "normal", "plane")
COUNTS = ("pixels", "hit_pixels", "reused_pixels", "taps_tested", "taps_accepted")
INT32_MAX = 2 ** 31 - 1


def camera_vectors(cam):
    """a Camera, or a dict of its four vectors -> {"origin", "lower_left_corner", "horizontal", "vertical"}"""
    v = cam.vectors() if hasattr(cam, "vectors") else cam
    return {k: np.ascontiguousarray(v[k], F32).reshape(3)
            for k in ("origin", "lower_left_corner", "horizontal", "vertical")}


def reproject(prev_cam, position, W, H):
    """-> (fx, fy, z): where the previous camera sees the (H, W, 3) world-space points, in pixels, and the
    solve's third unknown (in front of the camera iff z > 0)"""
    c = camera_vectors(prev_cam)
    P = np.ascontiguousarray(position, F32).reshape(H, W, 3)
    with np.errstate(all="ignore"):
        A = (c["lower_left_corner"] - c["origin"]).astype(F32)
        Hh, V = c["horizontal"], c["vertical"]
        v = (P - c["origin"]).astype(F32)
        Ab, Hb, Vb = (np.broadcast_to(a, v.shape) for a in (A, Hh, V))
        cv = cross(Vb, v)
        det = dot(Hb, cv)
        x = (dot(Ab, cv) / det).astype(F32)
        y = (dot(Hb, cross(Ab, v)) / det).astype(F32)
        z = (dot(Hb, cross(Vb, Ab)) / det).astype(F32)
        fx = ((-x).astype(F32) * F32(W - 1)).astype(F32)
        fy = ((-y).astype(F32) * F32(H - 1)).astype(F32)
    return fx, fy, z


def accumulate(current, cur, prev_cam, history, history_n, prev, taps=4, max_history=32, normal_cos=0.9,
               plane_dist=0.0, same_object=True, reverse=False):
    """-> (out, out_n, stats): out has current's shape ((H, W) or (H, W, C)), out_n is (H, W) int32; stats holds
    COUNTS and, per stop of STOPS, how many tested taps it was the first to reject.  cur, prev: "normal",
    "position" (H*W*3 values each), "geom", "prim" (H*W each), in any shape."""
    img = np.ascontiguousarray(current, F32)
    H, W = img.shape[:2]
    I = img.reshape(H, W, -1)
    Hist = np.ascontiguousarray(history, F32).reshape(I.shape)
    Hn = np.asarray(history_n, np.int32).reshape(H, W)
    g = {}
    for name, d in (("c", cur), ("p", prev)):
        g["N" + name] = np.ascontiguousarray(d["normal"], F32).reshape(H, W, 3)
        g["P" + name] = np.ascontiguousarray(d["position"], F32).reshape(H, W, 3)
        g["G" + name] = np.asarray(d["geom"], np.int32).reshape(H, W)
        g["R" + name] = np.asarray(d["prim"], np.int32).reshape(H, W)
    Nc, Pc, Gc, Rc = g["Nc"], g["Pc"], g["Gc"], g["Rc"]
    Np_, Pp_, Gp, Rp = g["Np"], g["Pp"], g["Gp"], g["Rp"]
    nc, pd, M = F32(normal_cos), F32(plane_dist), int(max_history)
    hit = (Gc >= 0) | (Rc >= 0)
    hit_prev = (Gp >= 0) | (Rp >= 0)
    st = dict.fromkeys(COUNTS + STOPS, 0)
    st["pixels"], st["hit_pixels"] = H * W, int(hit.sum())
    one = F32(1)
    with np.errstate(all="ignore"):
        fx, fy, z = reproject(prev_cam, Pc, W, H)
        valid = hit & (z > 0) & (fx >= F32(-1)) & (fx <= F32(W)) & (fy >= F32(-1)) & (fy <= F32(H))
        if taps == 1:
            x0 = np.floor((fx + F32(0.5)).astype(F32)).astype(F32)
            y0 = np.floor((fy + F32(0.5)).astype(F32)).astype(F32)
            order = [(0, 0)]
        elif taps == 4:
            x0, y0 = np.floor(fx).astype(F32), np.floor(fy).astype(F32)
            ax, ay = (fx - x0).astype(F32), (fy - y0).astype(F32)
            order = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (j, i)
        else:
            raise ValueError("taps must be 1 or 4")
        if reverse:
            order.reverse()
        acc = np.zeros(I.shape, F32)
        ws = np.zeros((H, W), F32)
        n = np.full((H, W), INT32_MAX, np.int64)
        for j, i in order:
            qx, qy = (x0 + F32(i)).astype(F32), (y0 + F32(j)).astype(F32)
            take = valid & (qx >= 0) & (qx <= F32(W - 1)) & (qy >= 0) & (qy <= F32(H - 1))
            if taps == 1:
                k = np.ones((H, W), F32)
            else:
                k = ((ax if i else (one - ax).astype(F32)) * (ay if j else (one - ay).astype(F32))).astype(F32)
            take = take & (k > 0)
            st["taps_tested"] += int(take.sum())
            qw = np.where(take, qx, 0).astype(np.int64)  # converted only after the float range test
            qh = np.where(take, qy, 0).astype(np.int64)
            checks = [("missing", hit_prev[qh, qw]), ("history", Hn[qh, qw] >= 1)]
            if same_object:
                checks.append(("object", (Gp[qh, qw] == Gc) & ((Gc >= 0) | (Rp[qh, qw] == Rc))))
            checks.append(("normal", dot(Nc, Np_[qh, qw]) >= nc))
            checks.append(("plane", np.abs(dot((Pp_[qh, qw] - Pc).astype(F32), Nc)) <= pd))
            for name, ok in checks:
                st[name] += int((take & ~ok).sum())
                take = take & ok
            st["taps_accepted"] += int(take.sum())
            acc = np.where(take[..., None], (acc + (k[..., None] * Hist[qh, qw]).astype(F32)).astype(F32), acc)
            ws = np.where(take, (ws + k).astype(F32), ws)
            n = np.where(take, np.minimum(n, Hn[qh, qw]), n)
        reused = hit & (ws > 0)
        st["reused_pixels"] = int(reused.sum())
        m = np.minimum(n, M - 1) + 1
        alpha = (one / m.astype(F32)).astype(F32)
        hc = (acc / ws[..., None]).astype(F32)
        blend = (hc + ((I - hc).astype(F32) * alpha[..., None]).astype(F32)).astype(F32)
    out = np.where(reused[..., None], blend, I)
    out_n = np.where(hit, np.where(reused, m, 1), 0).astype(np.int32)
    return np.ascontiguousarray(out.reshape(img.shape), F32), out_n, st
