"""Developer tool: batched ray query throughput (Renderer.intersect_rays / occluded_rays), filtered
and exact, on the synthetic configs, for two ray sets:
  coherent    the camera rays of a W x H frame (camera.h:31-34 formula in fp32 numpy, pixel centres)
  incoherent  origins uniform in the scene's box, unit directions from a seeded sphere sample
HIP events on the renderer's stream, warm-up first; prints one JSON line.
    python tools/ray_query_time.py [configs=c4,c5] [W=3840] [H=2160] [reps=5]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import esctp1raytracer_amd as esc

F32 = np.float32


def normalize(v):  # vec.h:135 in fp32, vec.h:95 dot order
    s = ((F32(0) + v[:, 0] * v[:, 0]) + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return (v / np.sqrt(s)[:, None]).astype(F32)


def coherent(W, H):
    c = esc.Camera.for_image(*esc.synthetic_view(), W, H).vectors()
    s = ((np.arange(W, dtype=F32) + F32(0.5)) / F32(W))[None, :].repeat(H, 0).reshape(-1)
    t = ((np.arange(H, dtype=F32) + F32(0.5)) / F32(H))[:, None].repeat(W, 1).reshape(-1)
    p = (c["lower_left_corner"] + c["horizontal"] * s[:, None]) + c["vertical"] * t[:, None]
    d = normalize((p - c["origin"]).astype(F32))
    return np.broadcast_to(c["origin"], d.shape).astype(F32).copy(), d


def incoherent(lo, hi, n, seed=1):
    rng = np.random.default_rng(seed)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F32)
    return o, normalize(rng.standard_normal((n, 3)).astype(F32))


def scene_box(sc):
    info = sc.info()
    pts = []
    for g in range(info["n_geometry"]):
        v = sc.geometry(g)["vertex"]
        if len(v):
            pts.append(v)
    sp, _ = sc.spheres()
    if len(sp):
        pts += [sp[:, :3] - sp[:, 3:], sp[:, :3] + sp[:, 3:]]
    p = np.concatenate(pts)
    return p.min(0), p.max(0)


def main():
    cfgs = (sys.argv[1] if len(sys.argv) > 1 else "c4,c5").split(",")
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 3840
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2160
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    out = {"W": W, "H": H, "reps": reps, "results": []}
    for cfg in cfgs:
        sc = esc.Scene.synthetic(cfg)
        r.upload(sc)
        info = sc.info()
        P = info["n_triangles"] + info["n_spheres"]
        lo, hi = scene_box(sc)
        sets = {"coherent": coherent(W, H), "incoherent": incoherent(lo, hi, W * H)}
        for set_name, (o, d) in sets.items():
            n = o.shape[0]
            with torch.cuda.stream(st):
                to = torch.from_numpy(o).to(dev)
                td = torch.from_numpy(d).to(dev)
                t = torch.empty(n, dtype=torch.float32, device=dev)
                g = torch.empty(n, dtype=torch.int32, device=dev)
                p = torch.empty(n, dtype=torch.int32, device=dev)
                oc = torch.empty(n, dtype=torch.uint8, device=dev)
            st.synchronize()
            for kind in ("closest", "occluded"):
                for exact in (False, True):
                    # exact: the first 2^20 rays only (every ray costs the same P tests there)
                    m_n = min(n, 1 << 20) if exact else n

                    def launch():
                        if kind == "closest":
                            r.intersect_rays(to[:m_n], td[:m_n], t[:m_n], g[:m_n], p[:m_n], exact=exact)
                        else:
                            r.occluded_rays(to[:m_n], td[:m_n], oc[:m_n], exact=exact)
                    launch()  # warm-up (and the stats of this configuration)
                    stats = r.query_stats()
                    k = 1 if exact else reps
                    ms = []
                    for _ in range(k):
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        launch()
                        e1.record(st)
                        st.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    ms.sort()
                    m = ms[len(ms) // 2]  # noqa: E741
                    hits = int((p[:m_n] >= 0).sum().item()) if kind == "closest" else int(oc[:m_n].sum().item())
                    out["results"].append({
                        "config": cfg, "rays": set_name, "query": kind, "exact": exact, "n": m_n,
                        "primitives": P, "ms": round(m, 4), "mrays_per_s": round(m_n / m / 1e3, 2),
                        "exact_rays": stats["exact_rays"], "exact_tests": stats["exact_tests"],
                        "exact_test_fraction": stats["exact_tests"] / float(m_n * P), "hits": hits})
                    print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
