"""Developer tool: throughput of the shading of caller-supplied rays (Renderer.shade_rays), filtered
and exact, and of supersampled frames (Renderer.render_supersampled), on the synthetic configs.
Ray sets:
  camera      the frame's own primary rays (Renderer.camera_rays) of a W x H frame
  incoherent  origins uniform in the scene's box, unit directions from a seeded sphere sample
Exact runs shade the first 2^18 rays only (every ray there costs the same (1 + lights) x P tests).
Then a c4 W x H frame at spp 1, 4 and 16, next to the default frame path.
HIP events on the renderer's stream, warm-up first; prints one JSON line.
    python tools/shade_rays_time.py [configs=c4,c5] [W=3840] [H=2160] [reps=3]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import esctp1raytracer_amd as esc
from ray_query_time import incoherent, scene_box


def timed(st, fn, reps):
    fn()  # warm-up
    st.synchronize()
    ms = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    cfgs = (sys.argv[1] if len(sys.argv) > 1 else "c4,c5").split(",")
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 3840
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2160
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    out = {"W": W, "H": H, "reps": reps, "results": [], "supersampled": []}
    for cfg in cfgs:
        sc = esc.Scene.synthetic(cfg)
        r.upload(sc)
        info = sc.info()
        P = info["n_triangles"] + info["n_spheres"]
        cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
        with torch.cuda.stream(st):
            co, cd = r.camera_rays(cam, W, H)
        lo, hi = scene_box(sc)
        io, idr = incoherent(lo, hi, W * H)
        with torch.cuda.stream(st):
            sets = {"camera": (co, cd), "incoherent": (torch.from_numpy(io).to(dev), torch.from_numpy(idr).to(dev))}
            rgb = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
        st.synchronize()
        for set_name, (o, d) in sets.items():
            for exact in (False, True):
                n = min(W * H, 1 << 18) if exact else W * H
                ms = timed(st, lambda: r.shade_rays(o[:n], d[:n], rgb[:n], exact=exact), 1 if exact else reps)
                s = r.shade_stats()
                out["results"].append({
                    "config": cfg, "rays": set_name, "exact": exact, "n": n, "primitives": P, "ms": round(ms, 3),
                    "grays_per_s": round(n / ms / 1e6, 4), "hit_rays": s["hit_rays"],
                    "shadow_rays": s["shadow_rays"], "exact_rays": s["exact_rays"],
                    "exact_tests": s["exact_tests"]})
                print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
        if cfg == "c4":
            with torch.cuda.stream(st):
                img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
            st.synchronize()
            frame_ms = timed(st, lambda: r.render_rows(cam, W, H, 0, H, img), reps)
            out["supersampled"].append({"config": cfg, "spp": "frame path", "ms": round(frame_ms, 3)})
            for spp in (1, 4, 16):
                o = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO)

                def ss():
                    esc.check(r._lib.esc_render_supersampled(r._h, esc.C.byref(cam.c), W, H, spp, esc.C.byref(o),
                                                             esc.C.c_void_p(img.data_ptr()), None))
                ms = timed(st, ss, 1 if spp == 16 else reps)
                out["supersampled"].append({"config": cfg, "spp": spp, "ms": round(ms, 3),
                                            "grays_per_s": round(W * H * spp / ms / 1e6, 4)})
                print(json.dumps(out["supersampled"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
