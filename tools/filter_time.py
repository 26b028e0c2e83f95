"""Developer tool: cost of the G-buffer (esc_render_gbuffer) and of the edge-stopping a-trous filter
(esc_filter_guided, 1 and 3 channels, L = 1, 3, 5) next to esc_render_ambient (K = 16) of the same frame, the
yardstick for what the filter adds to an ambient-occlusion frame.
  c4 at 1920 x 1080 and CornellBox-Water (tests/golden/cornell_models.tar.gz) at 960 x 540; the filtered image
  is the frame's vis (1 channel) or its sky light (3 channels), the guides are esc_render_gbuffer's, normal_cos
  0.9, plane_dist 0.02 x the scene's extent, same_object on.
For the filter the achieved bytes/s are stated against its algorithmic traffic: the pack reads the four guide
arrays (32 bytes) and writes the record (32 bytes) per pixel once; every iteration reads the guide record (32
bytes) and one image value and writes one (8 * channels bytes) per pixel -- taps beyond the pixel's own are
expected from cache -- and against the 6.29 TB/s a float4 copy measures on this part.
HIP events on the renderer's stream, warm-up first, median / min / max of the repetitions.  Prints one JSON line.
    python tools/filter_time.py [reps=7] [scale=1.0] [scenes=c4,water]     (scale scales both frames)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import esctp1raytracer_amd as esc
from ambient_time import BIAS, K, scene_tensors, stats_of, timed, water_box
from esctp1raytracer_amd import _capi

SKY = ((0.2, 0.4, 1.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1))
HBM_COPY_TBS = 6.29
ITERATIONS = (1, 3, 5)


def measure(r, st, dev, name, sc, view, W, H, reps, out):
    r.upload(sc)
    _, extent = scene_tensors(sc, dev)
    cam = esc.Camera.for_image(*view, W, H)
    n = W * H
    lib, h = r._lib, r._h
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.stream(st):
        vis = torch.empty(n, dtype=torch.float32, device=dev)
        light = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out1 = torch.empty_like(vis)
        out3 = torch.empty_like(light)
    st.synchronize()
    g = r.render_gbuffer(cam, W, H)
    radius = float(np.float32(0.25 * extent))
    ao = _capi.esc_ambient_options(K, 16, radius, BIAS, 0, 0, 0)

    def ambient_frame():
        esc.check(lib.esc_render_ambient(h, C.byref(cam.c), W, H, C.byref(ao), p(vis), None))

    def gbuffer_frame():
        esc.check(lib.esc_render_gbuffer(h, C.byref(cam.c), W, H, 0, p(g["normal"]), p(g["position"]), p(g["albedo"]),
                                         p(g["t"]), p(g["geom"]), p(g["prim"])))

    def gbuffer_guides():  # what the filter reads: no albedo, no t
        esc.check(lib.esc_render_gbuffer(h, C.byref(cam.c), W, H, 0, p(g["normal"]), p(g["position"]), None, None,
                                         p(g["geom"]), p(g["prim"])))

    esc.check(lib.esc_render_skylight(h, C.byref(cam.c), W, H, C.byref(ao), None, p(light), p(vis), None))
    r.synchronize()
    res = {"scene": name, "W": W, "H": H, "K": K, "S": 16, "radius": "0.25 extent", "normal_cos": 0.9,
           "plane_dist": "0.02 extent", "gbuffer": r.gbuffer_stats()}
    for key, fn in (("ambient_frame_ms", ambient_frame), ("gbuffer_frame_ms", gbuffer_frame),
                    ("gbuffer_guides_ms", gbuffer_guides)):
        fn()
        res[key] = stats_of([timed(st, fn) for _ in range(reps)])
    res["filter"] = []
    for ch, src, dst in ((1, vis, out1), (3, light, out3)):
        for L in ITERATIONS:
            o = _capi.esc_filter_options(L, 0.9, float(np.float32(0.02 * extent)), 1)

            def filt():
                esc.check(lib.esc_filter_guided(h, W, H, ch, p(src), p(g["normal"]), p(g["position"]), p(g["geom"]),
                                                p(g["prim"]), C.byref(o), p(dst)))

            filt()  # warm-up: the scratch grows here
            s = r.filter_stats()
            ms = stats_of([timed(st, filt) for _ in range(reps)])
            traffic = n * (64 + L * (32 + 8 * ch))
            tbs = traffic / (ms["median"] * 1e-3) / 1e12
            row = {"channels": ch, "L": L, "ms": ms, "algorithmic_bytes": traffic, "achieved_TBps": round(tbs, 3),
                   "share_of_copy_bandwidth": round(tbs / HBM_COPY_TBS, 3),
                   "share_of_ambient_frame": round(ms["median"] / res["ambient_frame_ms"]["median"], 4),
                   "accepted_share": round(s["taps_accepted"] / max(1, s["taps_tested"]), 4), "stats": s}
            res["filter"].append(row)
    out["results"].append(res)
    print(json.dumps(res), file=sys.stderr, flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    if reps < 5:
        raise SystemExit("at least 5 repetitions")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    r.set_environment(esc.environment_sky(64, *SKY))
    r.set_ambient_table(esc.ambient_table(16, K, 0))
    scenes = (sys.argv[3] if len(sys.argv) > 3 else "c4,water").split(",")
    out = {"K": K, "reps": reps, "bias": BIAS, "scale": scale, "hbm_copy_TBps": HBM_COPY_TBS, "results": []}
    if "c4" in scenes:
        measure(r, st, dev, "c4", esc.Scene.synthetic("c4"), esc.synthetic_view(), int(1920 * scale),
                int(1080 * scale), reps, out)
    if "water" in scenes:
        measure(r, st, dev, "CornellBox-Water", water_box(), ((0, 1, 3.5), (0, 1, 0)), int(960 * scale),
                int(540 * scale), reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
