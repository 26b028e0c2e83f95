"""Developer tool: cost of the temporal accumulation (esc_temporal_accumulate, 1 and 3 channels, 1 and 4 taps)
next to esc_filter_guided with L = 1 -- the yardstick: existing code that reads 25 taps per pixel where this
reads at most 4 -- and to esc_render_ambient with K = 4 and K = 16 of the same frame, in one session.
  c4 at 1920 x 1080 and CornellBox-Water (tests/golden/cornell_models.tar.gz) at 960 x 540; the accumulated
  image is the frame's vis (1 channel) or its sky light (3 channels); the previous frame is seen from an eye
  moved by 0.01 x the scene's extent, its guides are esc_render_gbuffer's, its image serves as the history and
  every history length is 8; normal_cos 0.9, plane_dist 0.02 x the scene's extent, same_object on, M = 32.
The achieved bytes/s are stated against the call's algorithmic traffic, per pixel: current, its guides (32
bytes), one previous guide record (32), one history length (4) and one history value read, the output and its
length written: 72 + 12 * channels bytes -- a history record is needed about once per pixel, further taps are
expected from cache -- and against the 6.29 TB/s a float4 copy measures on this part.
HIP events on the renderer's stream, warm-up first, median / min / max of the repetitions.  Prints one JSON line.
    python tools/temporal_time.py [reps=7] [scale=1.0] [scenes=c4,water]     (scale scales both frames)"""
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
from ambient_time import BIAS, scene_tensors, stats_of, timed, water_box
from esctp1raytracer_amd import _capi

SKY = ((0.2, 0.4, 1.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1))
HBM_COPY_TBS = 6.29
SAMPLES = (4, 16)


def measure(r, st, dev, name, sc, view, W, H, reps, out):
    r.upload(sc)
    _, extent = scene_tensors(sc, dev)
    eye, look = (np.array(v, np.float32) for v in view)
    cam = esc.Camera.for_image(tuple(eye), tuple(look), W, H)
    prev_cam = esc.Camera.for_image(tuple(eye + np.float32(0.01 * extent)), tuple(look), W, H)
    n = W * H
    lib, h = r._lib, r._h
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.stream(st):
        vis, hist1 = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        light, hist3 = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(2))
        out1, out3 = torch.empty_like(vis), torch.empty_like(light)
        hist_n = torch.full((n,), 8, dtype=torch.int32, device=dev)
        out_n = torch.empty_like(hist_n)
    st.synchronize()
    g, gp = r.render_gbuffer(cam, W, H), r.render_gbuffer(prev_cam, W, H)
    guides = [_capi.esc_guides(*[x[k].data_ptr() for k in ("normal", "position", "geom", "prim")]) for x in (g, gp)]
    radius = float(np.float32(0.25 * extent))
    plane = float(np.float32(0.02 * extent))
    res = {"scene": name, "W": W, "H": H, "S": 16, "radius": "0.25 extent", "normal_cos": 0.9,
           "plane_dist": "0.02 extent", "max_history": 32, "eye_shift": "0.01 extent", "ambient_frame_ms": {}}
    for K in SAMPLES:
        r.set_ambient_table(esc.ambient_table(16, K, 0))
        ao = _capi.esc_ambient_options(K, 16, radius, BIAS, 0, 0, 0)

        def ambient_frame():
            esc.check(lib.esc_render_ambient(h, C.byref(cam.c), W, H, C.byref(ao), p(vis), None))

        ambient_frame()
        res["ambient_frame_ms"][f"K{K}"] = stats_of([timed(st, ambient_frame) for _ in range(reps)])
    # the images: the two frames' vis and sky light at K = 16
    esc.check(lib.esc_render_skylight(h, C.byref(prev_cam.c), W, H, C.byref(ao), None, p(hist3), p(hist1), None))
    esc.check(lib.esc_render_skylight(h, C.byref(cam.c), W, H, C.byref(ao), None, p(light), p(vis), None))
    r.synchronize()
    res["filter_L1"], res["temporal"] = [], []
    for ch, src, hist, dst in ((1, vis, hist1, out1), (3, light, hist3, out3)):
        fo = _capi.esc_filter_options(1, 0.9, plane, 1)

        def filt():
            esc.check(lib.esc_filter_guided(h, W, H, ch, p(src), p(g["normal"]), p(g["position"]), p(g["geom"]),
                                            p(g["prim"]), C.byref(fo), p(dst)))

        filt()  # warm-up: the scratch grows here
        fms = stats_of([timed(st, filt) for _ in range(reps)])
        res["filter_L1"].append({"channels": ch, "ms": fms, "algorithmic_bytes": n * (64 + 32 + 8 * ch)})
        for taps in (1, 4):
            to = _capi.esc_temporal_options(taps, 32, 0.9, plane, 1)

            def accumulate():
                esc.check(lib.esc_temporal_accumulate(h, C.byref(prev_cam.c), W, H, ch, p(src), C.byref(guides[0]),
                                                      p(hist), p(hist_n), C.byref(guides[1]), C.byref(to), p(dst),
                                                      p(out_n)))

            accumulate()
            s = r.temporal_stats()
            ms = stats_of([timed(st, accumulate) for _ in range(reps)])
            traffic = n * (72 + 12 * ch)
            tbs = traffic / (ms["median"] * 1e-3) / 1e12
            res["temporal"].append({
                "channels": ch, "taps": taps, "ms": ms, "algorithmic_bytes": traffic, "achieved_TBps": round(tbs, 3),
                "share_of_copy_bandwidth": round(tbs / HBM_COPY_TBS, 3),
                "times_filter_L1": round(ms["median"] / fms["median"], 3),
                "share_of_ambient_K4_frame": round(ms["median"] / res["ambient_frame_ms"]["K4"]["median"], 4),
                "reused_share": round(s["reused_pixels"] / max(1, s["hit_pixels"]), 4), "stats": s})
    a = res["ambient_frame_ms"]
    t = max(x["ms"]["median"] for x in res["temporal"] if x["channels"] == 1)
    gb = stats_of([timed(st, lambda: esc.check(lib.esc_render_gbuffer(
        h, C.byref(cam.c), W, H, 0, p(g["normal"]), p(g["position"]), None, None, p(g["geom"]), p(g["prim"]))))
        for _ in range(reps)])
    res["gbuffer_guides_ms"] = gb
    # four frames of K = 4, each with its guides and one accumulation, against one frame of K = 16
    res["four_K4_frames_accumulated_ms"] = round(4 * (a["K4"]["median"] + gb["median"] + t), 4)
    res["one_K16_frame_ms"] = a["K16"]["median"]
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
    scenes = (sys.argv[3] if len(sys.argv) > 3 else "c4,water").split(",")
    out = {"reps": reps, "bias": BIAS, "scale": scale, "hbm_copy_TBps": HBM_COPY_TBS, "results": []}
    if "c4" in scenes:
        measure(r, st, dev, "c4", esc.Scene.synthetic("c4"), esc.synthetic_view(), int(1920 * scale),
                int(1080 * scale), reps, out)
    if "water" in scenes:
        measure(r, st, dev, "CornellBox-Water", water_box(), ((0, 1, 3.5), (0, 1, 0)), int(960 * scale),
                int(540 * scale), reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
