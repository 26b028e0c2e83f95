"""Developer tool: cost of sky lighting (esc_render_skylight) next to ambient occlusion on the same inputs
(esc_render_ambient) and next to the path a caller had to compose before: intersect_rays, normals and sample
rays in torch, occluded_rays on the n x K rays, environment_rays on the open ones, the sum per ray in torch.
  c4 at 1920 x 1080 and CornellBox-Water (tests/golden/cornell_models.tar.gz) at 960 x 540, K = 16,
  S in {1, 16}, radius 0.25 x the scene's extent and unbounded, a 64-texel sky cube.  Per configuration:
    ambient_frame   esc_render_ambient (vis and count)
    skylight_frame  esc_render_skylight (sky, light, vis and count)
    skylight_light  esc_render_skylight writing light alone (what the viewer asks for)
    skylight_rays   esc_skylight_rays on esc_camera_rays' rays
    composed        esc_intersect_rays + [torch glue] + esc_occluded_rays on the hit x K sample rays + [torch
                    glue] + esc_environment_rays on the open ones + [torch glue: the sum per ray]; the three
                    library calls are timed apart from the glue
HIP events on the renderer's stream, warm-up first, median / min / max of the repetitions.  The verdict per
configuration: skylight_frame's median minus the composed LIBRARY calls' median, against the spread (max - min)
of the composed library calls' own repetitions.  Prints one JSON line.  The glue and the scenes are those of
tools/ambient_time.py.
    python tools/skylight_time.py [reps=7] [scale=1.0] [scenes=c4,water]     (scale scales both frames)"""
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
from ambient_time import BIAS, FLT_MAX, K, glue, mix_hi32, scene_tensors, stats_of, timed, water_box
from esctp1raytracer_amd import _capi

SKY_RES = 64
SKY = ((0.2, 0.4, 1.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1))


def measure(r, st, dev, name, sc, view, W, H, reps, out):
    r.upload(sc)
    T, extent = scene_tensors(sc, dev)
    cam = esc.Camera.for_image(*view, W, H)
    n = W * H
    lib, h = r._lib, r._h
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.stream(st):
        sky = torch.empty((n, 3), dtype=torch.float32, device=dev)
        light = torch.empty((n, 3), dtype=torch.float32, device=dev)
        vis = torch.empty(n, dtype=torch.float32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        geom = torch.empty(n, dtype=torch.int32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
    st.synchronize()
    to, td = r.camera_rays(cam, W, H)
    r.synchronize()
    for S in (1, 16):
        table_h = esc.ambient_table(S, K, 0)
        r.set_ambient_table(table_h)
        with torch.cuda.stream(st):
            table = torch.from_numpy(table_h).to(dev)
            sets = torch.from_numpy((mix_hi32(0, np.arange(n, dtype=np.uint32), 0xFFFFFFFE) % np.uint32(S))
                                    .astype(np.int64)).to(dev)
        st.synchronize()
        for rname, radius in (("0.25 extent", float(np.float32(0.25 * extent))), ("unbounded", FLT_MAX)):
            o = _capi.esc_ambient_options(K, S, radius, BIAS, 0, 0, 0)

            def ambient_frame():
                esc.check(lib.esc_render_ambient(h, C.byref(cam.c), W, H, C.byref(o), p(vis), p(cnt)))

            def skylight_frame():
                esc.check(lib.esc_render_skylight(h, C.byref(cam.c), W, H, C.byref(o), p(sky), p(light), p(vis),
                                                  p(cnt)))

            def skylight_light():
                esc.check(lib.esc_render_skylight(h, C.byref(cam.c), W, H, C.byref(o), None, p(light), None, None))

            def skylight_rays():
                esc.check(lib.esc_skylight_rays(h, n, p(to), p(td), C.byref(o), p(sky), p(light), p(vis), p(cnt),
                                                None, None, None))

            res = {"scene": name, "W": W, "H": H, "K": K, "S": S, "radius": rname, "sky_res": SKY_RES}
            skylight_frame()  # warm-up, and the counts of this configuration
            s = r.ambient_stats()
            res.update(hit_rays=s["hit_rays"], samples=s["samples"], occluded_samples=s["occluded_samples"],
                       exact_rays=s["exact_rays"], mean_vis=round(float(vis.mean().item()), 5),
                       mean_sky=[round(float(x), 5) for x in sky.mean(0).tolist()])
            for key, fn in (("ambient_frame_ms", ambient_frame), ("skylight_frame_ms", skylight_frame),
                            ("skylight_light_ms", skylight_light), ("skylight_rays_ms", skylight_rays)):
                fn()
                res[key] = stats_of([timed(st, fn) for _ in range(reps)])
            # the composed path, library calls timed apart from the glue
            lib_ms, glue_ms, n_open = [], [], 0
            for k in range(reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
                with torch.cuda.stream(st):
                    ev[0].record(st)
                    r.intersect_rays(to, td, t, geom, prim, uv=uv)
                    ev[1].record(st)
                    idx, so, sd, tm = glue(T, to, td, t, geom, prim, uv, sets, table, radius)
                    occ = torch.empty(so.shape[0], dtype=torch.uint8, device=dev)
                    ev[2].record(st)
                    r.occluded_rays(so, sd, occ, tmax=tm)
                    ev[3].record(st)
                    op = torch.nonzero(occ == 0).squeeze(1)
                    od = sd[op].contiguous()
                    rgb = torch.empty((od.shape[0], 3), dtype=torch.float32, device=dev)
                    ev[4].record(st)
                    if od.shape[0]:
                        r.environment_rays(od, rgb)
                    ev[5].record(st)
                    acc = torch.zeros((n, 3), dtype=torch.float32, device=dev)
                    acc.index_add_(0, idx[op // K], rgb)
                    acc /= float(K)
                    ev[6].record(st)
                st.synchronize()
                if k:  # the first round is the warm-up
                    lib_ms.append(ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]) + ev[4].elapsed_time(ev[5]))
                    glue_ms.append(ev[1].elapsed_time(ev[2]) + ev[3].elapsed_time(ev[4]) + ev[5].elapsed_time(ev[6]))
                n_open = int(od.shape[0])
                del so, sd, tm, occ, op, od, rgb, acc
            res["composed_lib_ms"] = stats_of(lib_ms)
            res["composed_glue_ms"] = stats_of(glue_ms)
            res["composed_open_samples"] = n_open  # torch's rounding of the glue may move a few samples
            spread = res["composed_lib_ms"]["max"] - res["composed_lib_ms"]["min"]
            diff = res["skylight_frame_ms"]["median"] - res["composed_lib_ms"]["median"]
            res["skylight_minus_ambient_ms"] = round(res["skylight_frame_ms"]["median"] -
                                                     res["ambient_frame_ms"]["median"], 4)
            res["skylight_minus_composed_lib_ms"] = round(diff, 4)
            res["composed_lib_spread_ms"] = round(spread, 4)
            res["skylight_not_slower_beyond_spread"] = bool(diff <= spread)
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
    r.set_environment(esc.environment_sky(SKY_RES, *SKY))
    scenes = (sys.argv[3] if len(sys.argv) > 3 else "c4,water").split(",")
    out = {"K": K, "reps": reps, "bias": BIAS, "scale": scale, "sky_res": SKY_RES, "results": []}
    if "c4" in scenes:
        measure(r, st, dev, "c4", esc.Scene.synthetic("c4"), esc.synthetic_view(), int(1920 * scale),
                int(1080 * scale), reps, out)
    if "water" in scenes:
        measure(r, st, dev, "CornellBox-Water", water_box(), ((0, 1, 3.5), (0, 1, 0)), int(960 * scale),
                int(540 * scale), reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
