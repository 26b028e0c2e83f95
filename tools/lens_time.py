"""Developer tool: what the thin lens costs a traced frame.  c4 at W x H with spp samples per pixel and
max_depth 0: esc_render_traced (the existing call, the reference of the comparison), esc_render_lens at
aperture 0 (the same rays, made by k_lens_rays) and at 1 % of the scene's extent (less coherent waves in the
sweeps), the three alternating inside every round.  The scene's extent is taken from its spheres.
HIP events on the renderer's stream, warm-up first, median of reps; every repetition is printed; one JSON line.
    python tools/lens_time.py [W=3840] [H=2160] [spp=4] [reps=3]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi

C = esc.C


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 3840
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 2160
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    sc = esc.Scene.synthetic("c4")
    r.upload(sc)
    sph, _ = sc.spheres()
    extent = float(np.max((sph[:, :3] + sph[:, 3:4]).max(axis=0) - (sph[:, :3] - sph[:, 3:4]).min(axis=0)))
    eye, look = esc.synthetic_view()
    cam = esc.Camera.for_image(eye, look, W, H)
    focus = float(np.sqrt(((look - eye).astype(np.float32) ** 2).sum(dtype=np.float32)))
    r.set_lens_table(esc.lens_table(16, spp, 0))
    with torch.cuda.stream(st):
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    st.synchronize()
    o = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO)
    to = _capi.esc_trace_options(0, 1e-4, esc.ESC_TRANSMIT_OFF, 0)
    pi = C.c_void_p(img.data_ptr())

    def traced():
        esc.check(r._lib.esc_render_traced(r._h, C.byref(cam.c), W, H, spp, 0, 1e-4, C.byref(o), pi, None))

    def lens(aperture):
        lo = _capi.esc_lens_options(aperture, focus, 0)
        return lambda: esc.check(r._lib.esc_render_lens(r._h, C.byref(cam.c), W, H, spp, C.byref(o), C.byref(to),
                                                        C.byref(lo), pi, None))

    calls = {"render_traced": traced, "render_lens aperture 0": lens(0.0),
             "render_lens aperture 1%": lens(0.01 * extent)}
    ms = {k: [] for k in calls}
    for fn in calls.values():  # warm-up
        fn()
    st.synchronize()
    for _ in range(reps):
        for k, fn in calls.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            ms[k].append(round(e0.elapsed_time(e1), 3))
    out = {"config": "c4", "W": W, "H": H, "spp": spp, "max_depth": 0, "reps": reps, "extent": round(extent, 4),
           "focus_dist": round(focus, 4), "aperture_1pct": round(0.01 * extent, 5),
           "ms": {k: {"median": sorted(v)[len(v) // 2], "all": v} for k, v in ms.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
