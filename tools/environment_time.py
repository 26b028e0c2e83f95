"""Developer tool: cost of the environment cube map (Renderer.set_environment / environment_rays).
  lookup     environment_rays on the W x H frame's camera directions of c4 (coherent: neighbouring lanes read
             neighbouring texels) and on the same number of random directions (every lane its own texel rows),
             at R = 64 and R = 1024, next to a plain device copy of the same 24 bytes per direction (12 read,
             12 written) measured in the same run
  frames     render_traced of tools/trace_rays_time.py's c4 (a third of the spheres reflecting) at depth
             0 / 1 / 2, without an environment and with one (R = 64 and R = 1024), with the misses per frame
HIP events on the renderer's stream, warm-up first, every repetition printed; prints one JSON line.
    python tools/environment_time.py [W=3840] [H=2160] [reps=5]"""
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
from trace_rays_time import mirror_c4, timed


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 3840
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 2160
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    n = W * H
    out = {"W": W, "H": H, "reps": reps, "directions": n, "lookup": [], "frames": []}
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    msc = mirror_c4()
    r.upload(msc)
    rng = np.random.default_rng(1)
    with torch.cuda.stream(st):
        _, coherent = r.camera_rays(cam, W, H)
        scattered = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    r.synchronize()

    def copy():
        with torch.cuda.stream(st):
            rgb.copy_(coherent)

    ms = timed(st, copy, reps)
    out["copy_24_bytes_per_direction"] = {"ms": ms, "G_directions_per_s": n / ms[len(ms) // 2] * 1e-6}
    sky = ((0.1, 0.3, 0.9), (0.8, 0.8, 0.7), (0.2, 0.15, 0.1))
    for res in (64, 1024):
        cube = esc.environment_sky(res, *sky)
        cube += rng.uniform(0, 0.05, cube.shape).astype(np.float32)  # not constant along a row
        r.set_environment(cube)
        for name, dirs in (("coherent", coherent), ("random", scattered)):
            ms = timed(st, lambda: r.environment_rays(dirs, rgb), reps)
            out["lookup"].append({"res": res, "directions": name, "ms": ms,
                                  "G_directions_per_s": n / ms[len(ms) // 2] * 1e-6})
    bias = 1e-3
    opt = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO, 0, 0)
    for res in (0, 64, 1024):
        r.set_environment(None if res == 0 else esc.environment_sky(res, *sky))
        for depth in (0, 1, 2):
            ms = timed(st, lambda: esc.check(r._lib.esc_render_traced(r._h, C.byref(cam.c), W, H, 1, depth, bias,
                                                                      C.byref(opt), C.c_void_p(img.data_ptr()),
                                                                      None)), reps)
            s = r.trace_stats()
            out["frames"].append({"environment_res": res, "max_depth": depth, "ms": ms,
                                  "depth_rays": s["depth_rays"][:depth + 1], "misses": s["rays"] - s["hit_rays"]})
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
