"""Developer tool: cost of the mirror-reflection loop (Renderer.trace_rays / render_traced).
  level 0    trace_rays(max_depth=0) next to shade_rays on the same W x H camera rays of c4 and c5
             (the same work; every repetition is printed, so the run-to-run spread is visible)
  levels     on c4 with a third of its sphere materials given ks in 0.2..0.9: the bounce rays of levels 1
             and 2 are computed here (shade's t / prim, numpy reflection) and fed to shade_rays; beside it
             what the level costs inside the loop, trace_rays(max_depth=k) - trace_rays(max_depth=k-1).
             The difference is the price of the queue (and of launching the level over the whole batch)
  frames     ms per W x H frame of that c4 and of CornellBox-Mirror (tests/golden/cornell_models.tar.gz)
             at max_depth 0 / 1 / 2 / 4, with depth_rays beside them
HIP events on the renderer's stream, warm-up first, median of reps; prints one JSON line.
    python tools/trace_rays_time.py [configs=c4,c5] [W=3840] [H=2160] [reps=3]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import esctp1raytracer_amd as esc


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
    return sorted(ms)


def mirror_c4():
    sc = esc.Scene.synthetic("c4")
    sp, mats = sc.spheres()
    rng = np.random.default_rng(4)
    sel = rng.uniform(size=len(mats)) < 1 / 3
    mats = mats.copy()
    mats[sel, 6:9] = rng.uniform(0.2, 0.9, (int(sel.sum()), 3))
    out = esc.Scene()
    for i in range(sc.info()["n_geometry"]):
        g = sc.geometry(i)
        out.add_geometry(g["vertex"], g["face_index"], g["material"], normals=g.get("normals"))
    out.add_spheres(sp, mats)
    return out


F32 = np.float32


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F32) + a[:, 2] * b[:, 2]).astype(F32)


def bounce(sp, mats, o, d, w, sh, bias):
    """the survivors of one level on a scene whose reflecting primitives are spheres: (o', d', w')"""
    sph = (sh["geom"] < 0) & (sh["prim"] >= 0)
    k = np.where(sph, sh["prim"], 0)
    w = (w * np.where(sph[:, None], mats[k, 6:9], 0)).astype(F32)
    go = sph & (w > 0).any(axis=1)
    o, d, w, k, t = o[go], d[go], w[go], k[go], sh["t"][go]
    hit = (o + (d * t[:, None]).astype(F32)).astype(F32)
    N = (hit - sp[k, :3]).astype(F32)
    N = (N / np.sqrt(_dot(N, N))[:, None]).astype(F32)
    s = _dot(d, N)
    Nf = np.where((s > 0)[:, None], -N, N).astype(F32)
    x = (d - (N * (F32(2) * s)[:, None]).astype(F32)).astype(F32)
    return (hit + (Nf * F32(bias)).astype(F32)).astype(F32), (x / np.sqrt(_dot(x, x))[:, None]).astype(F32), w


def mirror_box():
    import tarfile
    import tempfile
    tmp = tempfile.mkdtemp()
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        t.extractall(tmp, filter="data") if hasattr(tarfile, "data_filter") else t.extractall(tmp)
    return esc.Scene.load_obj(os.path.join(tmp, "cornell", "CornellBox-Mirror.obj"))


def main():
    cfgs = (sys.argv[1] if len(sys.argv) > 1 else "c4,c5").split(",")
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 3840
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2160
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    out = {"W": W, "H": H, "reps": reps, "level0": [], "frames": []}
    cam = esc.Camera.for_image(*esc.synthetic_view(), W, H)
    for cfg in cfgs:
        r.upload(esc.Scene.synthetic(cfg))
        with torch.cuda.stream(st):
            o, d = r.camera_rays(cam, W, H)
            rgb = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
        shade = timed(st, lambda: r.shade_rays(o, d, rgb), reps)
        trace = timed(st, lambda: r.trace_rays(o, d, rgb, max_depth=0, bias=0.0), reps)
        out["level0"].append({"config": cfg, "rays": W * H, "shade_ms": shade, "trace_depth0_ms": trace})
    bias = 1e-3
    msc = mirror_c4()
    r.upload(msc)
    sp, mats = msc.spheres()
    with torch.cuda.stream(st):
        o, d = r.camera_rays(cam, W, H)
        rgb = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    r.synchronize()
    total = [timed(st, lambda: r.trace_rays(o, d, rgb, max_depth=k, bias=bias), reps)[reps // 2] for k in range(3)]
    on, dn, w = o.cpu().numpy(), d.cpu().numpy(), np.ones((W * H, 3), F32)
    out["levels"] = [{"level": 0, "rays": W * H, "trace_total_ms": total[0]}]
    for k in (1, 2):
        on, dn, w = bounce(sp, mats, on, dn, w, r.shade(on, dn), bias)
        with torch.cuda.stream(st):
            bo, bd = torch.from_numpy(on).to(dev), torch.from_numpy(dn).to(dev)
            brgb = torch.empty((len(on), 3), dtype=torch.float32, device=dev)
        ms = timed(st, lambda: r.shade_rays(bo, bd, brgb), reps)[reps // 2]
        out["levels"].append({"level": k, "rays": len(on), "shade_on_the_same_rays_ms": ms,
                              "trace_total_ms": total[k], "level_in_the_loop_ms": total[k] - total[k - 1]})
    import ctypes as C
    opt = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO, 0, 0)
    with torch.cuda.stream(st):
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    for name, sc, view in (("c4, a third of the spheres reflecting", msc, esc.synthetic_view()),
                           ("CornellBox-Mirror", mirror_box(), ((0, 1, 3.5), (0, 1, 0)))):
        r.upload(sc)
        fcam = esc.Camera.for_image(*view, W, H)
        for depth in (0, 1, 2, 4):
            ms = timed(st, lambda: esc.check(r._lib.esc_render_traced(r._h, C.byref(fcam.c), W, H, 1, depth, bias,
                                                                      C.byref(opt), C.c_void_p(img.data_ptr()),
                                                                      None)), reps)
            out["frames"].append({"scene": name, "max_depth": depth, "ms": ms[len(ms) // 2],
                                  "depth_rays": r.trace_stats()["depth_rays"][:depth + 1]})
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
