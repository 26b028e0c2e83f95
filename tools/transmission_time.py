"""Developer tool: cost of refraction in the bounce loop (Renderer.render_traced(transmission=...)).
  frames     ms per W x H frame of CornellBox-Sphere and CornellBox-Water (tests/golden/cornell_models.tar.gz)
             and of c4 with a third of its spheres made glass, at max_depth 0 / 2 / 4 / 8 in the modes off /
             refract / fresnel, with depth_rays and the transmit counters beside them
  no_glass   c4 with ONE glass sphere behind the camera, where no ray meets it: "off" runs the mirror-only
             kernels, "refract" the TRANSMIT kernels on the very same rays; the difference is what the extra
             bounce code costs a level
--plain-only  times only the calls that exist without the feature (render_traced without a mode), on the
             same scenes minus their transmission entries: run it in a checkout of the parent commit to
             compare the TRANSMIT = false path with the kernels it must equal
HIP events on the renderer's stream, warm-up first, median of reps; prints one JSON line.
    python tools/transmission_time.py [--plain-only] [W=3840] [H=2160] [reps=5]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import esctp1raytracer_amd as esc

F32 = np.float32
DEPTHS = (0, 2, 4, 8)


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
    return sorted(ms)[len(ms) // 2]


def cornell(name):
    import tarfile
    import tempfile
    tmp = tempfile.mkdtemp()
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        t.extractall(tmp, filter="data") if hasattr(tarfile, "data_filter") else t.extractall(tmp)
    return esc.Scene.load_obj(os.path.join(tmp, "cornell", name + ".obj"))


def glass_c4(plain, hidden=False):
    """c4 with a third of its spheres glass, or (hidden) with one more glass sphere behind the camera"""
    sc = esc.Scene.synthetic("c4")
    sp, mats = sc.spheres()
    if hidden:
        sc.add_spheres(np.array([[0, 3, 60, 1]], F32), mats[:1])
        if not plain:
            sc.set_sphere_transmission(len(sp), [[0.9, 0.9, 0.9]], [1.5])
    elif not plain:
        sel = np.flatnonzero(np.random.default_rng(4).uniform(size=len(sp)) < 1 / 3)
        for k in sel:
            sc.set_sphere_transmission(int(k), [[0.9, 0.9, 0.9]], [1.5])
    return sc


def main():
    args = [a for a in sys.argv[1:] if a != "--plain-only"]
    plain = "--plain-only" in sys.argv
    W = int(args[0]) if len(args) > 0 else 3840
    H = int(args[1]) if len(args) > 1 else 2160
    reps = int(args[2]) if len(args) > 2 else 5
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    bias = 1e-3
    out = {"W": W, "H": H, "reps": reps, "plain_only": plain, "frames": [], "no_glass": []}
    modes = (None,) if plain else (None, "off", "refract", "fresnel")

    def measure(key, name, sc, view, depths, modes):
        r.upload(sc)
        cam = esc.Camera.for_image(*view, W, H)
        for depth in depths:
            for mode in modes:
                # Renderer.render_traced is synchronous and copies the frame back: the events go around
                # the asynchronous C call instead
                ms = timed(st, _async_frame(r, cam, W, H, depth, bias, mode), reps)
                ent = {"scene": name, "max_depth": depth, "mode": mode or "plain call", "ms": ms,
                       "depth_rays": r.trace_stats()["depth_rays"][:depth + 1]}
                if not plain:
                    ent.update(r.transmit_stats())
                out[key].append(ent)

    cview = ((0, 1, 3), (0, 1, 0))
    measure("frames", "CornellBox-Sphere", cornell("CornellBox-Sphere"), cview, DEPTHS, modes)
    measure("frames", "CornellBox-Water", cornell("CornellBox-Water"), cview, DEPTHS, modes)
    measure("frames", "c4, a third of the spheres glass", glass_c4(plain), esc.synthetic_view(), DEPTHS, modes)
    measure("no_glass", "c4 + one glass sphere behind the camera", glass_c4(plain, hidden=True), esc.synthetic_view(),
            (2, 4), (None,) if plain else (None, "off", "refract"))
    r.close()
    print(json.dumps(out))


_IMG = {}


def _async_frame(r, cam, W, H, depth, bias, mode):
    import ctypes as C
    from esctp1raytracer_amd import _capi
    if (W, H) not in _IMG:
        _IMG[(W, H)] = torch.empty((H, W, 3), dtype=torch.float32, device=torch.device("cuda", r.device))
        torch.cuda.synchronize()
    img = _IMG[(W, H)]
    opt = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO, 0, 0)
    if mode is None:
        return lambda: esc.check(r._lib.esc_render_traced(r._h, C.byref(cam.c), W, H, 1, depth, bias, C.byref(opt),
                                                          C.c_void_p(img.data_ptr()), None))
    to = _capi.esc_trace_options(depth, bias, {"off": 0, "refract": 1, "fresnel": 2}[mode], 0)
    return lambda: esc.check(r._lib.esc_render_traced_ex(r._h, C.byref(cam.c), W, H, 1, C.byref(opt), C.byref(to),
                                                         C.c_void_p(img.data_ptr()), None))


if __name__ == "__main__":
    main()
