"""Developer tool: cost of adaptive supersampling (Renderer.render_adaptive) next to the frame and to full
supersampling, in one process:
  c4 at 3840 x 2160 and CornellBox-Water (tests/golden/cornell_models.tar.gz) at 1920 x 1080:
  esc_render_rows (the frame), esc_render_supersampled(spp) and esc_render_adaptive(spp, T) for T in
  0.02, 0.05, 0.1, all into device buffers, with the refined fraction beside every adaptive time and the
  model  t_render + fraction * t_supersampled  it is compared with.
HIP events on the renderer's stream, warm-up first; the variants alternate inside every round and every
round is printed (sorted), so the run-to-run spread is visible.  Prints one JSON line.
    python tools/adaptive_time.py [spp=16] [rounds=5] [scale=1.0]     (scale shrinks both frames)"""
import ctypes as C
import json
import os
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi

THRESHOLDS = (0.02, 0.05, 0.1)


def water_box():
    tmp = tempfile.mkdtemp()
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        t.extractall(tmp, filter="data") if hasattr(tarfile, "data_filter") else t.extractall(tmp)
    return esc.Scene.load_obj(os.path.join(tmp, "cornell", "CornellBox-Water.obj"))


def event_ms(st, fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1)


def measure(r, st, dev, name, scene, view, W, H, spp, rounds):
    r.upload(scene)
    cam = esc.Camera.for_image(*view, W, H)
    opt = esc._options(True, esc.ESC_FACE_FIXED, 0, 0, esc.ESC_STAGE_AUTO, 0, 0)
    with torch.cuda.stream(st):
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    st.synchronize()
    p_img = C.c_void_p(img.data_ptr())
    lib, h = r._lib, r._h

    def render():
        esc.check(lib.esc_render_rows(h, C.byref(cam.c), W, H, 0, H, C.byref(opt), p_img, None))

    def supersampled():
        esc.check(lib.esc_render_supersampled(h, C.byref(cam.c), W, H, spp, C.byref(opt), p_img, None))

    def adaptive(threshold):
        a = _capi.esc_adaptive_options(spp, threshold, 0, 0)
        return lambda: esc.check(lib.esc_render_adaptive(h, C.byref(cam.c), W, H, C.byref(opt), C.byref(a), p_img,
                                                         None, None))

    variants = [("render", render), ("supersampled", supersampled)] + \
        [(f"adaptive_{t}", adaptive(t)) for t in THRESHOLDS]
    fraction = {}
    for key, fn in variants:  # warm-up of every shape and code path; the refined fractions
        fn()
        st.synchronize()
        if key.startswith("adaptive"):
            s = r.adaptive_stats()
            fraction[key] = s["refined_pixels"] / s["pixels"]
    ms = {key: [] for key, _ in variants}
    for _ in range(rounds):
        for key, fn in variants:
            ms[key].append(event_ms(st, fn))
    med = {key: sorted(v)[len(v) // 2] for key, v in ms.items()}
    rows = []
    for key, _ in variants:
        row = {"call": key, "ms_median": round(med[key], 4), "ms_all": [round(x, 4) for x in sorted(ms[key])]}
        if key in fraction:
            row["refined_fraction"] = round(fraction[key], 5)
            row["model_ms"] = round(med["render"] + fraction[key] * med["supersampled"], 4)
            row["over_model"] = round(med[key] / row["model_ms"], 3)
            row["vs_supersampled"] = round(med["supersampled"] / med[key], 2)
        rows.append(row)
    return {"scene": name, "W": W, "H": H, "spp": spp, "rounds": rounds, "calls": rows}


def main():
    spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    scale = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    out = []
    for name, scene, view, W, H in (("c4", esc.Scene.synthetic("c4"), esc.synthetic_view(), 3840, 2160),
                                    ("CornellBox-Water", water_box(), ((0, 1, 3.5), (0, 1, 0)), 1920, 1080)):
        W, H = max(2, int(W * scale)), max(2, int(H * scale))
        out.append(measure(r, st, dev, name, scene, view, W, H, spp, rounds))
        print(f"{name} done", file=sys.stderr, flush=True)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
