"""Developer tool: cost of ambient occlusion (esc_render_ambient / esc_ambient_rays) next to the path a caller
had to compose before: intersect_rays, normals and sample rays in torch, occluded_rays on the n x K rays.
  c4 at 1920 x 1080 and CornellBox-Water (tests/golden/cornell_models.tar.gz) at 960 x 540, K = 16,
  S in {1, 16}, radius 0.25 x the scene's extent and unbounded.  Per configuration:
    fused_frame     esc_render_ambient (the rays made in the kernel)
    fused_rays      esc_ambient_rays on esc_camera_rays' rays
    fused_no_stats  esc_render_ambient with ESC_AMBIENT_STATS=0 (no counters, no atomics)
    composed        esc_intersect_rays + [torch glue] + esc_occluded_rays on the same hit x K sample rays; the
                    two library calls are timed apart from the glue
HIP events on the renderer's stream, warm-up first, median / min / max of the repetitions.  The verdict per
configuration: fused_frame's median minus the composed LIBRARY calls' median, against the spread (max - min)
of the composed library calls' own repetitions.  Prints one JSON line.
    python tools/ambient_time.py [reps=5] [scale=1.0] [scenes=c4,water]     (scale scales both frames)"""
import ctypes as C
import json
import os
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import esctp1raytracer_amd as esc
from esctp1raytracer_amd import _capi

K = 16
FLT_MAX = float(np.finfo(np.float32).max)
BIAS = 1e-4


def water_box():
    tmp = tempfile.mkdtemp()
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        t.extractall(tmp, filter="data") if hasattr(tarfile, "data_filter") else t.extractall(tmp)
    return esc.Scene.load_obj(os.path.join(tmp, "cornell", "CornellBox-Water.obj"))


def mix_hi32(seed, pixel, light):
    U = np.uint64
    with np.errstate(over="ignore"):
        z = U(seed) + ((pixel.astype(U) << U(32)) | U(light)) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
    return (z >> U(32)).astype(np.uint32)


def scene_tensors(sc, dev):
    """the geometry the glue needs on the device: triangles (vertices, vertex normals or zeros, a flag),
    the first triangle of every geometry, spheres -> dict, and the scene's extent"""
    info = sc.info()
    V, NV, flag, first, pts = [], [], [], [], []
    n = 0
    for g in range(info["n_geometry"]):
        G = sc.geometry(g)
        f = G["face_index"].astype(np.int64)
        first.append(n)
        n += len(f)
        if not len(f):
            continue
        V.append(G["vertex"][f])
        has = len(G["normals"]) > 0
        NV.append(G["normals"][f] if has else np.zeros((len(f), 3, 3), np.float32))
        flag.append(np.full(len(f), has))
        pts.append(G["vertex"])
    sp, _ = sc.spheres()
    if len(sp):
        pts += [sp[:, :3] - sp[:, 3:], sp[:, :3] + sp[:, 3:]]
    p = np.concatenate(pts)
    cat = lambda a, shape: np.concatenate(a) if a else np.zeros(shape, np.float32)  # noqa: E731
    t = {"V": torch.from_numpy(cat(V, (1, 3, 3))).to(dev), "NV": torch.from_numpy(cat(NV, (1, 3, 3))).to(dev),
         "flag": torch.from_numpy(np.concatenate(flag) if flag else np.zeros(1, bool)).to(dev),
         "first": torch.tensor(first or [0], dtype=torch.int64, device=dev),
         "sph": torch.from_numpy(sp if len(sp) else np.zeros((1, 4), np.float32)).to(dev)}
    return t, float(np.max(p.max(0) - p.min(0)))


def unit(v):
    return v / torch.sqrt((v * v).sum(-1, keepdim=True))


def glue(T, o, d, t, geom, prim, uv, sets, table, radius):
    """the caller's side of the composed path: normals of the hits, the frame, the hit x K sample rays"""
    hit = (geom >= 0) | (prim >= 0)
    idx = torch.nonzero(hit).squeeze(1)
    o, d, t, geom, prim, v = o[idx], d[idx], t[idx], geom[idx], prim[idx], uv[idx, 1]
    tri = geom >= 0
    tid = (T["first"][geom.clamp(min=0).long()] + prim.long()).clamp(0, T["V"].shape[0] - 1)
    tid = torch.where(tri, tid, torch.zeros_like(tid))
    Vt = T["V"][tid]
    Nface = unit(torch.linalg.cross(Vt[:, 1] - Vt[:, 0], Vt[:, 2] - Vt[:, 0]))
    NVt = T["NV"][tid]
    Nv = unit(NVt[:, 2] * v[:, None] + NVt[:, 0] * (1.0 - v)[:, None])  # quirk S1: u == 0
    N = torch.where(T["flag"][tid][:, None], Nv, Nface)
    P0 = o + d * t[:, None]
    sp = T["sph"][torch.where(tri, torch.zeros_like(prim), prim).long().clamp(0, T["sph"].shape[0] - 1)]
    N = torch.where(tri[:, None], N, unit(P0 - sp[:, :3]))
    sn = (d * N).sum(-1)
    Nf = torch.where((sn > 0)[:, None], -N, N)
    P = P0 + Nf * BIAS
    x, y, z = Nf[:, 0], Nf[:, 1], Nf[:, 2]
    sg = torch.copysign(torch.ones_like(z), z)
    a = -1.0 / (sg + z)
    b = x * y * a
    Tt = torch.stack([1.0 + sg * x * x * a, sg * b, -sg * x], -1)
    Bt = torch.stack([b, sg + y * y * a, -y], -1)
    l = table[sets[idx]]  # noqa: E741  (nh, K, 3)
    w = unit(Tt[:, None] * l[..., 0:1] + Bt[:, None] * l[..., 1:2] + Nf[:, None] * l[..., 2:3]).reshape(-1, 3)
    so = P[:, None, :].expand(-1, l.shape[1], -1).reshape(-1, 3).contiguous()
    return idx, so, w.contiguous(), torch.full((so.shape[0],), radius, dtype=torch.float32, device=so.device)


def stats_of(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def timed(st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1)


def measure(r, st, dev, name, sc, view, W, H, reps, out):
    r.upload(sc)
    T, extent = scene_tensors(sc, dev)
    cam = esc.Camera.for_image(*view, W, H)
    n = W * H
    lib, h = r._lib, r._h
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.stream(st):
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

            def fused_frame():
                esc.check(lib.esc_render_ambient(h, C.byref(cam.c), W, H, C.byref(o), p(vis), p(cnt)))

            def fused_rays():
                esc.check(lib.esc_ambient_rays(h, n, p(to), p(td), C.byref(o), p(vis), p(cnt), None, None, None))

            res = {"scene": name, "W": W, "H": H, "K": K, "S": S, "radius": rname}
            fused_frame()  # warm-up, and the counts of this configuration
            s = r.ambient_stats()
            res.update(hit_rays=s["hit_rays"], samples=s["samples"], occluded_samples=s["occluded_samples"],
                       exact_rays=s["exact_rays"], mean_vis=round(float(vis.mean().item()), 5))
            res["fused_frame_ms"] = stats_of([timed(st, fused_frame) for _ in range(reps)])
            fused_rays()
            res["fused_rays_ms"] = stats_of([timed(st, fused_rays) for _ in range(reps)])
            os.environ["ESC_AMBIENT_STATS"] = "0"
            fused_frame()
            res["fused_no_stats_ms"] = stats_of([timed(st, fused_frame) for _ in range(reps)])
            del os.environ["ESC_AMBIENT_STATS"]
            # the composed path, library calls timed apart from the glue
            lib_ms, glue_ms, comp_occ = [], [], 0
            for k in range(reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                with torch.cuda.stream(st):
                    ev[0].record(st)
                    r.intersect_rays(to, td, t, geom, prim, uv=uv)
                    ev[1].record(st)
                    idx, so, sd, tm = glue(T, to, td, t, geom, prim, uv, sets, table, radius)
                    occ = torch.empty(so.shape[0], dtype=torch.uint8, device=dev)
                    ev[2].record(st)
                    r.occluded_rays(so, sd, occ, tmax=tm)
                    ev[3].record(st)
                st.synchronize()
                if k:  # the first round is the warm-up
                    lib_ms.append(ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]))
                    glue_ms.append(ev[1].elapsed_time(ev[2]))
                comp_occ = int(occ.sum().item())
                del so, sd, tm, occ
            res["composed_lib_ms"] = stats_of(lib_ms)
            res["composed_glue_ms"] = stats_of(glue_ms)
            res["composed_occluded_samples"] = comp_occ  # torch's rounding of the glue may move a few samples
            spread = res["composed_lib_ms"]["max"] - res["composed_lib_ms"]["min"]
            diff = res["fused_frame_ms"]["median"] - res["composed_lib_ms"]["median"]
            res["fused_minus_composed_lib_ms"] = round(diff, 4)
            res["composed_lib_spread_ms"] = round(spread, 4)
            res["fused_not_slower_beyond_spread"] = bool(diff <= spread)
            out["results"].append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    if reps < 5:
        raise SystemExit("at least 5 repetitions")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    r = esc.Renderer(0, stream=st)
    scenes = (sys.argv[3] if len(sys.argv) > 3 else "c4,water").split(",")
    out = {"K": K, "reps": reps, "bias": BIAS, "scale": scale, "results": []}
    if "c4" in scenes:
        measure(r, st, dev, "c4", esc.Scene.synthetic("c4"), esc.synthetic_view(), int(1920 * scale),
                int(1080 * scale), reps, out)
    if "water" in scenes:
        measure(r, st, dev, "CornellBox-Water", water_box(), ((0, 1, 3.5), (0, 1, 0)), int(960 * scale),
                int(540 * scale), reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
