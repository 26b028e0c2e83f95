"""esctp1raytracer_amd -- MI355X-native drop-in for the per-pixel render loop of
pg42819/EscTp1RayTracer.

Python here is a thin host mirror over the C ABI (include/esctp1_rt.h, libesctp1rt.so);
all rendering happens in hand-written HIP kernels for gfx950.  Names follow the reference:
`Scene` ~ tracer::scene (scene.h), `Scene.load_obj` ~ model::loadobj (sceneloader.h:10),
`Camera` ~ tracer::camera (camera.h), `Renderer.render_rows` ~ the scan_row row loop
(main.cpp:628-636), `trace` ~ ispc::trace (trace.ispc:86-92), `write_ppm` ~ main.cpp:658-689.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (ESC_FACE_FIXED, ESC_FACE_HASH, ESC_STAGE_AUTO, ESC_STAGE_BVH, ESC_STAGE_LDS,
                    ESC_RENDER_EXACT_ONLY, ESC_RENDER_INDEX_ORDER, ESC_RENDER_SHADE_FUSED,
                    ESC_RENDER_SHADE_QUEUE, ESC_RENDER_TIME_KERNELS, ESC_RENDER_NO_TILE_LISTS, ESC_RENDER_NO_LIGHT_LISTS, ESC_RENDER_TWO_KERNELS, ESC_RENDER_BVH_HEURISTIC_PADS, ESC_RENDER_NO_COUNTERS, ESC_RENDER_NO_PACKED_LIGHT_LISTS, ESC_RENDER_VOTE,
                    ESC_STAGE_SMEM, ESC_TRANSMIT_OFF, ESC_TRANSMIT_REFRACT, ESC_TRANSMIT_FRESNEL, EscError,
                    check)

__all__ = ["Scene", "Camera", "Renderer", "RecordedFrame", "TemporalAccumulator", "FlatScene", "MultiRenderer", "render_multi", "render_multi_rccl", "rccl_available", "strip_local_rows", "live_device_allocations", "trace", "write_ppm", "quantise", "synthetic_view", "ambient_table", "lens_table", "environment_sky", "environment_lookup_host",
           "EscError", "ESC_FACE_FIXED", "ESC_FACE_HASH", "ESC_STAGE_AUTO", "ESC_STAGE_SMEM",
           "ESC_STAGE_LDS", "ESC_STAGE_BVH", "ESC_RENDER_EXACT_ONLY", "ESC_RENDER_TIME_KERNELS", "ESC_RENDER_INDEX_ORDER", "ESC_RENDER_SHADE_QUEUE",
           "ESC_RENDER_SHADE_FUSED", "ESC_RENDER_NO_TILE_LISTS", "ESC_RENDER_NO_LIGHT_LISTS", "ESC_RENDER_TWO_KERNELS", "ESC_RENDER_BVH_HEURISTIC_PADS", "ESC_RENDER_NO_COUNTERS", "ESC_RENDER_NO_PACKED_LIGHT_LISTS", "ESC_RENDER_VOTE", "ESC_TRANSMIT_OFF", "ESC_TRANSMIT_REFRACT", "ESC_TRANSMIT_FRESNEL", "version"]


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


_TRANSMIT_MODES = {"off": ESC_TRANSMIT_OFF, "refract": ESC_TRANSMIT_REFRACT, "fresnel": ESC_TRANSMIT_FRESNEL}


def _transmit_mode(transmission):
    try:
        return _TRANSMIT_MODES[transmission]
    except (KeyError, TypeError):
        raise ValueError(f"transmission must be 'off', 'refract' or 'fresnel', not {transmission!r}") from None


def version():
    return _capi.load().esc_version().decode()


class Scene:
    """Host scene: geometries (de-indexed triangles + one material), light list, spheres."""

    def __init__(self):
        self._lib = _capi.load()
        self._h = self._lib.esc_scene_new()
        if not self._h:
            raise MemoryError("esc_scene_new")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.esc_scene_free(h)

    # -- building -------------------------------------------------------------------
    def add_geometry(self, vertex, face_index, material, normals=None):
        v = _f32(vertex, (-1, 3))
        f = np.ascontiguousarray(face_index, dtype=np.uint32).reshape(-1, 3)
        m = _f32(material, (13,))
        if normals is None or len(normals) == 0:
            n, nn = None, 0
        else:
            n = _f32(normals, (-1, 3))
            nn = n.shape[0]
        return check(self._lib.esc_scene_add_geometry(
            self._h, _fp(v), v.shape[0], _fp(n) if n is not None else None, nn,
            f.ctypes.data_as(C.POINTER(C.c_uint32)), f.shape[0], _fp(m)))

    def add_spheres(self, spheres_xyzr, materials):
        s = _f32(spheres_xyzr, (-1, 4))
        m = _f32(materials, (-1, 13))
        if s.shape[0] != m.shape[0]:
            raise ValueError("one material per sphere")
        check(self._lib.esc_scene_add_spheres(self._h, _fp(s), _fp(m), s.shape[0]))

    @classmethod
    def load_obj(cls, path):
        """model::loadobj (sceneloader.cpp:14-106)."""
        sc = cls()
        check(sc._lib.esc_scene_load_obj(sc._h, str(path).encode()))
        return sc

    @classmethod
    def synthetic(cls, config, n_override=0):
        """BASELINE.json workloads: 'c2' | 'c3' | 'c4' | 'c5' (SURVEY.md 8(d))."""
        sc = cls()
        check(sc._lib.esc_scene_synthetic(sc._h, config.encode(), int(n_override)))
        return sc

    # -- introspection --------------------------------------------------------------
    def info(self):
        i = _capi.esc_scene_info()
        check(self._lib.esc_scene_get_info(self._h, C.byref(i)))
        return {"n_geometry": i.n_geometry, "n_lights": i.n_lights,
                "n_triangles": i.n_triangles, "n_spheres": i.n_spheres}

    def geometry(self, g):
        cnt = (C.c_int32 * 3)()
        check(self._lib.esc_scene_geometry_counts(self._h, g, cnt))
        nv, nn, nf = cnt[0], cnt[1], cnt[2]
        v = np.zeros((nv, 3), np.float32)
        n = np.zeros((nn, 3), np.float32)
        f = np.zeros((nf, 3), np.uint32)
        m = np.zeros(13, np.float32)
        check(self._lib.esc_scene_geometry_copy(
            self._h, g, _fp(v), _fp(n) if nn else None,
            f.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(m)))
        return {"vertex": v, "normals": n, "face_index": f, "material": m}

    def light_sources(self):
        n = self.info()["n_lights"]
        out = np.zeros(max(n, 1), np.int32)
        check(self._lib.esc_scene_light_sources(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:n].copy()

    def spheres(self):
        n = self.info()["n_spheres"]
        s = np.zeros((n, 4), np.float32)
        m = np.zeros((n, 13), np.float32)
        if n:
            check(self._lib.esc_scene_spheres_copy(self._h, _fp(s), _fp(m)))
        return s, m

    # -- transmission (extension: the side table of esc_trace_rays_ex) -----------------
    def set_transmission(self, geom, tf, ni):
        """tf (3 floats, the MTL's Tf) and ni (its Ni) of geometry `geom`; tf = 0, ni = 1 is opaque."""
        t = np.concatenate([_f32(tf, (3,)), _f32([ni], (1,))])
        check(self._lib.esc_scene_set_geometry_transmission(self._h, int(geom), _fp(t)))

    def set_sphere_transmission(self, first, tf, ni):
        """tf (n x 3) and ni (n) of spheres first .. first + n - 1."""
        tf = _f32(tf, (-1, 3))
        ni = _f32(ni, (-1,))
        if tf.shape[0] != ni.shape[0]:
            raise ValueError("one ni per tf")
        t = np.ascontiguousarray(np.concatenate([tf, ni[:, None]], axis=1))
        check(self._lib.esc_scene_set_sphere_transmission(self._h, int(first), t.shape[0], _fp(t)))

    def transmission(self, geom):
        """(tf, ni) of geometry `geom`"""
        t = np.zeros(4, np.float32)
        check(self._lib.esc_scene_get_geometry_transmission(self._h, int(geom), _fp(t)))
        return t[:3].copy(), t[3]

    def sphere_transmission(self):
        """(tf (n x 3), ni (n)) of the spheres"""
        t = np.zeros((self.info()["n_spheres"], 4), np.float32)
        if len(t):
            check(self._lib.esc_scene_get_sphere_transmission(self._h, _fp(t)))
        return t[:, :3].copy(), t[:, 3].copy()

    def build_accel(self, origin, which):
        """Host-side build of the ESC_STAGE_BVH tree (no GPU needed): which = 'triangles' |
        'spheres'.  Returns nodes (structured array), order (block slot -> primitive index, -1 =
        pad), the padded primitive boxes (n, 2, 3) and the build summary."""
        w = {"triangles": 0, "spheres": 1}[which]
        o = _f32(origin, (3,))
        info = _capi.esc_accel_info()
        check(self._lib.esc_scene_build_accel(self._h, _fp(o), w, C.byref(info), None, 0, None, 0,
                                              None, 0))
        n_nodes = info.sph_nodes if w else info.tri_nodes
        n_blocks = info.sph_blocks if w else info.tri_blocks
        block = 4 if w else 2
        n_prims = self.info()["n_spheres" if w else "n_triangles"]
        node_dt = np.dtype([("lo0", np.float32, 3), ("hi0", np.float32, 3), ("lo1", np.float32, 3),
                            ("hi1", np.float32, 3), ("child", np.int32, 2),
                            ("minkey", np.uint32, 2)])
        nodes = np.zeros(max(n_nodes, 1), node_dt)
        order = np.full(max(n_blocks * block, 1), -1, np.int32)
        boxes = np.zeros((max(n_prims, 1), 2, 3), np.float32)
        check(self._lib.esc_scene_build_accel(
            self._h, _fp(o), w, C.byref(info),
            nodes.ctypes.data_as(C.POINTER(_capi.esc_bvh_node)), nodes.shape[0],
            order.ctypes.data_as(C.POINTER(C.c_int32)), order.shape[0], _fp(boxes),
            boxes.size))
        return {"nodes": nodes[:n_nodes], "order": order[:n_blocks * block],
                "boxes": boxes[:n_prims], "block": block,
                "root": info.sph_root if w else info.tri_root,
                "depth": info.sph_depth if w else info.tri_depth, "build_ms": info.build_ms}

    def table(self, name):
        """Host only (no GPU needed): one of the tables an upload of this scene computes, as the
        bytes it uploads (numpy.uint8).  `name` is one of _capi.ESC_TABLE_NAMES: the staged records,
        the computed tables (csrc/rt_device.h layouts), or "header" (esc_scene_table_header)."""
        which = _capi.ESC_TABLE_NAMES.index(name)
        out = np.zeros(check(self._lib.esc_scene_table(self._h, which, None, 0)), np.uint8)
        check(self._lib.esc_scene_table(self._h, which, out.ctypes.data, out.size))
        return out

    def shadow_origins_inside(self, origin):
        """Host only: esc_scene_shadow_origins_inside -- True when every shadow-ray origin of a camera at
        `origin` provably lies in the scene's grown box."""
        o = _f32(origin, (3,))
        return bool(check(self._lib.esc_scene_shadow_origins_inside(self._h, _fp(o))))

    def flatten_ispc(self, sort_by_centroid_x=False):
        """flatten_scene_ispc (flatten_iscp.cpp:35-111) -> FlatScene."""
        return FlatScene(self, sort_by_centroid_x)


class FlatScene:
    """FlatScene of flatten_iscp.h:9-13: ispc_triangle[] / ispc_light[] / light faces."""

    def __init__(self, scene, sort_by_centroid_x=False):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        check(self._lib.esc_flatten_ispc(scene._h, 1 if sort_by_centroid_x else 0,
                                         C.byref(self._h)))
        n = C.c_int32()
        self.triangles = self._lib.esc_flat_triangles(self._h, C.byref(n))
        self.num_triangles = n.value
        self.light_triangles = self._lib.esc_flat_light_triangles(self._h, C.byref(n))
        self.num_light_triangles = n.value
        self.lights = self._lib.esc_flat_lights(self._h, C.byref(n))
        self.num_lights = n.value

    def check(self):
        """esc_check_flat: host-only validation of what `trace` would stage (raises EscError)."""
        check(self._lib.esc_check_flat(self.num_triangles, self.triangles, self.num_lights,
                                       self.lights, self.num_light_triangles,
                                       self.light_triangles))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.esc_flat_free(h)


class Camera:
    """tracer::camera (camera.h:16-29): the four vectors get_ray needs, computed on the host."""

    def __init__(self, lookfrom, lookat, vup=(0.0, 1.0, 0.0), vfov=60.0, aspect=4.0 / 3.0):
        self.lookfrom = _f32(lookfrom, (3,))
        self.lookat = _f32(lookat, (3,))
        self.vup = _f32(vup, (3,))
        self.vfov = float(np.float32(vfov))
        self.aspect = float(np.float32(aspect))
        self.c = _capi.esc_camera()
        _capi.load().esc_camera_init(C.byref(self.c), _fp(self.lookfrom), _fp(self.lookat),
                                     _fp(self.vup), self.vfov, self.aspect)

    @classmethod
    def for_image(cls, lookfrom, lookat, W, H, vup=(0.0, 1.0, 0.0), vfov=60.0):
        # main.cpp:548  float aspect = float(image_width) / image_height;
        return cls(lookfrom, lookat, vup, vfov, np.float32(W) / np.float32(H))

    def vectors(self):
        return {k: np.array(getattr(self.c, k), np.float32)
                for k in ("origin", "lower_left_corner", "horizontal", "vertical")}


def synthetic_view():
    eye = np.zeros(3, np.float32)
    look = np.zeros(3, np.float32)
    _capi.load().esc_synthetic_view(_fp(eye), _fp(look))
    return eye, look


def ambient_table(sets, samples, seed=0):
    """esc_ambient_cosine_table: (sets, samples, 3) float32 cosine-weighted unit vectors about +z, made on the
    host (no GPU needed) and deterministic in (sets, samples, seed).  Renderer.set_ambient_table takes it,
    or any other array of local directions of that shape."""
    out = np.zeros((int(sets), int(samples), 3), np.float32) if sets > 0 and samples > 0 else np.zeros(3, np.float32)
    check(_capi.load().esc_ambient_cosine_table(int(sets), int(samples), int(seed) & (2 ** 64 - 1), _fp(out)))
    return out


def lens_table(sets, samples, seed=0):
    """esc_lens_disk_table: (sets, samples, 2) float32 points of the unit disk, made on the host (no GPU
    needed) and deterministic in (sets, samples, seed): jittered over a grid when samples is a square, mapped
    concentrically onto the disk, shuffled inside each set.  Renderer.set_lens_table takes it, or any other
    array of lens points of that shape."""
    out = np.zeros((int(sets), int(samples), 2), np.float32) if sets > 0 and samples > 0 else np.zeros(2, np.float32)
    check(_capi.load().esc_lens_disk_table(int(sets), int(samples), int(seed) & (2 ** 64 - 1), _fp(out)))
    return out


def environment_sky(res, zenith, horizon, ground):
    """esc_environment_sky: a vertical gradient (zenith above, horizon, ground below) as an environment cube,
    (6, res, res, 3) float32, made on the host (no GPU needed) in double arithmetic without transcendentals.
    Renderer.set_environment takes it, or any other array of that shape."""
    res = int(res)
    out = np.zeros((6, res, res, 3), np.float32) if 1 <= res <= 1024 else np.zeros(3, np.float32)
    check(_capi.load().esc_environment_sky(res, _fp(_f32(zenith, (3,))), _fp(_f32(horizon, (3,))),
                                           _fp(_f32(ground, (3,))), _fp(out)))
    return out


def environment_lookup_host(cube, dirs):
    """esc_environment_lookup_host: env(d) of include/esctp1_rt.h for numpy directions (n, 3) on the host, by
    the code the kernels run.  cube: (6, R, R, 3) float32.  -> (n, 3) float32"""
    t = np.ascontiguousarray(cube, dtype=np.float32)
    if t.ndim != 4 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or t.shape[3] != 3:
        raise ValueError("cube must have shape (6, R, R, 3)")
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(d)
    check(_capi.load().esc_environment_lookup_host(t.shape[1], _fp(t), d.shape[0], _fp(d), _fp(out)))
    return out


FLT_MAX = float(np.finfo(np.float32).max)


def _options(shadows, face_mode, fixed_face, seed, stage, px=0, flags=0):
    o = _capi.esc_render_options()
    o.pixels_per_lane = px
    o.flags = flags
    o.shadows = 1 if shadows else 0
    o.face_mode = face_mode
    o.fixed_face = fixed_face
    o.stage = stage
    o.seed = seed
    return o


class Renderer:
    """Device context: one per GPU / host thread.  Raises EscError(ESC_ERR_NO_DEVICE) when no
    GPU is present -- there is no CPU fallback."""

    def __init__(self, device=0, stream=None):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        check(self._lib.esc_context_create(int(device), C.byref(self._h)))
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        self.close()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.esc_context_destroy(h)

    def set_stream(self, stream):
        """stream: a raw hipStream_t (int) or an object with .cuda_stream (torch.cuda.Stream)."""
        ptr = getattr(stream, "cuda_stream", stream)
        check(self._lib.esc_context_set_stream(self._h, C.c_void_p(int(ptr))))

    def stream_handle(self):
        return self._lib.esc_context_stream(self._h)

    def synchronize(self):
        check(self._lib.esc_context_synchronize(self._h))

    def upload(self, scene):
        if isinstance(scene, FlatScene):
            check(self._lib.esc_upload_flat(self._h, scene.num_triangles, scene.triangles,
                                            scene.num_lights, scene.lights,
                                            scene.num_light_triangles, scene.light_triangles))
        else:
            check(self._lib.esc_upload_scene(self._h, scene._h))

    def render_rows(self, camera, W, H, row_begin, row_end, out_f32=None, out_u8=None, *,
                    shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0,
                    stage=ESC_STAGE_AUTO, px=0, flags=0):
        """Asynchronous band render into DEVICE buffers (torch tensors or raw pointers),
        band-local layout ((h - row_begin) * W + w) * 3."""
        n = max(0, row_end - row_begin) * W * 3
        o = _options(shadows, face_mode, fixed_face, seed, stage, px, flags)
        check(self._lib.esc_render_rows(self._h, C.byref(camera.c), W, H, row_begin, row_end,
                                        C.byref(o), self._dev_ptr(out_f32, n * 4), self._dev_ptr(out_u8, n)))

    @staticmethod
    def _dev_ptr(buf, nbytes):
        if buf is None:
            return None
        if hasattr(buf, "data_ptr"):
            if buf.numel() * buf.element_size() < nbytes:
                raise ValueError("device buffer too small")
            if not buf.is_cuda or not buf.is_contiguous():
                raise ValueError("need a contiguous device tensor")
            return C.c_void_p(buf.data_ptr())
        return C.c_void_p(int(buf))

    def render_strips(self, camera, W, H, first_strip, strip_stride, out_f32=None, out_u8=None, *,
                      strip_rows=8, shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0,
                      stage=ESC_STAGE_AUTO, px=0, flags=0):
        """Rank `first_strip` of `strip_stride`: renders strips first, first+stride, ... of
        `strip_rows` rows (counted from h = 0) into device buffers, rows packed in ascending h.
        Returns the number of rows rendered."""
        rows = strip_local_rows(H, strip_rows, first_strip, strip_stride)
        n = rows * W * 3
        o = _options(shadows, face_mode, fixed_face, seed, stage, px, flags)
        check(self._lib.esc_render_strips(self._h, C.byref(camera.c), W, H, strip_rows,
                                          first_strip, strip_stride, C.byref(o),
                                          self._dev_ptr(out_f32, n * 4), self._dev_ptr(out_u8, n)))
        return rows

    def record_strips(self, camera, W, H, first_strip, strip_stride, out_f32=None, out_u8=None, *,
                      strip_rows=8, shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0,
                      stage=ESC_STAGE_AUTO, px=0, flags=0):
        """esc_frame_record: the launches of this render_strips call captured into a HIP graph.
        Returns a RecordedFrame; .launch() replays it with one host call."""
        rows = strip_local_rows(H, strip_rows, first_strip, strip_stride)
        n = rows * W * 3
        o = _options(shadows, face_mode, fixed_face, seed, stage, px, flags)
        h = C.c_void_p()
        check(self._lib.esc_frame_record(self._h, C.byref(camera.c), W, H, strip_rows, first_strip,
                                         strip_stride, C.byref(o), self._dev_ptr(out_f32, n * 4),
                                         self._dev_ptr(out_u8, n), C.byref(h)))
        return RecordedFrame(self._lib, h, (self, out_f32, out_u8))

    def assemble_strips(self, gathered, n_ranks, rank_pitch_bytes, W, H, frame, *, strip_rows=8,
                        bytes_per_pixel=12):
        """gathered: n_ranks blocks of local rows (block r at r*rank_pitch_bytes) -> frame."""
        need = 0  # the end of the last local row the kernel reads, over the ranks
        if hasattr(gathered, "data_ptr") and n_ranks >= 1 and strip_rows >= 1:
            n_strips = (H + strip_rows - 1) // strip_rows
            for r in range(min(n_ranks, n_strips)):
                rows = (n_strips - r + n_ranks - 1) // n_ranks * strip_rows
                if (n_strips - 1) % n_ranks == r:  # the image's last strip may be short
                    rows -= n_strips * strip_rows - H
                need = max(need, r * rank_pitch_bytes + rows * W * bytes_per_pixel)
        check(self._lib.esc_assemble_strips(
            self._h, self._dev_ptr(gathered, need), n_ranks, rank_pitch_bytes, W, H, strip_rows,
            bytes_per_pixel, self._dev_ptr(frame, W * H * bytes_per_pixel)))

    def render(self, camera, W, H, *, want_u8=False, shadows=True, face_mode=ESC_FACE_FIXED,
               fixed_face=0, seed=0, stage=ESC_STAGE_AUTO, px=0, flags=0, out=None):
        """Whole frame into host numpy arrays (synchronous): fp32 (H, W, 3), h = 0 bottom row,
        and optionally the PPM-quantised bytes.  `out`: a C-contiguous float32 (H, W, 3) array to
        render into (a fresh np.zeros of a 4K frame costs more in first-touch page faults than the
        frame and its copy back together)."""
        if out is not None:
            if out.dtype != np.float32 or out.shape != (H, W, 3) or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous float32 array of shape (H, W, 3)")
            img = out
        else:
            img = np.zeros((H, W, 3), np.float32)
        u8 = np.zeros((H, W, 3), np.uint8) if want_u8 else None
        o = _options(shadows, face_mode, fixed_face, seed, stage, px, flags)
        check(self._lib.esc_render_frame_host(
            self._h, C.byref(camera.c), W, H, C.byref(o), _fp(img),
            u8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_u8 else None))
        return (img, u8) if want_u8 else img

    def build_accel(self, origin):
        """Build (or rebuild) the ESC_STAGE_BVH tree now instead of at the first frame that
        asks for it."""
        o = _f32(origin, (3,))
        check(self._lib.esc_build_accel(self._h, _fp(o)))
        return self.accel_info()

    def accel_info(self):
        i = _capi.esc_accel_info()
        check(self._lib.esc_get_accel_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k in ("tri_nodes", "tri_blocks", "tri_depth", "tri_root",
                                           "sph_nodes", "sph_blocks", "sph_depth", "sph_root",
                                           "build_ms", "builds")}

    def last_kernel_ms(self):
        """(k_primary ms, k_shade ms) of the last frame rendered with ESC_RENDER_TIME_KERNELS."""
        ms = np.zeros(2, np.float32)
        check(self._lib.esc_last_kernel_ms(self._h, _fp(ms)))
        return float(ms[0]), float(ms[1])

    def last_frame_kernel(self):
        """esc_last_frame_kernel: the ESC_FRAME_KERNEL_* bits of the one-kernel frame the last frame
        launched (0: it took another path), as a dict of booleans."""
        bits = check(self._lib.esc_last_frame_kernel(self._h))
        return {"fused": bool(bits & _capi.ESC_FRAME_KERNEL_FUSED), "grp": bool(bits & _capi.ESC_FRAME_KERNEL_GRP),
                "tgrp": bool(bits & _capi.ESC_FRAME_KERNEL_TGRP), "idl": bool(bits & _capi.ESC_FRAME_KERNEL_IDL),
                "sure": bool(bits & _capi.ESC_FRAME_KERNEL_SURE)}

    def frame_tripwire(self):
        """esc_frame_tripwire: reads and clears the "unserved wave in a frame without fallback" word; 0."""
        return check(self._lib.esc_frame_tripwire(self._h))

    def check_inv_det_exact(self, first_bits, n):
        """esc_check_inv_det_exact over the float bit patterns first_bits .. first_bits + n - 1:
        (patterns whose refined reciprocal differs from 1.0 / (double)x, the smallest of them)."""
        bad, first = C.c_uint64(0), C.c_uint32(0)
        check(self._lib.esc_check_inv_det_exact(self._h, int(first_bits) & 0xffffffff, int(n), C.byref(bad),
                                                C.byref(first)))
        return int(bad.value), int(first.value)

    def reset_counters(self):
        check(self._lib.esc_reset_counters(self._h))

    def counters(self):
        c = _capi.esc_counters()
        check(self._lib.esc_read_counters(self._h, C.byref(c)))
        return {"primary_rays": c.primary_rays, "hit_pixels": c.hit_pixels,
                "shadow_rays": c.shadow_rays, "anyhit_tests": c.anyhit_tests,
                "anyhit_lane_tests": c.anyhit_lane_tests}


    # ---- batched ray queries (esc_intersect_rays / esc_occluded_rays) --------------------------
    def _query_ptr(self, name, buf, dtype, shape):
        import torch
        if not isinstance(buf, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor on the renderer's device")
        if buf.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {buf.dtype}")
        if tuple(buf.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(buf.shape)}")
        if not buf.is_cuda or buf.device.index != self.device:
            raise ValueError(f"{name} must be a device tensor on cuda:{self.device}")
        if not buf.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return C.c_void_p(buf.data_ptr())

    def _query_inputs(self, origins, dirs, tmax):
        import torch
        if not hasattr(origins, "shape") or len(origins.shape) != 2:
            raise ValueError("origins must have shape (n, 3)")
        n = int(origins.shape[0])
        po = self._query_ptr("origins", origins, torch.float32, (n, 3))
        pd = self._query_ptr("dirs", dirs, torch.float32, (n, 3))
        pt = None if tmax is None else self._query_ptr("tmax", tmax, torch.float32, (n,))
        return n, po, pd, pt

    def intersect_rays(self, origins, dirs, t, geom, prim, *, tmax=None, uv=None, exact=False):
        """Closest hit of n rays (main.cpp:176-192 with the sphere extension), asynchronous on the
        renderer's stream.  Contiguous device tensors: origins, dirs (n, 3) float32, tmax (n,)
        float32 or None (FLT_MAX); outputs t (n,) float32, geom, prim (n,) int32, uv (n, 2) float32
        or None.  geom / prim: geometry and face of a triangle hit, -1 / k for sphere k, -1 / -1 for
        a miss (t is then the bound).  exact=True: the reference arithmetic for every pair."""
        import torch
        n, po, pd, pt = self._query_inputs(origins, dirs, tmax)
        args = (self._query_ptr("t", t, torch.float32, (n,)),
                self._query_ptr("geom", geom, torch.int32, (n,)),
                self._query_ptr("prim", prim, torch.int32, (n,)),
                None if uv is None else self._query_ptr("uv", uv, torch.float32, (n, 2)))
        check(self._lib.esc_intersect_rays(self._h, n, po, pd, pt, *args,
                                           ESC_RENDER_EXACT_ONLY if exact else 0))

    def occluded_rays(self, origins, dirs, out, *, tmax=None, exact=False):
        """Occlusion of n rays (main.cpp:314-329 with the sphere extension), asynchronous: out (n,)
        uint8 receives 1 where some primitive is hit before the bound, else 0."""
        import torch
        n, po, pd, pt = self._query_inputs(origins, dirs, tmax)
        check(self._lib.esc_occluded_rays(self._h, n, po, pd, pt,
                                          self._query_ptr("out", out, torch.uint8, (n,)),
                                          ESC_RENDER_EXACT_ONLY if exact else 0))

    def _stage(self, origins, dirs, tmax):
        import torch
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and dirs must both have shape (n, 3)")
        dev = torch.device("cuda", self.device)
        to = torch.from_numpy(o).to(dev)
        td = torch.from_numpy(d).to(dev)
        tt = None
        if tmax is not None:
            m = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if m.shape[0] != o.shape[0]:
                raise ValueError("tmax must have n entries")
            tt = torch.from_numpy(m).to(dev)
        # the copies run on torch's stream, the query on the renderer's: order them
        torch.cuda.current_stream(dev).synchronize()
        return to, td, tt

    def intersect(self, origins, dirs, tmax=None, *, exact=False):
        """Synchronous closest hit of numpy rays: {"t", "geom", "prim", "uv"} as numpy arrays."""
        import torch
        to, td, tt = self._stage(origins, dirs, tmax)
        n = to.shape[0]
        dev = to.device
        t = torch.empty(n, dtype=torch.float32, device=dev)
        geom = torch.empty(n, dtype=torch.int32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
        self.intersect_rays(to, td, t, geom, prim, tmax=tt, uv=uv, exact=exact)
        self.synchronize()
        return {"t": t.cpu().numpy(), "geom": geom.cpu().numpy(), "prim": prim.cpu().numpy(),
                "uv": uv.cpu().numpy()}

    def occluded(self, origins, dirs, tmax=None, *, exact=False):
        """Synchronous occlusion of numpy rays: a uint8 array (1 = occluded)."""
        import torch
        to, td, tt = self._stage(origins, dirs, tmax)
        out = torch.empty(to.shape[0], dtype=torch.uint8, device=to.device)
        self.occluded_rays(to, td, out, tmax=tt, exact=exact)
        self.synchronize()
        return out.cpu().numpy()

    def query_stats(self):
        """Counts of the last query call: rays, exact_rays (rays that took the reference loop),
        exact_tests ((ray, primitive) pairs that ran the reference arithmetic).  Synchronises."""
        s = _capi.esc_query_stats()
        check(self._lib.esc_last_query_stats(self._h, C.byref(s)))
        return {"rays": s.rays, "exact_rays": s.exact_rays, "exact_tests": s.exact_tests}

    # ---- shading of caller-supplied rays (esc_camera_rays / esc_shade_rays) -----------------------
    def camera_rays(self, camera, W, H, rows=None, offsets=None):
        """The frame's primary rays as device tensors (origins, dirs), each (n, 3) float32, ray
        (h - r0) * W + w for rows (r0, r1) (None: the whole frame).  offsets: None or a contiguous
        (n, 2) float32 device tensor of sub-pixel offsets (dx, dy).  Asynchronous."""
        import torch
        r0, r1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(0, (r1 - r0) * W)
        dev = torch.device("cuda", self.device)
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        po = None if offsets is None else self._query_ptr("offsets", offsets, torch.float32, (n, 2))
        check(self._lib.esc_camera_rays(self._h, C.byref(camera.c), W, H, r0, r1, po,
                                        C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
        return o, d

    def shade_rays(self, origins, dirs, rgb, *, rgb8=None, t=None, geom=None, prim=None, pixel_base=0,
                   shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, exact=False):
        """scan_row's colour (main.cpp:698-791) of n rays, asynchronous on the renderer's stream.
        Contiguous device tensors: origins, dirs (n, 3) float32; outputs rgb (n, 3) float32, rgb8
        (n, 3) uint8 or None, t (n,) float32, geom, prim (n,) int32 or None (esc_intersect_rays's
        values).  pixel_base: the face_hash pixel index of ray 0.  exact=True: every primary and
        shadow ray through the reference loop."""
        import torch
        n, po, pd, _ = self._query_inputs(origins, dirs, None)
        args = (self._query_ptr("rgb", rgb, torch.float32, (n, 3)),
                None if rgb8 is None else self._query_ptr("rgb8", rgb8, torch.uint8, (n, 3)),
                None if t is None else self._query_ptr("t", t, torch.float32, (n,)),
                None if geom is None else self._query_ptr("geom", geom, torch.int32, (n,)),
                None if prim is None else self._query_ptr("prim", prim, torch.int32, (n,)))
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        check(self._lib.esc_shade_rays(self._h, n, po, pd, int(pixel_base) & 0xffffffff, C.byref(o), *args))

    def shade(self, origins, dirs, *, pixel_base=0, shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0,
              seed=0, exact=False):
        """Synchronous shading of numpy rays: {"rgb", "rgb8", "t", "geom", "prim"} as numpy arrays."""
        import torch
        to, td, _ = self._stage(origins, dirs, None)
        n = to.shape[0]
        dev = to.device
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        geom = torch.empty(n, dtype=torch.int32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        self.shade_rays(to, td, rgb, rgb8=rgb8, t=t, geom=geom, prim=prim, pixel_base=pixel_base,
                        shadows=shadows, face_mode=face_mode, fixed_face=fixed_face, seed=seed, exact=exact)
        self.synchronize()
        return {"rgb": rgb.cpu().numpy(), "rgb8": rgb8.cpu().numpy(), "t": t.cpu().numpy(),
                "geom": geom.cpu().numpy(), "prim": prim.cpu().numpy()}

    def render_supersampled(self, camera, W, H, spp, *, want_u8=False, shadows=True, face_mode=ESC_FACE_FIXED,
                            fixed_face=0, seed=0, exact=False):
        """Anti-aliased frame (esc_render_supersampled): spp = n*n samples per pixel, n in 1..8.
        Returns numpy fp32 (H, W, 3) and optionally the quantised bytes.  Synchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        check(self._lib.esc_render_supersampled(self._h, C.byref(camera.c), W, H, int(spp), C.byref(o),
                                                C.c_void_p(img.data_ptr()),
                                                None if u8 is None else C.c_void_p(u8.data_ptr())))
        self.synchronize()
        return (img.cpu().numpy(), u8.cpu().numpy()) if want_u8 else img.cpu().numpy()

    def shade_stats(self):
        """Counts of the last shade_rays / render_supersampled call: rays, hit_rays, shadow_rays,
        exact_rays (primary or shadow rays that took the reference loop), exact_tests.  Synchronises."""
        s = _capi.esc_shade_stats()
        check(self._lib.esc_last_shade_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k in ("rays", "hit_rays", "shadow_rays", "exact_rays", "exact_tests")}

    def render_adaptive(self, camera, W, H, spp, threshold, *, band_rows=0, want_u8=False, want_mask=False,
                        shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, exact=False):
        """Adaptively anti-aliased frame (esc_render_adaptive): the 1-sample frame, with render_supersampled's
        spp-sample value in every pixel that differs from a 4-neighbour by more than `threshold` in some
        channel.  band_rows: 0 (automatic) or the rows refined per band (a memory knob; same image).
        Returns numpy fp32 (H, W, 3), then the quantised bytes (want_u8) and the uint8 (H, W) mask
        (want_mask) when asked for.  Synchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_mask else None
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        a = _capi.esc_adaptive_options(int(spp), float(threshold), int(band_rows), 0)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        check(self._lib.esc_render_adaptive(self._h, C.byref(camera.c), W, H, C.byref(o), C.byref(a),
                                            C.c_void_p(img.data_ptr()),
                                            None if u8 is None else C.c_void_p(u8.data_ptr()),
                                            None if mask is None else C.c_void_p(mask.data_ptr())))
        self.synchronize()
        out = [img.cpu().numpy()]
        if want_u8:
            out.append(u8.cpu().numpy())
        if want_mask:
            out.append(mask.cpu().numpy())
        return out[0] if len(out) == 1 else tuple(out)

    def adaptive_stats(self):
        """Counts of the last render_adaptive call: pixels, refined_pixels, samples (refined_pixels * spp)
        and, of the refinement rays, hit_rays, shadow_rays, exact_rays, exact_tests.  Synchronises."""
        s = _capi.esc_adaptive_stats()
        check(self._lib.esc_last_adaptive_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("pixels", "refined_pixels", "samples", "hit_rays", "shadow_rays",
                                                "exact_rays", "exact_tests")}

    # ---- ambient occlusion (esc_ambient_rays / esc_render_ambient / esc_modulate) -----------------------
    def set_ambient_table(self, table):
        """esc_set_ambient_table: table is a (sets, samples, 3) float32 array of local directions about +z
        (ambient_table makes a cosine-weighted one), 1 <= sets, samples <= 64.  It belongs to the renderer
        and survives uploads of other scenes.  Its contents are not validated."""
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("table must have shape (sets, samples, 3)")
        check(self._lib.esc_set_ambient_table(self._h, t.shape[0], t.shape[1], _fp(t)))
        self._ambient_shape = (t.shape[0], t.shape[1])

    def _ambient_options(self, samples, sets, radius, bias, seed, pixel_base, exact):
        s0, k0 = getattr(self, "_ambient_shape", (0, 0))
        return _capi.esc_ambient_options(int(k0 if samples is None else samples), int(s0 if sets is None else sets),
                                         float(radius), float(bias), int(seed) & (2 ** 64 - 1),
                                         int(pixel_base) & 0xffffffff, ESC_RENDER_EXACT_ONLY if exact else 0)

    def ambient_rays(self, origins, dirs, vis, *, radius=FLT_MAX, bias=1e-4, count=None, t=None, geom=None,
                     prim=None, samples=None, sets=None, seed=0, pixel_base=0, exact=False):
        """Ambient occlusion of n rays (esc_ambient_rays), asynchronous on the renderer's stream: of the K
        directions of the table's set drawn for each ray, rotated about the hit's normal, how many reach
        `radius` (FLT_MAX: unbounded) from the hit point, moved `bias` off its surface, without meeting a
        primitive.  Contiguous device tensors: origins, dirs (n, 3) float32; outputs vis (n,) float32 =
        count / K (1 for a miss), count (n,) int32 or None, t (n,) float32, geom, prim (n,) int32 or None
        (intersect_rays' values).  samples, sets: K and S, None = the table's.  exact=True: every ray
        through the reference loop."""
        import torch
        n, po, pd, _ = self._query_inputs(origins, dirs, None)
        args = (self._query_ptr("vis", vis, torch.float32, (n,)),
                None if count is None else self._query_ptr("count", count, torch.int32, (n,)),
                None if t is None else self._query_ptr("t", t, torch.float32, (n,)),
                None if geom is None else self._query_ptr("geom", geom, torch.int32, (n,)),
                None if prim is None else self._query_ptr("prim", prim, torch.int32, (n,)))
        o = self._ambient_options(samples, sets, radius, bias, seed, pixel_base, exact)
        check(self._lib.esc_ambient_rays(self._h, n, po, pd, C.byref(o), *args))

    def ambient(self, origins, dirs, *, radius=FLT_MAX, bias=1e-4, samples=None, sets=None, seed=0, pixel_base=0,
                exact=False):
        """Synchronous ambient occlusion of numpy rays: {"vis", "count", "t", "geom", "prim"} as numpy arrays."""
        import torch
        to, td, _ = self._stage(origins, dirs, None)
        n = to.shape[0]
        dev = to.device
        vis = torch.empty(n, dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        geom = torch.empty(n, dtype=torch.int32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        self.ambient_rays(to, td, vis, radius=radius, bias=bias, count=count, t=t, geom=geom, prim=prim,
                          samples=samples, sets=sets, seed=seed, pixel_base=pixel_base, exact=exact)
        self.synchronize()
        return {"vis": vis.cpu().numpy(), "count": count.cpu().numpy(), "t": t.cpu().numpy(),
                "geom": geom.cpu().numpy(), "prim": prim.cpu().numpy()}

    def render_ambient(self, camera, W, H, *, radius=FLT_MAX, bias=1e-4, samples=None, sets=None, seed=0,
                       want_count=False, exact=False):
        """Pixel-centre visibility of a frame (esc_render_ambient): ambient_rays on camera_rays(camera, W, H)
        with pixel ids h * W + w, the rays made inside the kernel.  Returns numpy float32 (H, W), and the
        int32 (H, W) counts when asked for.  Synchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        vis = torch.empty((H, W), dtype=torch.float32, device=dev)
        count = torch.empty((H, W), dtype=torch.int32, device=dev) if want_count else None
        o = self._ambient_options(samples, sets, radius, bias, seed, 0, exact)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        check(self._lib.esc_render_ambient(self._h, C.byref(camera.c), W, H, C.byref(o), C.c_void_p(vis.data_ptr()),
                                           None if count is None else C.c_void_p(count.data_ptr())))
        self.synchronize()
        return (vis.cpu().numpy(), count.cpu().numpy()) if want_count else vis.cpu().numpy()

    def modulate(self, image, vis, *, want_u8=False):
        """image * vis per pixel and channel on the GPU (esc_modulate): image (..., 3) float32 and vis (...)
        float32 numpy arrays of the same pixels.  Returns the float32 product, and its quantised bytes when
        asked for.  Synchronous."""
        import torch
        img = np.ascontiguousarray(image, dtype=np.float32)
        v = np.ascontiguousarray(vis, dtype=np.float32)
        if img.shape[-1:] != (3,) or img.shape[:-1] != v.shape:
            raise ValueError("image must have shape vis.shape + (3,)")
        dev = torch.device("cuda", self.device)
        ti = torch.from_numpy(img).to(dev)
        tv = torch.from_numpy(v).to(dev)
        out = torch.empty_like(ti)
        u8 = torch.empty(img.shape, dtype=torch.uint8, device=dev) if want_u8 else None
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.esc_modulate(self._h, v.size, C.c_void_p(ti.data_ptr()), C.c_void_p(tv.data_ptr()),
                                     C.c_void_p(out.data_ptr()), None if u8 is None else C.c_void_p(u8.data_ptr())))
        self.synchronize()
        return (out.cpu().numpy(), u8.cpu().numpy()) if want_u8 else out.cpu().numpy()

    def ambient_stats(self):
        """Counts of the last ambient_rays / render_ambient / skylight_rays / render_skylight call: rays, hit_rays, samples (K * hit_rays),
        occluded_samples, exact_rays (primary or sample rays that took the reference loop), exact_tests.
        Synchronises."""
        s = _capi.esc_ambient_stats()
        check(self._lib.esc_last_ambient_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("rays", "hit_rays", "samples", "occluded_samples", "exact_rays",
                                                "exact_tests")}

    # ---- sky lighting (esc_skylight_rays / esc_render_skylight / esc_add_light) --------------------------
    def skylight_rays(self, origins, dirs, *, sky=None, light=None, vis=None, radius=FLT_MAX, bias=1e-4, count=None,
                      t=None, geom=None, prim=None, samples=None, sets=None, seed=0, pixel_base=0, exact=False):
        """Sky lighting of n rays (esc_skylight_rays), asynchronous on the renderer's stream: ambient_rays'
        samples, and what the open ones see of the environment cube.  sky (n, 3) float32 = the sum of env(w_k)
        over the open samples / K, light (n, 3) float32 = the hit material's kd * sky; both zero for a miss.
        Contiguous device tensors; sky or light may be None, not both; vis, count, t, geom, prim are
        ambient_rays' outputs, each optional here.  Needs a sample table and an environment."""
        import torch
        n, po, pd, _ = self._query_inputs(origins, dirs, None)
        opt = lambda name, x, dtype, shape: None if x is None else self._query_ptr(name, x, dtype, shape)  # noqa: E731
        args = (opt("sky", sky, torch.float32, (n, 3)), opt("light", light, torch.float32, (n, 3)),
                opt("vis", vis, torch.float32, (n,)), opt("count", count, torch.int32, (n,)),
                opt("t", t, torch.float32, (n,)), opt("geom", geom, torch.int32, (n,)),
                opt("prim", prim, torch.int32, (n,)))
        o = self._ambient_options(samples, sets, radius, bias, seed, pixel_base, exact)
        check(self._lib.esc_skylight_rays(self._h, n, po, pd, C.byref(o), *args))

    def skylight(self, origins, dirs, *, radius=FLT_MAX, bias=1e-4, samples=None, sets=None, seed=0, pixel_base=0,
                 exact=False):
        """Synchronous sky lighting of numpy rays: {"sky", "light", "vis", "count", "t", "geom", "prim"} as
        numpy arrays."""
        import torch
        to, td, _ = self._stage(origins, dirs, None)
        n = to.shape[0]
        dev = to.device
        out = {"sky": torch.empty((n, 3), dtype=torch.float32, device=dev),
               "light": torch.empty((n, 3), dtype=torch.float32, device=dev),
               "vis": torch.empty(n, dtype=torch.float32, device=dev),
               "count": torch.empty(n, dtype=torch.int32, device=dev),
               "t": torch.empty(n, dtype=torch.float32, device=dev),
               "geom": torch.empty(n, dtype=torch.int32, device=dev),
               "prim": torch.empty(n, dtype=torch.int32, device=dev)}
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        self.skylight_rays(to, td, radius=radius, bias=bias, samples=samples, sets=sets, seed=seed,
                           pixel_base=pixel_base, exact=exact, **out)
        self.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def render_skylight(self, camera, W, H, *, radius=FLT_MAX, bias=1e-4, samples=None, sets=None, seed=0,
                        want_light=True, want_count=False, exact=False):
        """Pixel-centre sky lighting of a frame (esc_render_skylight): skylight_rays on camera_rays(camera, W,
        H) with pixel ids h * W + w, the rays made inside the kernel.  Returns a dict of numpy arrays: "sky"
        (H, W, 3) and "vis" (H, W) float32, "light" (H, W, 3) when want_light, "count" (H, W) int32 when
        want_count.  Synchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        out = {"sky": torch.empty((H, W, 3), dtype=torch.float32, device=dev),
               "vis": torch.empty((H, W), dtype=torch.float32, device=dev)}
        if want_light:
            out["light"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        if want_count:
            out["count"] = torch.empty((H, W), dtype=torch.int32, device=dev)
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None  # noqa: E731
        o = self._ambient_options(samples, sets, radius, bias, seed, 0, exact)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        check(self._lib.esc_render_skylight(self._h, C.byref(camera.c), W, H, C.byref(o), ptr("sky"), ptr("light"),
                                            ptr("vis"), ptr("count")))
        self.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def add_light(self, image, light, *, want_u8=False):
        """image + light per pixel and channel on the GPU (esc_add_light): two float32 numpy arrays (..., 3)
        of the same shape.  Returns the float32 sum, and its quantised bytes when asked for.  Synchronous."""
        import torch
        img = np.ascontiguousarray(image, dtype=np.float32)
        lt = np.ascontiguousarray(light, dtype=np.float32)
        if img.shape[-1:] != (3,) or img.shape != lt.shape:
            raise ValueError("image and light must have the same shape (..., 3)")
        dev = torch.device("cuda", self.device)
        ti = torch.from_numpy(img).to(dev)
        tl = torch.from_numpy(lt).to(dev)
        out = torch.empty_like(ti)
        u8 = torch.empty(img.shape, dtype=torch.uint8, device=dev) if want_u8 else None
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.esc_add_light(self._h, img.size // 3, C.c_void_p(ti.data_ptr()), C.c_void_p(tl.data_ptr()),
                                      C.c_void_p(out.data_ptr()), None if u8 is None else C.c_void_p(u8.data_ptr())))
        self.synchronize()
        return (out.cpu().numpy(), u8.cpu().numpy()) if want_u8 else out.cpu().numpy()

    # ---- G-buffer and the edge-stopping filter (esc_gbuffer_rays / esc_render_gbuffer / esc_filter_guided) ----
    _GBUFFER = (("normal", "float32", 3), ("position", "float32", 3), ("albedo", "float32", 3),
                ("t", "float32", 0), ("geom", "int32", 0), ("prim", "int32", 0))

    def _gbuffer_tensors(self, shape):
        import torch
        dev = torch.device("cuda", self.device)
        return {k: torch.empty(tuple(shape) + ((c,) if c else ()), dtype=getattr(torch, dt), device=dev)
                for k, dt, c in self._GBUFFER}

    def gbuffer_rays(self, origins, dirs, *, normal=None, position=None, albedo=None, t=None, geom=None, prim=None,
                     exact=False):
        """The guides of n rays (esc_gbuffer_rays), asynchronous on the renderer's stream: normal (n, 3) = the
        shading normal of the closest hit, not flipped towards the ray, position (n, 3) = o + d*t, albedo
        (n, 3) = the hit material's kd, all float32 and zero for a miss, and t (n,) float32, geom, prim (n,)
        int32 = intersect_rays' values.  Contiguous device tensors; each output may be None, not all of them.
        exact=True: every ray through the reference loop."""
        import torch
        n, po, pd, _ = self._query_inputs(origins, dirs, None)
        given = {"normal": normal, "position": position, "albedo": albedo, "t": t, "geom": geom, "prim": prim}
        args = [None if given[k] is None else
                self._query_ptr(k, given[k], getattr(torch, dt), (n, c) if c else (n,)) for k, dt, c in self._GBUFFER]
        check(self._lib.esc_gbuffer_rays(self._h, n, po, pd, ESC_RENDER_EXACT_ONLY if exact else 0, *args))

    def gbuffer(self, origins, dirs, *, exact=False):
        """Synchronous G-buffer of numpy rays: {"normal", "position", "albedo", "t", "geom", "prim"} as numpy
        arrays."""
        import torch
        to, td, _ = self._stage(origins, dirs, None)
        out = self._gbuffer_tensors((to.shape[0],))
        torch.cuda.current_stream(to.device).synchronize()  # the buffers were made on torch's stream
        self.gbuffer_rays(to, td, exact=exact, **out)
        self.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def render_gbuffer(self, camera, W, H, *, exact=False):
        """The guides of a frame's pixel centres (esc_render_gbuffer): gbuffer_rays on camera_rays(camera, W, H),
        the rays made inside the kernel.  Returns a dict of DEVICE tensors: "normal", "position", "albedo"
        (H, W, 3) float32, "t" (H, W) float32, "geom", "prim" (H, W) int32 -- what filter_guided takes as
        guides.  The renderer's stream is synchronised before it returns."""
        import torch
        out = self._gbuffer_tensors((H, W))
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
        check(self._lib.esc_render_gbuffer(self._h, C.byref(camera.c), W, H, ESC_RENDER_EXACT_ONLY if exact else 0,
                                           *[C.c_void_p(out[k].data_ptr()) for k, _, _ in self._GBUFFER]))
        self.synchronize()
        return out

    def gbuffer_stats(self):
        """Counts of the last gbuffer_rays / gbuffer / render_gbuffer call: rays, hit_rays, exact_rays,
        exact_tests.  Synchronises."""
        s = _capi.esc_gbuffer_stats()
        check(self._lib.esc_last_gbuffer_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("rays", "hit_rays", "exact_rays", "exact_tests")}

    def filter_guided(self, image, guides, *, iterations=3, normal_cos=0.9, plane_dist, same_object=True, out=None):
        """The edge-stopping a-trous filter (esc_filter_guided): `iterations` passes of a 5 x 5 B3-spline
        kernel with steps 1, 2, 4, ... pixels over `image`, (H, W) or (H, W, 3) float32, a numpy array or a
        contiguous device tensor.  A tap counts only when it is a hit of the same object (same_object) whose
        normal has dot >= normal_cos with the pixel's and which lies within plane_dist of the pixel's tangent
        plane; pixels without a hit are copied.  guides: the dict render_gbuffer returns ("normal", "position",
        "geom", "prim" are read), device tensors or numpy arrays.  Returns a numpy array for a numpy image
        (synchronous); for a device tensor a device tensor (`out`, or a new one), asynchronous on the
        renderer's stream."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(image, torch.Tensor)
        img = torch.from_numpy(np.array(image, dtype=np.float32, order="C")).to(dev) if as_numpy else image
        if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
            raise ValueError("image must have shape (H, W) or (H, W, 3)")
        H, W = int(img.shape[0]), int(img.shape[1])
        ch = 3 if img.dim() == 3 else 1
        pi = self._query_ptr("image", img, torch.float32, tuple(img.shape))
        ptrs = []
        for k, dt, c in (("normal", torch.float32, 3), ("position", torch.float32, 3), ("geom", torch.int32, 0),
                         ("prim", torch.int32, 0)):
            g = guides[k]
            if not isinstance(g, torch.Tensor):
                g = torch.from_numpy(np.array(g, dtype=np.float32 if c else np.int32, order="C")).to(dev)
            g = g.reshape((H, W, 3) if c else (H, W))
            ptrs.append((self._query_ptr(k, g, dt, (H, W, 3) if c else (H, W)), g))
        if out is None:
            out = torch.empty_like(img)
        po = self._query_ptr("out", out, torch.float32, tuple(img.shape))
        o = _capi.esc_filter_options(int(iterations), float(normal_cos), float(plane_dist), int(bool(same_object)))
        torch.cuda.current_stream(dev).synchronize()  # copies and buffers were made on torch's stream
        check(self._lib.esc_filter_guided(self._h, W, H, ch, pi, *[p for p, _ in ptrs], C.byref(o), po))
        if as_numpy:
            self.synchronize()
            return out.cpu().numpy()
        self._filter_keep = (img, [g for _, g in ptrs])  # alive until the next call: the launch is asynchronous
        return out

    def filter_stats(self):
        """Counts of the last filter_guided call: pixels, hit_pixels, taps_tested and taps_accepted (both summed
        over the iterations).  Synchronises."""
        s = _capi.esc_filter_stats()
        check(self._lib.esc_last_filter_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("pixels", "hit_pixels", "taps_tested", "taps_accepted")}

    # ---- temporal accumulation (esc_temporal_accumulate) -------------------------------------------------
    def _guide_tensors(self, name, guides, H, W):
        """-> the four guide arrays as contiguous device tensors of a (H, W) frame, and an esc_guides of them"""
        import torch
        dev = torch.device("cuda", self.device)
        t = {}
        for k, dt, c in (("normal", torch.float32, 3), ("position", torch.float32, 3), ("geom", torch.int32, 0),
                         ("prim", torch.int32, 0)):
            g = guides[k]
            if not isinstance(g, torch.Tensor):
                g = torch.from_numpy(np.array(g, dtype=np.float32 if c else np.int32, order="C")).to(dev)
            g = g.reshape((H, W, 3) if c else (H, W))
            self._query_ptr(f"{name}[{k!r}]", g, dt, (H, W, 3) if c else (H, W))
            t[k] = g
        return t, _capi.esc_guides(*[t[k].data_ptr() for k in ("normal", "position", "geom", "prim")])

    def temporal_accumulate(self, image, guides, prev_camera, history, history_n, prev_guides, *, taps=4,
                            max_history=32, normal_cos=0.9, plane_dist, same_object=True, out=None, out_n=None):
        """Temporal accumulation (esc_temporal_accumulate): every hit pixel of `image`, (H, W) or (H, W, 3)
        float32 with the guides of its frame, is looked up in the previous frame -- rendered with prev_camera at
        the same size, whose accumulated image is `history`, whose history lengths are `history_n` (H, W) int32
        and whose guides are prev_guides -- through `taps` = 1 (nearest) or 4 (bilinear) history pixels, which
        count under the stops of filter_guided, and blended with alpha = 1 / n, n at most max_history.  A first
        frame is the call with history_n all zero.  guides, prev_guides: dicts as render_gbuffer returns them
        ("normal", "position", "geom", "prim" are read).  Arrays may be numpy arrays or contiguous device
        tensors.  Returns (out, out_n): numpy arrays for a numpy image (synchronous); for a device tensor
        device tensors (`out` / `out_n`, or new ones), asynchronous on the renderer's stream.  out may be
        image, but not history, and out_n not history_n."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(image, torch.Tensor)
        img = torch.from_numpy(np.array(image, dtype=np.float32, order="C")).to(dev) if as_numpy else image
        if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
            raise ValueError("image must have shape (H, W) or (H, W, 3)")
        H, W = int(img.shape[0]), int(img.shape[1])
        ch = 3 if img.dim() == 3 else 1
        pi = self._query_ptr("image", img, torch.float32, tuple(img.shape))
        hist = history
        if not isinstance(hist, torch.Tensor):
            hist = torch.from_numpy(np.array(hist, dtype=np.float32, order="C")).to(dev)
        hn = history_n
        if not isinstance(hn, torch.Tensor):
            hn = torch.from_numpy(np.array(hn, dtype=np.int32, order="C")).to(dev)
        ph = self._query_ptr("history", hist, torch.float32, tuple(img.shape))
        phn = self._query_ptr("history_n", hn, torch.int32, (H, W))
        tc, gc = self._guide_tensors("guides", guides, H, W)
        tp, gp = self._guide_tensors("prev_guides", prev_guides, H, W)
        if out is None:
            out = torch.empty_like(img)
        if out_n is None:
            out_n = torch.empty((H, W), dtype=torch.int32, device=dev)
        po = self._query_ptr("out", out, torch.float32, tuple(img.shape))
        pon = self._query_ptr("out_n", out_n, torch.int32, (H, W))
        o = _capi.esc_temporal_options(int(taps), int(max_history), float(normal_cos), float(plane_dist),
                                       int(bool(same_object)))
        torch.cuda.current_stream(dev).synchronize()  # copies and buffers were made on torch's stream
        check(self._lib.esc_temporal_accumulate(self._h, C.byref(prev_camera.c), W, H, ch, pi, C.byref(gc), ph, phn,
                                                C.byref(gp), C.byref(o), po, pon))
        if as_numpy:
            self.synchronize()
            return out.cpu().numpy(), out_n.cpu().numpy()
        self._temporal_keep = (img, hist, hn, tc, tp)  # alive until the next call: the launch is asynchronous
        return out, out_n

    def temporal_stats(self):
        """Counts of the last temporal_accumulate call: pixels, hit_pixels, reused_pixels, taps_tested and
        taps_accepted.  Synchronises."""
        s = _capi.esc_temporal_stats()
        check(self._lib.esc_last_temporal_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("pixels", "hit_pixels", "reused_pixels", "taps_tested",
                                                "taps_accepted")}

    # ---- environment cube map (esc_set_environment / esc_environment_rays) ------------------------------
    def set_environment(self, cube):
        """esc_set_environment: cube is a (6, R, R, 3) float32 array, faces +x, -x, +y, -y, +z, -z
        (environment_sky makes a gradient), 1 <= R <= 1024, or None to remove the environment.  While one is
        set, the rays of trace_rays / trace / render_traced that miss take its colour instead of black, at
        every level; nothing else changes.  It belongs to the renderer and survives uploads.  Synchronises."""
        if cube is None:
            check(self._lib.esc_set_environment(self._h, 0, None))
            return
        t = np.ascontiguousarray(cube, dtype=np.float32)
        if t.ndim != 4 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or t.shape[3] != 3:
            raise ValueError("cube must have shape (6, R, R, 3)")
        check(self._lib.esc_set_environment(self._h, t.shape[1], _fp(t)))

    @property
    def environment_res(self):
        """R of the renderer's environment cube, 0 when none is set"""
        r = C.c_int32(-1)
        check(self._lib.esc_get_environment_res(self._h, C.byref(r)))
        return int(r.value)

    def environment_rays(self, dirs, rgb, rgb8=None):
        """env(d) of n directions (esc_environment_rays), asynchronous on the renderer's stream.  Contiguous
        device tensors: dirs (n, 3) float32; outputs rgb (n, 3) float32 or None, rgb8 (n, 3) uint8 or None
        (not both None).  Needs an environment, no scene."""
        import torch
        if not hasattr(dirs, "shape") or len(dirs.shape) != 2:
            raise ValueError("dirs must have shape (n, 3)")
        n = int(dirs.shape[0])
        pd = self._query_ptr("dirs", dirs, torch.float32, (n, 3))
        check(self._lib.esc_environment_rays(
            self._h, n, pd, None if rgb is None else self._query_ptr("rgb", rgb, torch.float32, (n, 3)),
            None if rgb8 is None else self._query_ptr("rgb8", rgb8, torch.uint8, (n, 3))))

    def environment(self, dirs):
        """Synchronous lookup of numpy directions: {"rgb", "rgb8"} as numpy arrays."""
        import torch
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        dev = torch.device("cuda", self.device)
        td = torch.from_numpy(d).to(dev)
        rgb = torch.empty((d.shape[0], 3), dtype=torch.float32, device=dev)
        rgb8 = torch.empty((d.shape[0], 3), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the copy ran on torch's stream
        self.environment_rays(td, rgb, rgb8)
        self.synchronize()
        return {"rgb": rgb.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}

    def trace_rays(self, origins, dirs, rgb, *, max_depth, bias, rgb8=None, pixel_base=0, shadows=True,
                   face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, exact=False, transmission="off"):
        """Mirror reflections (esc_trace_rays): shade_rays' colour plus up to max_depth (0..16) specular
        bounces weighted by the materials' ks; bias >= 0 moves a bounce's origin off its surface.
        Asynchronous on the renderer's stream, one launch per depth level.  Contiguous device tensors
        as for shade_rays; max_depth=0 is shade_rays bit for bit.  transmission="refract" | "fresnel"
        (esc_trace_rays_ex): materials with a transmission entry refract; "off" is the plain call."""
        import torch
        mode = _transmit_mode(transmission)
        n, po, pd, _ = self._query_inputs(origins, dirs, None)
        args = (self._query_ptr("rgb", rgb, torch.float32, (n, 3)),
                None if rgb8 is None else self._query_ptr("rgb8", rgb8, torch.uint8, (n, 3)))
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        if mode == ESC_TRANSMIT_OFF:
            check(self._lib.esc_trace_rays(self._h, n, po, pd, int(pixel_base) & 0xffffffff, C.byref(o),
                                           int(max_depth), float(bias), *args))
        else:
            to = _capi.esc_trace_options(int(max_depth), float(bias), mode, 0)
            check(self._lib.esc_trace_rays_ex(self._h, n, po, pd, int(pixel_base) & 0xffffffff, C.byref(o),
                                              C.byref(to), *args))

    def trace(self, origins, dirs, *, max_depth, bias, pixel_base=0, shadows=True, face_mode=ESC_FACE_FIXED,
              fixed_face=0, seed=0, exact=False, transmission="off"):
        """Synchronous tracing of numpy rays: {"rgb", "rgb8"} as numpy arrays."""
        import torch
        to, td, _ = self._stage(origins, dirs, None)
        n = to.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float32, device=to.device)
        rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=to.device)
        self.trace_rays(to, td, rgb, max_depth=max_depth, bias=bias, rgb8=rgb8, pixel_base=pixel_base,
                        shadows=shadows, face_mode=face_mode, fixed_face=fixed_face, seed=seed, exact=exact,
                        transmission=transmission)
        self.synchronize()
        return {"rgb": rgb.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}

    def render_traced(self, camera, W, H, *, spp=1, max_depth, bias, want_u8=False, shadows=True,
                      face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, exact=False, transmission="off"):
        """Frame with mirror reflections (esc_render_traced): render_supersampled's samples, each
        traced through up to max_depth bounces.  Returns numpy fp32 (H, W, 3) and optionally the
        quantised bytes.  Synchronous.  transmission as for trace_rays (esc_render_traced_ex)."""
        import torch
        dev = torch.device("cuda", self.device)
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        mode = _transmit_mode(transmission)
        out = (C.c_void_p(img.data_ptr()), None if u8 is None else C.c_void_p(u8.data_ptr()))
        if mode == ESC_TRANSMIT_OFF:
            check(self._lib.esc_render_traced(self._h, C.byref(camera.c), W, H, int(spp), int(max_depth),
                                              float(bias), C.byref(o), *out))
        else:
            to = _capi.esc_trace_options(int(max_depth), float(bias), mode, 0)
            check(self._lib.esc_render_traced_ex(self._h, C.byref(camera.c), W, H, int(spp), C.byref(o),
                                                 C.byref(to), *out))
        self.synchronize()
        return (img.cpu().numpy(), u8.cpu().numpy()) if want_u8 else img.cpu().numpy()

    # ---- thin-lens camera (esc_set_lens_table / esc_lens_rays / esc_render_lens) -------------------------
    def set_lens_table(self, table):
        """esc_set_lens_table: table is a (sets, samples, 2) float32 array of points of the unit disk
        (lens_table makes one), 1 <= sets, samples <= 64, or None to remove the table.  It belongs to the
        renderer and survives uploads.  Its contents are not validated.  Synchronises."""
        if table is None:
            check(self._lib.esc_set_lens_table(self._h, 0, 0, None))
            return
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 3 or t.shape[2] != 2:
            raise ValueError("table must have shape (sets, samples, 2)")
        check(self._lib.esc_set_lens_table(self._h, t.shape[0], t.shape[1], _fp(t)))

    @property
    def lens_table_shape(self):
        """(sets, samples) of the renderer's lens table, (0, 0) when none is set"""
        s, k = C.c_int32(-1), C.c_int32(-1)
        check(self._lib.esc_get_lens_table_shape(self._h, C.byref(s), C.byref(k)))
        return int(s.value), int(k.value)

    def lens_rays(self, camera, W, H, *, aperture, focus_dist, sample=0, seed=0, rows=None, offsets=None):
        """The frame's primary rays through a thin lens (esc_lens_rays) as device tensors (origins, dirs),
        laid out as camera_rays' and with its rows and offsets: a ray starts at lens point `sample` of its
        pixel's set of the lens table, scaled by `aperture` (the lens radius), and aims at the point of the
        plane at `focus_dist` along the view axis that the pinhole ray meets.  seed picks the sets.
        aperture=0 gives camera_rays' bits and needs no table.  Asynchronous."""
        import torch
        r0, r1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(0, (r1 - r0) * W)
        dev = torch.device("cuda", self.device)
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        po = None if offsets is None else self._query_ptr("offsets", offsets, torch.float32, (n, 2))
        lo = _capi.esc_lens_options(float(aperture), float(focus_dist), int(seed) & (2 ** 64 - 1))
        check(self._lib.esc_lens_rays(self._h, C.byref(camera.c), W, H, r0, r1, po, C.byref(lo), int(sample),
                                      C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())))
        return o, d

    def render_lens(self, camera, W, H, *, spp, aperture, focus_dist, lens_seed=0, max_depth=0, bias=1e-4,
                    transmission="off", want_u8=False, shadows=True, face_mode=ESC_FACE_FIXED, fixed_face=0,
                    seed=0, exact=False):
        """Frame with depth of field (esc_render_lens): render_traced with sample k of every pixel sent
        through lens point k of the pixel's set (lens_rays), so spp <= the table's samples per set.  The
        plane at focus_dist stays sharp.  aperture=0 is render_traced, bit for bit.  Returns numpy fp32
        (H, W, 3) and optionally the quantised bytes.  Synchronous; trace_stats / transmit_stats report it."""
        import torch
        dev = torch.device("cuda", self.device)
        img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        o = _options(shadows, face_mode, fixed_face, seed, ESC_STAGE_AUTO, 0,
                     ESC_RENDER_EXACT_ONLY if exact else 0)
        to = _capi.esc_trace_options(int(max_depth), float(bias), _transmit_mode(transmission), 0)
        lo = _capi.esc_lens_options(float(aperture), float(focus_dist), int(lens_seed) & (2 ** 64 - 1))
        torch.cuda.current_stream(dev).synchronize()  # the buffers were made on torch's stream
        check(self._lib.esc_render_lens(self._h, C.byref(camera.c), W, H, int(spp), C.byref(o), C.byref(to),
                                        C.byref(lo), C.c_void_p(img.data_ptr()),
                                        None if u8 is None else C.c_void_p(u8.data_ptr())))
        self.synchronize()
        return (img.cpu().numpy(), u8.cpu().numpy()) if want_u8 else img.cpu().numpy()

    def trace_stats(self):
        """Counts of the last trace_rays / render_traced call: rays (primary and bounce), hit_rays,
        shadow_rays, exact_rays, exact_tests and depth_rays (17 values: the rays shaded at each
        level).  Synchronises."""
        s = _capi.esc_trace_stats()
        check(self._lib.esc_last_trace_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k in ("rays", "hit_rays", "shadow_rays", "exact_rays", "exact_tests")}
        out["depth_rays"] = [int(v) for v in s.depth_rays]
        return out

    def transmit_stats(self):
        """Counts of the last trace_rays / render_traced call with a transmission mode: the rays sent on
        as refracted, fresnel_reflected and total_internal (all zero after a plain call).  Synchronises."""
        s = _capi.esc_transmit_stats()
        check(self._lib.esc_last_transmit_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("refracted", "fresnel_reflected", "total_internal")}

    def tile_lists(self, which):
        """the lists of the last frame (0 / 1: tile lists of spheres / triangles; 2 / 3: light lists of
        sphere / triangle pair records) -> dict with the
        header numbers and the per-tile counts, or None when the frame used none"""
        hdr = (C.c_int32 * 8)()
        n = check(self._lib.esc_tile_list_counts(self._h, which, hdr, None, 0))
        if n == 0:
            return None
        cnt = np.zeros(n, np.int32)
        check(self._lib.esc_tile_list_counts(self._h, which, hdr, cnt.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return {"global": hdr[0], "cones": hdr[1], "off": hdr[2], "tiles_x": hdr[3], "tile_rows": hdr[4],
                "cap": hdr[5], "global_cap": hdr[6], "counts": cnt.reshape(hdr[4], hdr[3])}

    def tile_list_ids(self, which, index):
        """esc_tile_list_ids: the entries of ONE tile / cell of the last frame's lists (`index` in the order
        of tile_lists(which)["counts"], flattened) -> (int32 array of the stored entries, at most the list's
        capacity; the appended count)"""
        hdr = (C.c_int32 * 8)()
        if check(self._lib.esc_tile_list_counts(self._h, which, hdr, None, 0)) == 0:
            return np.zeros(0, np.int32), 0
        cap = hdr[6] if index < 0 else hdr[5]  # global capacity / list capacity
        ids = np.zeros(cap, np.int32)
        n = check(self._lib.esc_tile_list_ids(self._h, which, int(index),
                                              ids.ctypes.data_as(C.POINTER(C.c_int32)), cap))
        return ids[:min(n, cap)].copy(), n

    def tile_list_global(self, which):
        """the global list of the tile lists (which = 0 spheres, 1 triangles): the slots every tile tests
        -> (int32 array of the stored entries, at most the global capacity; the appended count)"""
        return self.tile_list_ids(which, -1)

    def tile_tri_masks(self):
        """esc_tile_tri_masks: the per-tile triangle masks of the last frame (a directly swept table of 1
        to 32 triangles) -> dict "off" (the masks switched themselves off), "global" (the word every tile
        ORs in), "tiles_x", "tile_rows", "n_tri", "masks" (tile_rows, tiles_x) uint32 -- or None when the
        frame had none"""
        info = (C.c_int32 * 8)()
        n = check(self._lib.esc_tile_tri_masks(self._h, info, None, 0))
        if n == 0:
            return None
        m = np.zeros(n, np.uint32)
        check(self._lib.esc_tile_tri_masks(self._h, info, m.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return {"off": info[0], "global": int(info[1]) & 0xFFFFFFFF, "tiles_x": info[2], "tile_rows": info[3],
                "n_tri": info[4], "masks": m.reshape(info[3], info[2])}

    def light_lists(self, which):
        """esc_light_list_read: the light lists of the last frame (which = 2 sphere pair records, 3 triangle
        pair records) as numpy arrays, or None when the frame used none -> dict: "n_listed", "R", "cap",
        "global_cap", "point" (n_listed,) rows of the light_points table, "face_counts" (n_listed, 6),
        "face_ids" (n_listed, 6, global_cap), "counts" (n_listed, 6, R, R) indexed [light, face, cw, cu] and
        "ids" (n_listed, 6, R, R, cap); an id array holds a list's stored ids first, then -1"""
        info = (C.c_int32 * 8)()
        i32 = C.POINTER(C.c_int32)
        n = check(self._lib.esc_light_list_read(self._h, which, info, None, None, 0, 0, None))
        if n == 0:
            return None
        n_listed, R, cap, gcap = info[0], info[1], info[2], info[3]
        per_light = 6 * R * R
        face_counts = np.zeros((n_listed, 6), np.int32)
        face_ids = np.zeros((n_listed, 6, gcap), np.int32)
        ids = np.zeros((n_listed, 6, R, R, cap), np.int32)
        for li in range(n_listed):  # one copy per light
            check(self._lib.esc_light_list_read(self._h, which, info, face_counts.ctypes.data_as(i32),
                                                face_ids.ctypes.data_as(i32), li * per_light, per_light,
                                                ids[li].ctypes.data_as(i32)))
        counts = np.zeros(n, np.int32)
        hdr = (C.c_int32 * 8)()
        check(self._lib.esc_tile_list_counts(self._h, which, hdr, counts.ctypes.data_as(i32), n))
        return {"n_listed": n_listed, "R": R, "cap": cap, "global_cap": gcap,
                "point": np.array(list(info[4:4 + n_listed]), np.int32), "face_counts": face_counts,
                "face_ids": face_ids, "counts": counts.reshape(n_listed, 6, R, R), "ids": ids}

    def light_lists_packed(self):
        """esc_light_list_packed_read: the packed form of the sphere light lists of the last frame, the
        form the shadow sweep reads, or None when there is none -> dict: "n_listed", "R", "per_step" (4),
        "total_steps", "steps" (n_listed, 6, R, R) indexed [light, face, cw, cu], -1 for a cell over its
        list capacity, and "slots" (n_listed, 6, R, R, 2 * list capacity): a cell's 4 * steps slots in the
        order they are tested, each a position 2 j + h in the group-sorted table or -1 (pad), then -1"""
        info = (C.c_int32 * 8)()
        i32 = C.POINTER(C.c_int32)
        n = check(self._lib.esc_light_list_packed_read(self._h, info, 0, 0, None, None))
        if n == 0:
            return None
        n_listed, R, per_cell = info[0], info[1], info[2]
        per_light = 6 * R * R
        steps = np.zeros((n_listed, 6, R, R), np.int32)
        slots = np.zeros((n_listed, 6, R, R, per_cell), np.int32)
        for li in range(n_listed):  # one copy per light
            check(self._lib.esc_light_list_packed_read(self._h, info, li * per_light, per_light,
                                                       steps[li].ctypes.data_as(i32),
                                                       slots[li].ctypes.data_as(i32)))
        return {"n_listed": n_listed, "R": R, "per_step": info[3], "total_steps": info[4],
                "steps": steps, "slots": slots}


class RecordedFrame:
    """esc_frame: one frame's launches as a HIP graph on its renderer's stream"""

    def __init__(self, lib, handle, keep):
        # the renderer (its context, under the graph) and the output buffers must outlive the graph
        self._lib, self._h, self._keep = lib, handle, keep
        self._launch = lib.esc_frame_launch

    def valid(self):
        """esc_frame_valid: True while launch() would be accepted (False once the renderer is closed)"""
        return bool(self._h and self._keep[0]._h and self._lib.esc_frame_valid(self._h))

    def launch(self):
        rc = self._launch(self._h)
        if rc:
            check(rc)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.esc_frame_destroy(h)

    def __del__(self):
        self.close()


class TemporalAccumulator:
    """Frame-to-frame state of Renderer.temporal_accumulate: the previous frame's camera, guides, accumulated
    image and history lengths, kept as device tensors.  The accumulated image and the lengths alternate
    between two buffers each, so no push reads what it writes.  options: temporal_accumulate's keywords
    (taps, max_history, normal_cos, plane_dist, same_object); plane_dist is required."""

    def __init__(self, renderer, **options):
        unknown = set(options) - {"taps", "max_history", "normal_cos", "plane_dist", "same_object"}
        if unknown:
            raise TypeError(f"unknown options: {sorted(unknown)}")
        if "plane_dist" not in options:
            raise TypeError("plane_dist is required")
        self._r, self._opts = renderer, dict(options)
        self.reset()

    def reset(self):
        """forget the history: the next push starts from zero"""
        self._camera = self._guides = None
        self._acc, self._n, self._at = [None, None], [None, None], 0

    @property
    def history_n(self):
        """the history lengths after the last push, a (H, W) int32 device tensor, or None before the first"""
        return self._n[self._at]

    def push(self, camera, image, guides):
        """Accumulate one frame: image (H, W) or (H, W, 3) float32 and its guides (render_gbuffer's dict), both
        numpy arrays or device tensors, rendered with `camera`.  The first push, or an image of another shape,
        starts from zero history.  Returns the accumulated image: a numpy array for a numpy image
        (synchronous), else the accumulator's own device tensor (asynchronous on the renderer's stream), which
        the push after the next one overwrites.  Guide tensors are kept until the next push, not copied."""
        import torch
        r = self._r
        dev = torch.device("cuda", r.device)
        as_numpy = not isinstance(image, torch.Tensor)
        img = torch.from_numpy(np.array(image, dtype=np.float32, order="C")).to(dev) if as_numpy else image
        if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
            raise ValueError("image must have shape (H, W) or (H, W, 3)")
        H, W = int(img.shape[0]), int(img.shape[1])
        cur, _ = r._guide_tensors("guides", guides, H, W)
        acc = self._acc[self._at]
        if acc is None or acc.shape != img.shape:
            self.reset()
            self._acc = [torch.zeros_like(img), torch.empty_like(img)]
            self._n = [torch.zeros((H, W), dtype=torch.int32, device=dev),
                       torch.empty((H, W), dtype=torch.int32, device=dev)]
            self._camera, self._guides = camera, cur
        to = 1 - self._at
        r.temporal_accumulate(img, cur, self._camera, self._acc[self._at], self._n[self._at], self._guides,
                              out=self._acc[to], out_n=self._n[to], **self._opts)
        self._at, self._camera, self._guides = to, camera, cur
        if as_numpy:
            r.synchronize()
            return self._acc[to].cpu().numpy()
        return self._acc[to]


def live_device_allocations():
    """esc_live_device_allocations: (buffers, bytes) the renderers of this process hold on their devices"""
    n, b = C.c_int64(), C.c_int64()
    check(_capi.load().esc_live_device_allocations(C.byref(n), C.byref(b)))
    return n.value, b.value


def strip_local_rows(H, strip_rows, first_strip, strip_stride):
    return check(_capi.load().esc_strip_local_rows(H, strip_rows, first_strip, strip_stride))


def render_multi(scene, camera, W, H, n_devices, *, want_u8=False, shadows=True,
                 face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, stage=ESC_STAGE_AUTO):
    """Single-process row-band split over n_devices (bands share devices when there are
    fewer GPUs than bands)."""
    lib = _capi.load()
    img = np.zeros((H, W, 3), np.float32)
    u8 = np.zeros((H, W, 3), np.uint8) if want_u8 else None
    ms = np.zeros(n_devices, np.float32)
    o = _options(shadows, face_mode, fixed_face, seed, stage)
    check(lib.esc_render_frame_multi(scene._h, C.byref(camera.c), W, H, C.byref(o), n_devices,
                                     _fp(img),
                                     u8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_u8 else None,
                                     _fp(ms)))
    return img, u8, ms


def rccl_available():
    """True when librccl.so could be bound at run time (esc_rccl_available)."""
    return bool(_capi.load().esc_rccl_available())


class MultiRenderer:
    """esc_multi: one process, n devices, 8-row strips dealt round-robin, the framebuffer gathered
    to the first device over RCCL (use_rccl=True) or by peer copies, then assembled there."""

    def __init__(self, n_devices, device_ids=None, use_rccl=True):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        ids = None
        if device_ids is not None:
            ids = (C.c_int32 * n_devices)(*[int(d) for d in device_ids])
        check(self._lib.esc_multi_create(int(n_devices), ids, 1 if use_rccl else 0,
                                         C.byref(self._h)))
        self.n_devices = int(n_devices)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.esc_multi_destroy(h)

    def __del__(self):
        self.close()

    def upload(self, scene):
        check(self._lib.esc_multi_upload_scene(self._h, scene._h))

    def render(self, camera, W, H, *, gather_u8=False, shadows=True, face_mode=ESC_FACE_FIXED,
               fixed_face=0, seed=0, stage=ESC_STAGE_AUTO, flags=0):
        """-> ((H, W, 3) fp32 or uint8 frame, per-device render ms, device address of the frame)"""
        o = _options(shadows, face_mode, fixed_face, seed, stage, 0, flags)
        ms = np.zeros(self.n_devices, np.float32)
        dptr = C.c_void_p()
        if gather_u8:
            out = np.zeros((H, W, 3), np.uint8)
            check(self._lib.esc_multi_render(self._h, C.byref(camera.c), W, H, C.byref(o), 1, None,
                                             out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             C.byref(dptr), _fp(ms)))
        else:
            out = np.zeros((H, W, 3), np.float32)
            check(self._lib.esc_multi_render(self._h, C.byref(camera.c), W, H, C.byref(o), 0,
                                             _fp(out), None, C.byref(dptr), _fp(ms)))
        return out, ms, dptr.value


def render_multi_rccl(scene, camera, W, H, n_devices, *, want_u8=False, shadows=True,
                      face_mode=ESC_FACE_FIXED, fixed_face=0, seed=0, stage=ESC_STAGE_AUTO):
    """esc_render_frame_multi_rccl: the one-call form (communicator set up and torn down inside)."""
    lib = _capi.load()
    img = np.zeros((H, W, 3), np.float32)
    u8 = np.zeros((H, W, 3), np.uint8) if want_u8 else None
    ms = np.zeros(n_devices, np.float32)
    o = _options(shadows, face_mode, fixed_face, seed, stage)
    check(lib.esc_render_frame_multi_rccl(
        scene._h, C.byref(camera.c), W, H, C.byref(o), n_devices, _fp(img),
        u8.ctypes.data_as(C.POINTER(C.c_uint8)) if want_u8 else None, _fp(ms)))
    return img, u8, ms


def trace(W, H, lookfrom, lookat, vup, vfov, aspect, flat, debug=0, test=0):
    """The ISPC drop-in symbol itself (trace.ispc:86-92 / main.cpp:619-624)."""
    lib = _capi.load()
    cam = _capi.ispc_cam()
    lib.esc_new_ispc_cam(C.byref(cam), _fp(_f32(lookfrom, (3,))), _fp(_f32(lookat, (3,))),
                         _fp(_f32(vup, (3,))), float(vfov), float(aspect))
    img = np.zeros((H, W, 3), np.float32)
    lib.trace(W, H, C.byref(cam), flat.num_triangles, flat.triangles, flat.num_lights,
              flat.lights, flat.num_light_triangles, flat.light_triangles, _fp(img), debug, test)
    return img


def quantise(image):
    img = _f32(image)
    out = np.zeros(img.shape, np.uint8)
    _capi.load().esc_quantise(_fp(img), img.size, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def write_ppm(path, image):
    """main.cpp:658-689 P3 writer; image (H, W, 3) fp32 or uint8, h = 0 bottom row."""
    lib = _capi.load()
    H, W = image.shape[0], image.shape[1]
    if image.dtype == np.uint8:
        a = np.ascontiguousarray(image)
        check(lib.esc_write_ppm_u8(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), W, H))
    else:
        a = _f32(image)
        check(lib.esc_write_ppm(str(path).encode(), _fp(a), W, H))
