"""GPU: ONE context walked through scenes, cameras, sizes, bands and options, every frame bit for bit the oracle's.

The frame path of csrc/rt_capi.cpp keeps tables with keys of their own (prepared_origin, ray_key, list_key and the
lists' flags, the light lists' face mode / fixed face / n_listed / allocation / packed steps, sure_origin, the
tree's origin bounds and bins, the grow-only d_hits / d_sq, and the epoch that ends recorded frames).  A frame is
right only if each is rebuilt when one of its inputs changes, which no test that starts from a fresh context can
see.  tests/context_walk_cases.py holds the walks (a directed one whose comments name the key each step aims at, and
tours of every ordered pair of scenes and of every option axis' values); tests/test_context_walk_cpu.py shows
that they cover what they claim and that consecutive references differ.

Each test keeps one Renderer for its whole walk.  After every frame step: the fp32 output as uint32 and the bytes
equal the oracle's band and its quantisation; the output buffers are fresh, poisoned, and keep their poison
outside the band; frame_tripwire() is 0; after esc_reset_counters, primary_rays, hit_pixels and shadow_rays equal
the oracle's of the band (anyhit_tests too under ESC_RENDER_INDEX_ORDER, where the sweep is the reference's --
unless the stage asked for is ESC_STAGE_BVH, whose tree and bins test other pairs in any order).  Up to
two recorded frames stay alive: after every step a valid one is replayed into its poisoned buffer and compared, an
invalid one must refuse its launch once and leave the poison, and a step identical to the recorded call must
leave a valid recording valid.  ("rays", ...) steps compare queries and shading with tests/ray_oracle.py and
trace / gbuffer / ambient with a fresh context, and may change neither a recording's validity, nor the render
counters, nor last_frame_kernel().  ("adaptive", ...) steps refine nothing (threshold FLT_MAX: the call refuses
inf) and give the oracle's frame.  At the end the library's device allocations are back where they were.

A failure -- a mismatch, or an error of a library call -- names the step and prints the walk up to it;
replay(steps) runs any such list, so a prefix can be shortened by hand.  No tolerance anywhere: every comparison is on bits.
"""
import time

import numpy as np
import pytest

import context_walk_cases as cw
import ray_oracle as ro

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON8 = 0xA5
POISON32 = 0xA5A5A5A5
FLT_MAX = float(np.finfo(np.float32).max)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Buffers:
    """fresh poisoned device buffers for n floats and n bytes with a guard of `guard` elements on either side"""

    def __init__(self, n, guard):
        import torch
        self.n, self.guard = n, guard
        self.f = torch.empty(n + 2 * guard, dtype=torch.int32, device="cuda:0")
        self.b = torch.empty(n + 2 * guard, dtype=torch.uint8, device="cuda:0")
        self.poison()

    def poison(self):
        import torch
        self.f.fill_(POISON32 - (1 << 32))
        self.b.fill_(POISON8)
        torch.cuda.current_stream().synchronize()  # filled on torch's stream; the renderer's is its own

    def out(self):
        import torch
        g, n = self.guard, self.n
        return self.f.view(torch.float32)[g:g + n], self.b[g:g + n]

    def read(self):
        """-> (uint32 band, byte band); the guards must still hold the poison"""
        g, n = self.guard, self.n
        f = self.f.cpu().numpy().view(np.uint32)
        b = self.b.cpu().numpy()
        for what, a, p in (("fp32", f, POISON32), ("byte", b, POISON8)):
            assert np.all(a[:g] == p) and np.all(a[g + n:] == p), f"the {what} output was written outside its band"
        return f[g:g + n], b[g:g + n]

    def untouched(self):
        f, b = self.read()
        return bool(np.all(f == POISON32) and np.all(b == POISON8))


def options(o):
    return dict(shadows=bool(o.shadows), face_mode=o.face_mode, fixed_face=o.fixed_face, seed=o.seed, stage=o.stage,
                px=o.px, flags=o.flags)


def compare(got_f, got_b, ref, ref8, what):
    ref_bits = bits(ref).reshape(-1)
    bad = np.flatnonzero(got_f.reshape(-1) != ref_bits)
    assert bad.size == 0, f"{what}: image mismatch, {bad.size} of {ref_bits.size} fp32 values differ from the " \
                          f"oracle's, first at {bad[:4].tolist()}"
    assert np.array_equal(got_b.reshape(-1), ref8.reshape(-1)), f"{what}: image mismatch in the bytes"


_RAYS = {}   # (scene, camera) -> the rays and their CPU references
_FRESH = {}  # (scene, kind, camera) -> the call's result on a fresh context


def rays_of(scene, cam):
    if (scene, cam) not in _RAYS:
        d = cw.pool()[scene]["dict"]
        o, targets = cw.ray_set(scene, cam)
        dirs, rgb = ro.ray_colours(d, o, targets)
        hit, occ = ro.ref_queries(d, o, dirs)
        _RAYS[(scene, cam)] = {"o": o, "dirs": dirs, "rgb": rgb, "hit": hit, "occ": occ}
    return _RAYS[(scene, cam)]


AMBIENT_TABLE = (4, 8, 1)  # sets, samples, seed of the table every context of this module gets


def new_renderer(esc):
    r = esc.Renderer(0)
    r.set_ambient_table(esc.ambient_table(*AMBIENT_TABLE))
    return r


def call(r, kind, o, dirs):
    if kind == "trace":
        return r.trace(o, dirs, max_depth=2, bias=1e-4)
    return r.gbuffer(o, dirs) if kind == "gbuffer" else r.ambient(o, dirs)


def fresh(esc, scene, kind, cam):
    if (scene, kind, cam) not in _FRESH:
        q = rays_of(scene, cam)
        r = new_renderer(esc)
        try:
            r.upload(cw.product(scene))
            _FRESH[(scene, kind, cam)] = call(r, kind, q["o"], q["dirs"])
        finally:
            r.close()
    return _FRESH[(scene, kind, cam)]


def rays_step(esc, r, scene, kind, cam):
    q = rays_of(scene, cam)
    if kind == "intersect":
        got = r.intersect(q["o"], q["dirs"])
        for k in ("t", "uv"):
            ro.assert_same(got[k], q["hit"][k], f"intersect: {k}")
        for k in ("geom", "prim"):
            assert np.array_equal(got[k], q["hit"][k]), f"intersect: {k} differs"
    elif kind == "occluded":
        assert np.array_equal(r.occluded(q["o"], q["dirs"]), q["occ"]), "occluded differs"
    elif kind == "shade":
        ro.assert_same(r.shade(q["o"], q["dirs"])["rgb"], q["rgb"], "shade: rgb")
    else:
        want = fresh(esc, scene, kind, cam)
        got = call(r, kind, q["o"], q["dirs"])
        assert set(got) == set(want)
        for k in want:
            if want[k].dtype == np.float32:
                ro.assert_same(got[k], want[k], f"{kind}: {k} against a fresh context")
            else:
                assert np.array_equal(got[k], want[k]), f"{kind}: {k} differs from a fresh context's"


class Recording:
    def __init__(self, frame, bufs, ref, call):
        self.frame, self.bufs, self.ref, self.call = frame, bufs, ref, call
        self.refused = False

    def check(self, r, esc):
        """a valid recording replays its frame; an invalid one refuses once, and is never launched again"""
        if self.frame.valid():
            assert not self.refused, "a recording that had refused its launch is valid again"
            self.bufs.poison()
            self.frame.launch()
            r.synchronize()
            compare(*self.bufs.read(), self.ref[0], self.ref[1], f"replay of the frame recorded as {self.call}")
        elif not self.refused:
            self.refused = True
            self.bufs.poison()
            with pytest.raises(esc.EscError):
                self.frame.launch()
            r.synchronize()
            assert self.bufs.untouched(), f"the refused launch of {self.call} wrote its buffer"


def frame_step(esc, r, scene, step):
    """renders a ("frame" | "record", camera, size, band, Opt) step into fresh poisoned buffers and checks it;
    -> the RecordedFrame's Recording for a record step"""
    kind, cam, size, band, o = step
    W, H = size
    ref, ref8, cnt = cw.reference(step, scene)
    camera = cw.camera(scene, cam, size)
    n = ref.size
    assert n > 0
    r.reset_counters()
    rec = None
    if band[0] == "host":
        out = np.full((H, W, 3), POISON32, np.uint32).view(F32)
        img, u8 = r.render(camera, W, H, want_u8=True, out=out, **options(o))
        got = bits(img).reshape(-1), u8.reshape(-1)
    else:
        bufs = Buffers(n, 3 * W * H)  # a whole frame on either side: a band written at its image rows would show
        of, ob = bufs.out()
        if kind == "record":
            assert band[0] == "strips"
            f = r.record_strips(camera, W, H, band[2], band[3], out_f32=of, out_u8=ob, strip_rows=band[1], **options(o))
            rec = Recording(f, bufs, (ref, ref8), step)
        elif band[0] == "rows":
            r.render_rows(camera, W, H, min(band[1], H), min(band[2], H), out_f32=of, out_u8=ob, **options(o))
        else:
            rows = r.render_strips(camera, W, H, band[2], band[3], out_f32=of, out_u8=ob, strip_rows=band[1],
                                   **options(o))
            assert rows * W * 3 == n
        r.synchronize()
        got = bufs.read()
    try:
        compare(*got, ref, ref8, "frame")
        assert r.frame_tripwire() == 0, "the tripwire of a frame without fallback is set"
        if not o.flags & esc.ESC_RENDER_NO_COUNTERS:
            c = r.counters()
            for k in ("primary_rays", "hit_pixels", "shadow_rays"):
                assert c[k] == cnt[k], f"counter {k}: {c[k]}, the oracle's {cnt[k]}"
            if o.flags & esc.ESC_RENDER_INDEX_ORDER and o.stage != esc.ESC_STAGE_BVH:
                assert c["anyhit_tests"] == cnt["anyhit_tests"], \
                    f"counter anyhit_tests in index order: {c['anyhit_tests']}, the oracle's {cnt['anyhit_tests']}"
    except BaseException:
        if rec is not None:
            rec.frame.close()
        raise
    return rec


def adaptive_step(esc, r, scene, step):
    _, cam, size, o = step
    ref, ref8, _ = cw.reference(step, scene)
    img, u8 = r.render_adaptive(cw.camera(scene, cam, size), size[0], size[1], 4, FLT_MAX, want_u8=True,
                                shadows=bool(o.shadows), face_mode=o.face_mode, fixed_face=o.fixed_face, seed=o.seed)
    compare(bits(img).reshape(-1), u8.reshape(-1), ref, ref8, "adaptive frame that refines nothing")
    assert r.adaptive_stats()["refined_pixels"] == 0
    assert r.frame_tripwire() == 0


def replay(steps, collect=False):
    """runs a walk on one fresh context.  A failing step raises AssertionError with its index and the walk up to
    it -- or, with collect=True, is noted and the walk goes on: -> [(index, step, message)]"""
    import esctp1raytracer_amd as esc
    failures = []
    before = esc.live_device_allocations()
    r = new_renderer(esc)
    recordings = []
    scene = None
    try:
        for i, step in enumerate(steps):
            try:
                valid = [rec.frame.valid() for rec in recordings]
                if step[0] == "upload":
                    scene = step[1]
                    r.upload(cw.product(scene))
                elif step[0] in ("frame", "record"):
                    if step[0] == "record" and len(recordings) == 2:
                        recordings.pop(0).frame.close()
                        valid.pop(0)
                    new = frame_step(esc, r, scene, step)
                    for rec, was in zip(recordings, valid):
                        if was and rec.call[1:] == step[1:] and step[3][0] == "strips":
                            assert rec.frame.valid(), f"the recording of {rec.call} ended at the same call again"
                    if new is not None:
                        recordings.append(new)
                elif step[0] == "adaptive":
                    adaptive_step(esc, r, scene, step)
                else:
                    counters, kernel = r.counters(), r.last_frame_kernel()
                    rays_step(esc, r, scene, step[1], step[2])
                    assert [rec.frame.valid() for rec in recordings] == valid, "a ray call ended a recording"
                    assert r.counters() == counters, "a ray call changed the render counters"
                    assert r.last_frame_kernel() == kernel, "a ray call changed last_frame_kernel()"
                for rec in recordings:
                    rec.check(r, esc)
            except AssertionError as e:
                if not collect:
                    raise AssertionError(f"step {i} {step!r}: {e}\nthe walk up to it:\n{steps[:i + 1]!r}") from None
                failures.append((i, step, str(e).splitlines()[0]))
            except esc.EscError as e:  # a refused call, or a HIP error: the walk ends here, collecting or not
                raise RuntimeError(f"step {i} {step!r}: {e}\nthe walk up to it:\n{steps[:i + 1]!r}") from e
    finally:
        for rec in recordings:
            rec.frame.close()
        r.close()
    assert esc.live_device_allocations() == before, "device allocations of the closed context are still live"
    return failures


@pytest.fixture(scope="module")
def walks():
    return cw.walks()


@pytest.mark.parametrize("name", cw.WALK_NAMES)
def test_walk(walks, name):
    t0 = time.perf_counter()
    replay(walks[name])
    print(f"walk {name!r}: {len(walks[name])} steps in {time.perf_counter() - t0:.2f} s")
