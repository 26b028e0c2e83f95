// rt_trace.hip -- Whitted-style mirror reflection and refraction on top of scan_row's body: one launch
// per depth level, one ray per lane, no host synchronisation between the levels (DESIGN.md §3.13 and
// §3.14; the definitions are in include/esctp1_rt.h at esc_trace_rays and esc_trace_options).
//
//   level k   reads its rays (k == 0: the caller's arrays, weight 1, destination = the ray's index;
//             k >= 1: queue k & 1, whose live count is read from device memory, lanes past it
//             leave), shades each with k_shade_rays' body (rt_shade_body.inc), updates the
//             destination's colour C, and appends the rays that bounce to the other queue.
//   append    wave ballot of the survivors, lane prefix by mbcnt, ONE ordinary global atomic add per
//             wave on the queue's counter, then plain vector stores into the SoA planes.
//   C         every destination has at most one ray in flight per level and the levels are
//             stream-ordered, so C = fl(C + fl(w * c)) is a plain load / multiply / add / store: no
//             float atomics, and the result does not depend on the order of the queue.
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt).
// A bounce ray is an ordinary ray to the sweeps: it passes the precondition gate or runs the
// index-order loop.  The kernel reads only per-scene tables.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_shade_body.h"
#include "rt_trace.h"
#include "rt_transmit.h"

namespace esc {

// FIRST: level 0 (the caller's arrays).  LAST: level max_depth, which never bounces: without the bounce
// nothing of the ray outlives the light loop, and the kernel is k_shade_rays plus the update of C.
// TRANSMIT: the scene has a transmissive material and the call asked for refraction (rt_transmit.h);
// every other call runs the <*, *, false> instantiations, which are the mirror-only kernels unchanged.
// ENV: the context holds an environment cube (rt_environ.h): a ray that misses takes the colour env(d)
// instead of black.  Without one the <*, *, *, false> instantiations run, the kernels as they were.
template <bool FIRST, bool LAST, bool TRANSMIT, bool ENV>
__global__ __launch_bounds__(256) void k_trace(const TraceParams T) {
  const ShadeParams &P = T.s;
  const QueryParams &p = P.q;
  const int64_t cap = p.n;
  int64_t n = cap;
  if (!FIRST) {
    n = (int64_t)*T.n_in;
    if (n > cap) n = cap; // one ray per destination bounds the count; this keeps every index in bounds
    if ((int64_t)blockIdx.x * 256 >= n) return;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool valid = i < n;
  f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f), w = mk(1.f, 1.f, 1.f);
  uint32_t dest = 0;
  if (valid) {
    if (FIRST) {
      o = mk(p.orig[3 * i], p.orig[3 * i + 1], p.orig[3 * i + 2]);
      d = mk(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
      dest = (uint32_t)i;
    } else {
      const float *q = T.q_in + i;
      o = mk(q[0], q[cap], q[2 * cap]);
      d = mk(q[3 * cap], q[4 * cap], q[5 * cap]);
      w = mk(q[6 * cap], q[7 * cap], q[8 * cap]);
      dest = __float_as_uint(q[9 * cap]);
      valid = dest < (uint64_t)cap; // always true; a record that is not is left alone, not written
    }
  }

#define SHADE_BODY_SEED P.seed
#define SHADE_BODY_PIXEL (P.pixel_base + dest)
#include "rt_shade_body.inc"
#undef SHADE_BODY_PIXEL
#undef SHADE_BODY_SEED

  if constexpr (ENV) { // lanes that hit are masked off, and a wave without a miss skips the loads
    if (valid && !has_hit) env_lookup(T.env.texels, T.env.res, d.x, d.y, d.z, r, g, b);
  }

  if (valid) {
    float *C = P.rgb + 3 * (int64_t)dest;
    if (!FIRST) {
      r = C[0] + w.x * r;
      g = C[1] + w.y * g;
      b = C[2] + w.z * b;
    }
    C[0] = r;
    C[1] = g;
    C[2] = b;
    if (P.rgb8) {
      uint8_t *C8 = P.rgb8 + 3 * (int64_t)dest;
      C8[0] = quantise_channel(r);
      C8[1] = quantise_channel(g);
      C8[2] = quantise_channel(b);
    }
  }

  // ---- the bounce
  uint32_t what = kBounceMirror; // TRANSMIT: what a transmissive hit did (rt_transmit.h)
  if (!LAST) {
    bool go = has_hit;
    f3 o2 = mk(0.f, 0.f, 0.f), d2 = mk(0.f, 0.f, 0.f);
    bool glass = false;
    if constexpr (TRANSMIT) {
      if (go) {
        const float *tr = T.transmit + kTransmitFloats * (int64_t)mi;
        const f3 tf = mk(tr[0], tr[1], tr[2]);
        const float ni = tr[3];
        glass = transmissive(tf.x, tf.y, tf.z, ni);
        if (glass)
          what = transmit_bounce(T.transmit_mode, P.seed, P.pixel_base + dest, tf, ni, T.bias, o, d, s.t, N, w,
                                 o2, d2, go);
        if (!go) what = kBounceMirror; // a refracted ray without weight is not counted
      }
    }
    if (go && !glass) {
      w = mk(w.x * P.mat[mi].ks[0], w.y * P.mat[mi].ks[1], w.z * P.mat[mi].ks[2]);
      go = w.x > 0.f || w.y > 0.f || w.z > 0.f; // a NaN or zero weight ends the path
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(go);
    if (m) {
      const uint32_t lane =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      uint32_t base = 0;
      if ((threadIdx.x & 63) == 0) base = atomicAdd(T.n_out, (uint32_t)__popcll(m));
      base = (uint32_t)__shfl((int)base, 0, 64);
      const int64_t slot = (int64_t)base + lane;
      if (go && slot < cap) {
        if (!glass) {
          const float sn = dot(d, N);
          const f3 Nf = (sn > 0.f) ? mk(-N.x, -N.y, -N.z) : N;
          o2 = (o + d * s.t) + Nf * T.bias;
          d2 = normalize(d - N * (2.f * sn));
        }
        float *q = T.q_out + slot;
        q[0] = o2.x;
        q[cap] = o2.y;
        q[2 * cap] = o2.z;
        q[3 * cap] = d2.x;
        q[4 * cap] = d2.y;
        q[5 * cap] = d2.z;
        q[6 * cap] = w.x;
        q[7 * cap] = w.y;
        q[8 * cap] = w.z;
        q[9 * cap] = __uint_as_float(dest);
      }
    }
  }

  // stats: wave reductions, then one ordinary global atomic per wave and counter that has something to
  // add.  All of them land on one cache line, and on light scenes these same-address atomics bound the
  // kernel (k_shade_rays' five per wave are 7.8 of c4's 7.8 ms at 4K), so the total of rays is not kept
  // here: esc_last_trace_stats sums depth_rays.
  const unsigned long long rays = __popcll(__builtin_amdgcn_ballot_w64(valid));
  const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(has_hit));
  const unsigned long long shadow = wave_sum64(n_shadow);
  const unsigned long long exact = wave_sum64(n_exact);
  tests = wave_sum64(tests);
  if ((threadIdx.x & 63) == 0 && rays) {
    atomicAdd(&P.stats[5 + T.level], rays);
    if (hits) atomicAdd(&P.stats[1], hits);
    if (shadow) atomicAdd(&P.stats[2], shadow);
    if (exact) atomicAdd(&P.stats[3], exact);
    if (tests) atomicAdd(&P.stats[4], tests);
  }
  if constexpr (TRANSMIT && !LAST) { // esc_transmit_stats, the same way
    const unsigned long long n1 = __popcll(__builtin_amdgcn_ballot_w64(what == kBounceRefracted));
    const unsigned long long n2 = __popcll(__builtin_amdgcn_ballot_w64(what == kBounceFresnel));
    const unsigned long long n3 = __popcll(__builtin_amdgcn_ballot_w64(what == kBounceTotalInternal));
    if ((threadIdx.x & 63) == 0) {
      if (n1) atomicAdd(&P.stats[kTraceStats + 0], n1);
      if (n2) atomicAdd(&P.stats[kTraceStats + 1], n2);
      if (n3) atomicAdd(&P.stats[kTraceStats + 2], n3);
    }
  }
}

} // namespace esc

extern "C" int esc_launch_trace_level(const esc::TraceParams *p, hipStream_t stream) {
  if (p->s.q.n <= 0) return 0;
  const dim3 grid((unsigned)((p->s.q.n + 255) / 256));
  const bool first = p->level == 0, last = p->level == p->max_depth;
  // a last level never bounces: <*, true, true> would be <*, true, false>
  const bool transmit = p->transmit != nullptr && p->transmit_mode != esc::kTransmitOff && !last;
  const bool env = p->env.texels != nullptr;
#define TRACE_LAUNCH(F, L, X)                                                                                   \
  do {                                                                                                          \
    if (env)                                                                                                    \
      hipLaunchKernelGGL((esc::k_trace<F, L, X, true>), grid, dim3(256), 0, stream, *p);                        \
    else                                                                                                        \
      hipLaunchKernelGGL((esc::k_trace<F, L, X, false>), grid, dim3(256), 0, stream, *p);                       \
  } while (0)
  if (first && last)
    TRACE_LAUNCH(true, true, false);
  else if (last)
    TRACE_LAUNCH(false, true, false);
  else if (first && transmit)
    TRACE_LAUNCH(true, false, true);
  else if (first)
    TRACE_LAUNCH(true, false, false);
  else if (transmit)
    TRACE_LAUNCH(false, false, true);
  else
    TRACE_LAUNCH(false, false, false);
#undef TRACE_LAUNCH
  return (int)hipGetLastError();
}
