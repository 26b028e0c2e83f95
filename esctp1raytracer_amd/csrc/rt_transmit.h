// rt_transmit.h -- refraction at a bounce of the trace loop (esc_trace_rays_ex; the
// definition is in include/esctp1_rt.h at esc_trace_options).  Included by rt_trace.hip only: the
// frame, query and shade kernels do not see it and keep their instruction streams.
//
// Arithmetic contract of rt_kernels.hip: fp32, one rounding per written operation, no contraction,
// correctly rounded divide and sqrt.  Every expression below is written in the order the header gives.
#pragma once
#include <stdint.h>

#include "rt_math.h"

namespace esc {

constexpr int kTransmitOff = 0, kTransmitRefract = 1, kTransmitFresnel = 2; // ESC_TRANSMIT_*
constexpr int kTransmitFloats = 4;                                          // tf[3], ni per material
constexpr uint32_t kTransmitLight = 0xFFFFFFFFu; // the hash's light index: no light reaches it

// what a bounce did, for esc_transmit_stats
enum : uint32_t { kBounceMirror = 0, kBounceRefracted = 1, kBounceFresnel = 2, kBounceTotalInternal = 3 };

// face_hash's mixer (rt_math.h) before the modulo: the high 32 bits of splitmix64's finaliser
DEVINL uint32_t mix_hi32(uint64_t seed, uint32_t pixel, uint32_t light) {
  uint64_t z = seed + (((uint64_t)pixel << 32) | (uint64_t)light) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

// a NaN in any term makes the material opaque
DEVINL bool transmissive(float tr, float tg, float tb, float ni) {
  return (tr > 0.f || tg > 0.f || tb > 0.f) && ni > 0.f;
}

// The bounce at a transmissive hit: ray (o, d) met the surface at o + d * t0 with shading normal N.
// Writes the next ray (o2, d2), scales w by tf when the ray refracts, and returns what happened.  `go`
// comes back false when the refracted weight has no positive channel.
DEVINL uint32_t transmit_bounce(int mode, uint64_t seed, uint32_t pixel, f3 tf, float ni, float bias, f3 o,
                                f3 d, float t0, f3 N, f3 &w, f3 &o2, f3 &d2, bool &go) {
  const float s = dot(d, N);
  const f3 Nf = (s > 0.f) ? mk(-N.x, -N.y, -N.z) : N;
  const float c1 = (s > 0.f) ? s : -s;
  const float eta = (s > 0.f) ? ni : 1.f / ni; // s > 0: the ray leaves the medium
  const float k = 1.f - (eta * eta) * (1.f - c1 * c1);
  bool reflect = !(k >= 0.f); // total internal reflection; also a NaN k
  uint32_t what = reflect ? kBounceTotalInternal : kBounceRefracted;
  if (!reflect && mode == kTransmitFresnel) {
    float r0 = (ni - 1.f) / (ni + 1.f);
    r0 = r0 * r0;
    const float cx = (s > 0.f) ? sqrtf(k) : c1; // the cosine on the outside of the surface
    const float m = 1.f - cx;
    const float m2 = m * m;
    const float F = r0 + (1.f - r0) * ((m2 * m2) * m);
    const float u = (float)(mix_hi32(seed, pixel, kTransmitLight) >> 8) * 0x1p-24f;
    reflect = u < F;
    if (reflect) what = kBounceFresnel;
  }
  const f3 P = o + d * t0;
  if (reflect) {
    o2 = P + Nf * bias;
    d2 = normalize(d - N * (2.f * s));
    go = true;
  } else {
    w = mk(w.x * tf.x, w.y * tf.y, w.z * tf.z);
    go = w.x > 0.f || w.y > 0.f || w.z > 0.f;
    o2 = P - Nf * bias;
    d2 = normalize(d * eta + Nf * (eta * c1 - sqrtf(k)));
  }
  return what;
}

} // namespace esc
