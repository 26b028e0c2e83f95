// rt_lens.h -- parameter block of the thin-lens ray generator (esc_lens_rays / esc_render_lens, DESIGN.md
// §3.22; the definition is in include/esctp1_rt.h at esc_lens_options).  Shared by rt_lens.hip (device) and
// rt_capi.cpp (host).
#pragma once
#include <math.h>
#include <stdint.h>

namespace esc {

constexpr int kLensMaxDim = 64;               // sets and samples of the lens table: 1..64 each
constexpr uint32_t kLensLight = 0xFFFFFFFDu;  // the hash's light index: no light reaches it, and it is
                                              // neither the ambient set's (..FE) nor the Fresnel draw's (..FF)

struct LensRayParams {
  float origin[3], llc[3], horizontal[3], vertical[3];
  float U[3], V[3];           // normalize(horizontal), normalize(vertical) (lens_axis below); unused at aperture 0
  float aperture, focus_dist;
  int32_t W, H;
  int64_t pix0;               // ray i is pixel pix0 + i of the frame: h = pix / W, w = pix % W
  int64_t n;
  const float *offsets;       // n x 2 (dx, dy), or nullptr: (dx, dy) below for every ray
  float dx, dy;
  const float *table;         // sets x samples x 2 points of the unit disk; nullptr only at aperture 0
  int32_t sets, samples;
  int32_t sample;             // the lens sample k of every ray of this launch, 0 .. samples - 1
  int32_t pad;
  uint64_t seed;              // esc_lens_options.seed: picks the pixel's set
  float *orig, *dir;          // n x 3 each
};

// normalize (rt_math.h, vec.h:135) of a camera axis on the host: the same fp32 operations in the same order,
// one rounding each (the host objects are compiled without contraction, like the kernels)
inline void lens_axis(const float v[3], float out[3]) {
  const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  out[0] = v[0] / len;
  out[1] = v[1] / len;
  out[2] = v[2] / len;
}

} // namespace esc
