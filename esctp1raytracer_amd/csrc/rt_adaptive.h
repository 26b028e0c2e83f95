// rt_adaptive.h -- parameter blocks of adaptive supersampling (esc_render_adaptive): the edge mask over
// the base frame, the list of a band's masked pixels, and the refinement of the listed pixels.
// Shared by rt_adaptive.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

#include "rt_shade_rays.h"

namespace esc {

constexpr int kAdaptiveStats = 5; // refined_pixels, hit_rays, shadow_rays, exact_rays, exact_tests

struct AdaptiveMaskParams {
  const float *image; // the base frame B, W*H*3
  uint8_t *mask;      // W*H
  int32_t W, H;
  float threshold;
  int32_t pad;
};

struct AdaptiveListParams {
  const uint8_t *mask; // W*H
  uint32_t *list;      // `n` slots: the ids h*W + w of the band's masked pixels, in no fixed order
  uint32_t *count;     // zero before the launch
  int64_t pix0, n;     // the band: pixels [pix0, pix0 + n) of the frame
};

struct AdaptiveRefineParams {
  // s.q.n = the band's pixel count = the capacity of the list; s.q.orig / s.q.dir unused (the rays are
  // made in-lane); s.rgb / s.rgb8 = the WHOLE frame (a listed id indexes it); s.seed = opts.seed (sample k
  // adds k); s.pixel_base unused (the listed id is the pixel id); s.stats = kAdaptiveStats counters
  ShadeParams s;
  float origin[3], llc[3], horizontal[3], vertical[3];
  int32_t W, H;
  int32_t spp, nn;        // spp = nn * nn
  const uint32_t *list;
  const uint32_t *count;  // how many ids the list holds (device memory; the host never reads it)
};

} // namespace esc
