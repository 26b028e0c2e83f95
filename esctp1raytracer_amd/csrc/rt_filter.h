// rt_filter.h -- parameter blocks of the edge-stopping a-trous filter (esc_filter_guided).
// Shared by rt_filter.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

namespace esc {

constexpr int kFilterStats = 3;   // hit_pixels, taps_tested, taps_accepted (pixels is W*H, known to the host)
constexpr int kFilterMaxIter = 8; // step 2^7 = 128 pixels at most
constexpr int kFilterTileW = 64, kFilterTileH = 4; // one workgroup: a wave per row segment of 64 pixels

// 32 bytes per pixel, written once per call by k_filter_pack: two 16-byte loads per tap
struct FilterGuide {
  float n[3];
  int32_t geom;
  float p[3];
  int32_t prim;
};
static_assert(sizeof(FilterGuide) == 32, "two 16-byte pieces");

struct FilterPackParams {
  int64_t n;                // W*H
  const float *normal;      // n x 3
  const float *position;    // n x 3
  const int32_t *geom, *prim;
  FilterGuide *guide;       // n
  unsigned long long *stats; // kFilterStats counters (zeroed per call): the pack counts hit_pixels
};

struct FilterParams {
  int32_t W, H;
  int32_t step;             // 2^i
  int32_t same_object;
  float normal_cos, plane_dist;
  int64_t tiles_x;          // ceil(W / kFilterTileW)
  const FilterGuide *guide; // W*H
  const float *in;          // W*H x channels
  float *out;               // W*H x channels, never `in`
  unsigned long long *stats;
};

} // namespace esc
