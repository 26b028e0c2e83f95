// rt_temporal.h -- parameter block of the temporal accumulation (esc_temporal_accumulate).
// Shared by rt_temporal.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

namespace esc {

constexpr int kTemporalStats = 4;     // hit_pixels, reused_pixels, taps_tested, taps_accepted (pixels is W*H)
// replicas of the counters, 64 B (8 words) each so that every one has a cache line of its own, summed on read:
// a workgroup adds to replica blockIdx.x % kTemporalStatSets (atomics on one line run one after the other)
constexpr int kTemporalStatSets = 64;
constexpr int kTemporalMaxHistory = 65536;
constexpr int kTemporalTileW = 64, kTemporalTileH = 4; // one workgroup: a wave per row segment of 64 pixels

struct TemporalGuides {
  const float *normal;      // W*H x 3
  const float *position;    // W*H x 3
  const int32_t *geom, *prim;
};

struct TemporalParams {
  int32_t W, H;
  int32_t same_object;
  int32_t max_history;      // M
  float normal_cos, plane_dist;
  float origin[3], lower_left_corner[3], horizontal[3], vertical[3]; // the previous frame's camera
  int64_t tiles_x;          // ceil(W / kTemporalTileW)
  const float *current;     // W*H x channels; may be `out`: a lane reads only its own pixel of it
  TemporalGuides cur, prev;
  const float *history;     // W*H x channels, never `out`
  const int32_t *history_n; // W*H, never `out_n`
  float *out;               // W*H x channels
  int32_t *out_n;           // W*H
  unsigned long long *stats; // kTemporalStatSets x 8 words, zeroed per call
};

} // namespace esc
