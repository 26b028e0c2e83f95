// rt_gbuffer.h -- parameter block of the G-buffer of rays and frames (esc_gbuffer_rays / esc_render_gbuffer,
// DESIGN.md §3.20).  Shared by rt_gbuffer.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

#include "rt_device.h"
#include "rt_query.h"

namespace esc {

constexpr int kGBufferStats = 4; // rays, hit_rays, exact_rays, exact_tests

struct GBufferParams {
  // q.n, the per-scene sweep tables and exact_only; q.orig / q.dir are the caller's rays (the frame variant
  // makes its rays in-lane and leaves them null); q.tmax and q's outputs are unused
  QueryParams q;
  float *normal, *position, *albedo; // n x 3 each, or nullptr (each of the six, not all)
  float *t;                          // n
  int32_t *geom, *prim;              // n
  const DevTriN *tri_n;              // vertex normals (nullptr when no geometry has them)
  const DevMat *mat;
  const int32_t *sph_mat;            // material index of sphere k (already offset by n_geom)
  // the frame variant: ray i is pixel i of the W x H frame (h = i / W, w = i % W)
  int32_t W, H;
  float origin[3], llc[3], horizontal[3], vertical[3];
  unsigned long long *stats;         // kGBufferStats counters (zeroed per call)
};

} // namespace esc
