// rt_query.h -- parameter block of the batched ray queries (esc_intersect_rays / esc_occluded_rays).
// Shared by rt_query.hip (device) and rt_capi.cpp (host).  Every table it points to is a per-scene
// table of the uploaded scene (rt_device.h); a query reads no per-camera state.
#pragma once
#include <stdint.h>

#include "rt_device.h"

namespace esc {

struct QueryParams {
  int64_t n;
  const float *orig; // n x 3
  const float *dir;  // n x 3
  const float *tmax; // n, or nullptr: FLT_MAX (main.cpp:715)
  float *t;          // closest hit: n
  int32_t *geom, *prim;
  float *uv;         // n x 2, or nullptr
  uint8_t *occ;      // occlusion: n
  int32_t n_tri, n_sph;
  const DevTri *tri;          // index order; pad[0] holds the face index (staging)
  const DevSph *sph;          // index order
  const DevSphPairF *sph2_f;  // shadow-ray (arbitrary origin) filter forms, index order
  const DevTriPairF *tri2_f;
  const DevTriPairPF *tri2_pf;
  SphGroups sg;               // only the static shadow-ray fields are read
  TriGroups tg;
  float g[3];                 // RenderParams::shadow_center
  float rho_max;              // RenderParams::shadow_rho_max
  int32_t exact_only;         // ESC_RENDER_EXACT_ONLY: every pair, reference arithmetic, index order
  int32_t pad;
  unsigned long long *stats;  // esc_query_stats: rays, exact_rays, exact_tests (zeroed per call)
};

} // namespace esc
