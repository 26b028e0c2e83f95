// rt_trace.h -- parameter block of one depth level of the bounce loop (esc_trace_rays,
// esc_render_traced and their _ex forms).  Shared by rt_trace.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

#include "rt_environ.h"
#include "rt_shade_rays.h"

namespace esc {

constexpr int kTraceMaxDepth = 16;
constexpr int kTraceQueuePlanes = 10; // ox oy oz dx dy dz wr wg wb dest, `cap` dwords each (SoA)
constexpr int kTraceStats = 5 + kTraceMaxDepth + 1; // esc_trace_stats, see TraceParams::s
constexpr int kTransmitStats = 3; // esc_transmit_stats, right after them in the same array

struct TraceParams {
  // s.q.n = the batch's rays = the capacity of either queue; s.q.orig / s.q.dir = the level-0 rays;
  // s.rgb / s.rgb8 = the accumulated colour C per destination; s.seed = the level's seed
  // (opts.seed + 64 * level, plus the sample index of a supersampled frame); s.t / geom / prim null;
  // s.stats = esc_trace_stats as 5 + 17 counters: (unused), hit_rays, shadow_rays, exact_rays,
  // exact_tests, depth_rays[0..16]; then refracted, fresnel_reflected, total_internal
  ShadeParams s;
  int32_t level, max_depth;
  float bias;
  int32_t pad;
  const float *q_in;     // level >= 1: the rays of this level
  float *q_out;          // survivors, for level + 1
  const uint32_t *n_in;  // level >= 1: how many rays q_in holds (device memory; the host never reads it)
  uint32_t *n_out;       // zero before the launch
  // k_trace<*, *, true> only (the fields sit at the end so that the other instantiations read theirs
  // where they always were): tf[3], ni per material, indexed like s.mat; ESC_TRANSMIT_REFRACT / _FRESNEL
  const float *transmit;
  int32_t transmit_mode;
  int32_t pad2;
  // k_trace<*, *, *, true> only, and at the end for the same reason: the context's environment cube
  // (esc_set_environment); texels == nullptr selects the kernels without the lookup
  EnvParams env;
};

} // namespace esc
