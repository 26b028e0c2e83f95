// rt_shade_body.h -- the helpers of scan_row's body (rt_shade_body.inc): one sweep of a ray in a given
// accumulator mode, the lane's start state, a 64-bit wave sum.  Included by rt_shade_rays.hip and
// rt_trace.hip ahead of the body.  The sweeps and the precondition gate are rt_query_sweep.h's.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_query_sweep.h"
#include "rt_shade.h"
#include "rt_shade_rays.h"

namespace esc {
namespace {

// one sweep of ray s in accumulator MODE: the filtered sweep for the lanes in `elig`, the exact
// (index-order) sweep for the lanes in `need`
template <int MODE>
DEVINL void sweep(const QueryParams &p, bool elig, bool need, const RayF &rs, const RayTF &rt, QLane &s) {
  s.live = elig;
  if (__builtin_amdgcn_ballot_w64(elig)) {
    if (p.n_tri > 0) {
      if (p.tg.n_grp > 0) tri_groups<MODE>(p, rs, rt, s);
      else tri_linear<MODE>(p, rs, rt, s);
    }
    // every sphere's index is above every triangle's: a triangle occluder is already the first
    if (MODE == kFirst) s.live = s.live && s.id < 0;
    if (p.n_sph > 0) {
      if (p.sg.n_grp > 0) sph_groups<MODE>(p, rs, s);
      else sph_linear<MODE>(p, rs, s);
    }
  }
  s.live = false;
  exact_sweep<MODE>(p, need, s);
}

DEVINL void lane_init(QLane &s, f3 o, f3 L, float tmax) {
  s.o = o;
  s.L = L;
  s.tmax = tmax;
  s.t = tmax;
  s.u = s.v = 0.f;
  s.id = -1;
  s.live = false;
  s.occ = false;
  s.tests = 0;
}

DEVINL unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

} // namespace
} // namespace esc
