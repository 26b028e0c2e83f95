// rt_adaptive.hip -- adaptive supersampling (esc_render_adaptive): the base frame comes
// from the frame kernels; these kernels find the pixels on an edge and give only those spp samples.
//
//   k_adaptive_mask    M[h,w] = some 4-neighbour inside the frame and some channel has
//                      !(|B[h,w,c] - B[h',w',c]| <= threshold), over the WHOLE frame, before any refined
//                      value is stored (the image is refined in place)
//   k_adaptive_list    the ids of a band's masked pixels: wave ballot, lane prefix by mbcnt, ONE ordinary
//                      global atomic add per wave on the list's counter, then plain vector stores
//                      (k_trace's append).  The order of the list is not fixed; every id owns its pixel,
//                      so the image does not depend on it.
//   k_adaptive_refine  one lane takes one SAMPLE of a listed pixel: a workgroup of 256 lanes holds 256 / spp
//                      listed pixels, lane j * spp + k sample k of its j-th (256 % spp lanes idle).  The grid
//                      covers the band's pixel count; a workgroup reads the live count from device memory
//                      and leaves if it lies past it (k_trace<!FIRST>).  Per lane: the camera ray of
//                      k_camera_rays made in-lane (rt_camera_ray.h), k_shade_rays' body
//                      (rt_shade_body.inc, one copy) with the listed id as pixel id and seed + k; the colour
//                      goes to LDS, and after one barrier lane j sums its pixel's spp colours in sample
//                      order (acc = 0; acc += rgb_k), divides by spp and stores fp32 and u8 once.  No ray
//                      and no colour goes through memory.  The counters are reduced per wave, then per
//                      workgroup through LDS: at most one global atomic per workgroup and counter.  Why not one lane per PIXEL with a loop over the
//                      samples: a frame's edges are a few thousand wavefronts, which then run spp shading
//                      bodies back to back on a mostly empty chip (DESIGN.md §3.16 has both measured).
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt): a
// refined pixel has the bits esc_render_supersampled gives it.  The refinement reads only per-scene
// tables, like k_shade_rays.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_camera_ray.h"
#include "rt_shade_body.h"

namespace esc {

namespace {

// some channel of the two pixels differs by more than the threshold, or the difference is NaN
DEVINL bool over(const float *a, const float *b, float thr) {
  return !(fabsf(a[0] - b[0]) <= thr) || !(fabsf(a[1] - b[1]) <= thr) || !(fabsf(a[2] - b[2]) <= thr);
}

} // namespace

__global__ __launch_bounds__(256) void k_adaptive_mask(const AdaptiveMaskParams p) {
  const int64_t total = (int64_t)p.W * p.H;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int h = (int)(i / p.W), w = (int)(i % p.W);
  const float *c = p.image + 3 * i;
  bool m = false;
  if (w > 0) m = m || over(c, c - 3, p.threshold);
  if (w + 1 < p.W) m = m || over(c, c + 3, p.threshold);
  if (h > 0) m = m || over(c, c - 3 * (int64_t)p.W, p.threshold);
  if (h + 1 < p.H) m = m || over(c, c + 3 * (int64_t)p.W, p.threshold);
  p.mask[i] = m ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_adaptive_list(const AdaptiveListParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool go = i < p.n && p.mask[p.pix0 + i] != 0;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(go);
  if (!m) return;
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  uint32_t base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(p.count, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, 0, 64);
  const int64_t slot = (int64_t)base + lane;
  if (go && slot < p.n) p.list[slot] = (uint32_t)(p.pix0 + i); // at most one id per pixel of the band
}

__global__ __launch_bounds__(256) void k_adaptive_refine(const AdaptiveRefineParams A) {
  const ShadeParams &P = A.s;
  const QueryParams &p = P.q;
  __shared__ float colour[3 * 256]; // r, g, b of the workgroup's samples, sample k of local pixel j at j * spp + k
  __shared__ unsigned long long counts[4 * kAdaptiveStats]; // esc_adaptive_stats' counters of the four waves
  const int64_t cap = p.n;
  int64_t n = (int64_t)*A.count;
  if (n > cap) n = cap; // one id per pixel of the band bounds the count; this keeps every index in bounds
  const int ppw = 256 / A.spp; // listed pixels per workgroup (spp <= 64: at least 4); 256 % spp lanes idle
  const int64_t first = (int64_t)blockIdx.x * ppw;
  if (first >= n) return; // the whole workgroup: nobody is left waiting at the barrier below
  const int tid = (int)threadIdx.x;
  const int lp = tid / A.spp, sk = tid - lp * A.spp; // local pixel, sample
  bool valid = lp < ppw && first + lp < n;
  uint32_t pix = 0;
  if (valid) {
    pix = A.list[first + lp];
    valid = (int64_t)pix < (int64_t)A.W * A.H; // always true; an id that is not is left alone, not written
  }
  const int h = (int)(pix / (uint32_t)A.W), w = (int)(pix % (uint32_t)A.W);
  const f3 origin = mk(A.origin[0], A.origin[1], A.origin[2]);
  const f3 o = valid ? origin : mk(0.f, 0.f, 0.f);
  // sample sk = j*n + i at (i + 1/2)/n - 1/2, (j + 1/2)/n - 1/2 pixels (fp32), esc_render_supersampled's
  const float dx = ((float)(sk % A.nn) + 0.5f) / (float)A.nn - 0.5f;
  const float dy = ((float)(sk / A.nn) + 0.5f) / (float)A.nn - 0.5f;
  f3 d = mk(0.f, 0.f, 0.f);
  if (valid) d = camera_ray_dir(origin, A.llc, A.horizontal, A.vertical, A.W, A.H, w, h, dx, dy);

#define SHADE_BODY_SEED (P.seed + (uint64_t)sk)
#define SHADE_BODY_PIXEL pix
#include "rt_shade_body.inc"
#undef SHADE_BODY_PIXEL
#undef SHADE_BODY_SEED

  colour[3 * tid] = r;
  colour[3 * tid + 1] = g;
  colour[3 * tid + 2] = b;
  // stats: wave reductions into LDS here, one workgroup sum after the barrier
  {
    const unsigned long long pixels = __popcll(__builtin_amdgcn_ballot_w64(valid && sk == 0));
    const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(has_hit));
    const unsigned long long shadow = wave_sum64(n_shadow);
    const unsigned long long exact = wave_sum64(n_exact);
    tests = wave_sum64(tests);
    if ((tid & 63) == 0) {
      unsigned long long *c = counts + kAdaptiveStats * (tid >> 6);
      c[0] = pixels;
      c[1] = hits;
      c[2] = shadow;
      c[3] = exact;
      c[4] = tests;
    }
  }
  __syncthreads();
  // lane j < ppw finishes local pixel j: acc = 0; acc += rgb_k for k = 0 .. spp-1 in that order; acc / spp
  if (tid < ppw && first + tid < n) {
    const uint32_t q = A.list[first + tid];
    if ((int64_t)q < (int64_t)A.W * A.H) {
      float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f;
      const float *c = colour + 3 * tid * A.spp;
      for (int k = 0; k < A.spp; ++k) {
        acc_r = acc_r + c[3 * k];
        acc_g = acc_g + c[3 * k + 1];
        acc_b = acc_b + c[3 * k + 2];
      }
      const float spp = (float)A.spp;
      const float vr = acc_r / spp, vg = acc_g / spp, vb = acc_b / spp;
      float *C = P.rgb + 3 * (int64_t)q;
      C[0] = vr;
      C[1] = vg;
      C[2] = vb;
      if (P.rgb8) {
        uint8_t *C8 = P.rgb8 + 3 * (int64_t)q;
        C8[0] = quantise_channel(vr);
        C8[1] = quantise_channel(vg);
        C8[2] = quantise_channel(vb);
      }
    }
  }

  // ... then one ordinary global atomic per WORKGROUP and counter that has something to add: these
  // same-address atomics are what bounds k_shade_rays on light scenes (rt_trace.hip), and a workgroup here
  // holds 256 / spp pixels only
  if (tid < kAdaptiveStats) {
    const unsigned long long v = counts[tid] + counts[kAdaptiveStats + tid] + counts[2 * kAdaptiveStats + tid] +
                                 counts[3 * kAdaptiveStats + tid];
    if (v) atomicAdd(&P.stats[tid], v);
  }
}

} // namespace esc

static dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" int esc_launch_adaptive_mask(const esc::AdaptiveMaskParams *p, hipStream_t stream) {
  const int64_t total = (int64_t)p->W * p->H;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(esc::k_adaptive_mask, grid_of(total), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_adaptive_list(const esc::AdaptiveListParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_adaptive_list, grid_of(p->n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_adaptive_refine(const esc::AdaptiveRefineParams *p, hipStream_t stream) {
  if (p->s.q.n <= 0 || p->spp < 1 || p->spp > 64) return 0;
  const int64_t ppw = 256 / p->spp; // listed pixels per workgroup
  const dim3 grid((unsigned)((p->s.q.n + ppw - 1) / ppw));
  hipLaunchKernelGGL(esc::k_adaptive_refine, grid, dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
