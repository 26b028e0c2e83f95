// rt_temporal.hip -- temporal accumulation of esc_temporal_accumulate (the definition is in
// include/esctp1_rt.h at esc_temporal_options): every hit pixel's world-space point is projected into the
// previous frame's camera (the inverse of camera.h:31-34 get_ray, a 3 x 3 solve by Cramer's rule), the 1 or
// 2 x 2 history pixels around that point are accepted or rejected by the filter's compares on the guides
// (hit, history length, object, normal, plane), and the new estimate is blended into their mean.
//
//   k_temporal<CH, TAPS>  CH = 1 or 3 interleaved channels, TAPS = 1 (nearest) or 4 (bilinear): one pixel per
//                         lane, tiles of 64 x 4 pixels, 64-bit pixel indices.  The previous frame's guides
//                         are read from their four arrays as they are: a record is needed about once per
//                         pixel (at most 4 times), so packing them first would move more bytes than it saves.
//
// Same arithmetic contract as rt_filter.hip (-ffp-contract=off, correctly rounded divide): only + - * /,
// floorf and compares.  Every lane owns its pixel's whole sum, taps in the order (0,0) (0,1) (1,0) (1,1) of
// (j, i), whatever the kernel's shape.  The tap coordinates stay floats until they have passed the range
// test: a NaN or a huge value never reaches a cast or an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_math.h"
#include "rt_temporal.h"

namespace esc {
namespace {

DEVINL uint32_t temporal_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

} // namespace

template <int CH, int TAPS>
__global__ __launch_bounds__(256) void k_temporal(const TemporalParams A) {
  const int64_t tile = blockIdx.x;
  const int64_t w = (tile % A.tiles_x) * kTemporalTileW + (threadIdx.x & (kTemporalTileW - 1));
  const int64_t h = (tile / A.tiles_x) * kTemporalTileH + (threadIdx.x / kTemporalTileW);
  const bool valid = w < A.W && h < A.H;
  bool hit = false, reused = false;
  uint32_t tested = 0, accepted = 0;
  if (valid) {
    const int64_t pi = h * A.W + w;
    const int32_t geom_p = A.cur.geom[pi], prim_p = A.cur.prim[pi];
    float cur[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) cur[c] = A.current[pi * CH + c];
    hit = geom_p >= 0 || prim_p >= 0;
    if (!hit) {
#pragma unroll
      for (int c = 0; c < CH; ++c) A.out[pi * CH + c] = cur[c];
      A.out_n[pi] = 0;
    } else {
      const f3 Np = ld3(A.cur.normal + 3 * pi), Pp = ld3(A.cur.position + 3 * pi);
      // x Hh + y V + z v = Av: the previous camera's ray through s = -x, t = -y passes through Pp
      const f3 O = ld3(A.origin), Hh = ld3(A.horizontal), V = ld3(A.vertical);
      const f3 Av = ld3(A.lower_left_corner) - O;
      const f3 v = Pp - O;
      const f3 cv = cross(V, v);
      const float det = dot(Hh, cv);
      const float x = dot(Av, cv) / det;
      const float y = dot(Hh, cross(Av, v)) / det;
      const float z = dot(Hh, cross(V, Av)) / det;
      const float fx = (-x) * float(A.W - 1), fy = (-y) * float(A.H - 1);
      const bool inside = z > 0.f && fx >= -1.f && fx <= float(A.W) && fy >= -1.f && fy <= float(A.H);
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = 0.f;
      float ws = 0.f;
      int32_t n = INT32_MAX;
      if (inside) {
        float x0, y0, ax = 0.f, ay = 0.f;
        if (TAPS == 1) {
          x0 = floorf(fx + 0.5f);
          y0 = floorf(fy + 0.5f);
        } else {
          x0 = floorf(fx);
          ax = fx - x0;
          y0 = floorf(fy);
          ay = fy - y0;
        }
        const float wmax = float(A.W - 1), hmax = float(A.H - 1);
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
          const int i = t & 1, j = t >> 1;
          const float qx = x0 + float(i), qy = y0 + float(j);
          if (!(qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax)) continue;
          const float k = TAPS == 1 ? 1.f : (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay);
          if (!(k > 0.f)) continue;
          ++tested;
          const int64_t qi = (int64_t)qy * A.W + (int64_t)qx; // both inside the image, tested as floats above
          const int32_t geom_q = A.prev.geom[qi], prim_q = A.prev.prim[qi];
          if (!(geom_q >= 0 || prim_q >= 0)) continue;
          const int32_t nq = A.history_n[qi];
          if (!(nq >= 1)) continue;
          if (A.same_object && !(geom_q == geom_p && (geom_p >= 0 || prim_q == prim_p))) continue;
          if (!(dot(Np, ld3(A.prev.normal + 3 * qi)) >= A.normal_cos)) continue;
          const f3 df = ld3(A.prev.position + 3 * qi) - Pp;
          if (!(fabsf(dot(df, Np)) <= A.plane_dist)) continue;
          ++accepted;
#pragma unroll
          for (int c = 0; c < CH; ++c) acc[c] = acc[c] + k * A.history[qi * CH + c];
          ws = ws + k;
          n = nq < n ? nq : n;
        }
      }
      if (!(ws > 0.f)) {
#pragma unroll
        for (int c = 0; c < CH; ++c) A.out[pi * CH + c] = cur[c];
        A.out_n[pi] = 1;
      } else {
        reused = true;
        const int32_t m = (n < A.max_history - 1 ? n : A.max_history - 1) + 1;
        const float alpha = 1.f / float(m);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float hc = acc[c] / ws;
          A.out[pi * CH + c] = hc + (cur[c] - hc) * alpha;
        }
        A.out_n[pi] = m;
      }
    }
  }
  // stats: wave reductions, then one ordinary global atomic per wave and counter that has something to add, into
  // the workgroup's replica of the counters
  const unsigned long long nh = __popcll(__builtin_amdgcn_ballot_w64(hit));
  const unsigned long long nr = __popcll(__builtin_amdgcn_ballot_w64(reused));
  const unsigned long long nt = temporal_wave_sum(tested), na = temporal_wave_sum(accepted);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *st = A.stats + (blockIdx.x % kTemporalStatSets) * 8;
    if (nh) atomicAdd(&st[0], nh);
    if (nr) atomicAdd(&st[1], nr);
    if (nt) atomicAdd(&st[2], nt);
    if (na) atomicAdd(&st[3], na);
  }
}

} // namespace esc

// tiles: tiles_x * ceil(H / kTemporalTileH), checked by the caller to fit one launch
extern "C" int esc_launch_temporal(const esc::TemporalParams *p, int channels, int taps, int64_t tiles,
                                   hipStream_t stream) {
  if (tiles <= 0) return 0;
  const dim3 grid((unsigned)tiles), block(256);
  if (channels == 3 && taps == 4)
    hipLaunchKernelGGL((esc::k_temporal<3, 4>), grid, block, 0, stream, *p);
  else if (channels == 3)
    hipLaunchKernelGGL((esc::k_temporal<3, 1>), grid, block, 0, stream, *p);
  else if (taps == 4)
    hipLaunchKernelGGL((esc::k_temporal<1, 4>), grid, block, 0, stream, *p);
  else
    hipLaunchKernelGGL((esc::k_temporal<1, 1>), grid, block, 0, stream, *p);
  return (int)hipGetLastError();
}
