// rt_filter.hip -- the edge-stopping a-trous filter of esc_filter_guided (the definition is
// in include/esctp1_rt.h at esc_filter_options): L iterations of a 5 x 5 B3-spline kernel with holes of
// 2^i pixels, whose taps are accepted or rejected by compares on the guides (hit, object, normal, plane) and
// never weighted by anything but the kernel's dyadic constants.
//
//   k_filter_pack         once per call: normal, position, geom, prim -> one 32-byte record per pixel
//                         (N.xyz, geom | P.xyz, prim), so a tap costs two 16-byte loads; counts hit_pixels
//   k_filter_atrous<CH>   one launch per iteration, CH = 1 or 3 interleaved channels: one pixel per lane,
//                         tiles of 64 x 4 pixels (a wave reads 64 consecutive records per tap row), 64-bit
//                         pixel indices.  Every tap is read through L2: at step s the 25 taps of a tile
//                         cover (64 + 4s) x (4 + 4s) pixels, which neighbouring tiles share in cache.
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide): only + - * / and
// compares.  The sums run dy ascending, inside it dx ascending, whatever the kernel's shape: every lane owns
// its pixel's whole sum.  No iteration reads what it writes (the host alternates two images).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_filter.h"
#include "rt_math.h"

namespace esc {
namespace {

DEVINL unsigned long long filter_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

} // namespace

__global__ __launch_bounds__(256) void k_filter_pack(const FilterPackParams A) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < A.n;
  bool hit = false;
  if (valid) {
    const int32_t geom = A.geom[i], prim = A.prim[i];
    hit = geom >= 0 || prim >= 0;
    float4 a, b;
    a.x = A.normal[3 * i];
    a.y = A.normal[3 * i + 1];
    a.z = A.normal[3 * i + 2];
    a.w = __int_as_float(geom);
    b.x = A.position[3 * i];
    b.y = A.position[3 * i + 1];
    b.z = A.position[3 * i + 2];
    b.w = __int_as_float(prim);
    float4 *g = reinterpret_cast<float4 *>(A.guide + i);
    g[0] = a;
    g[1] = b;
  }
  const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(hit));
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&A.stats[0], hits);
}

template <int CH>
__global__ __launch_bounds__(256) void k_filter_atrous(const FilterParams A) {
  constexpr float K1[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}; // the products are exact in fp32
  const int64_t tile = blockIdx.x;
  const int64_t w = (tile % A.tiles_x) * kFilterTileW + (threadIdx.x & (kFilterTileW - 1));
  const int64_t h = (tile / A.tiles_x) * kFilterTileH + (threadIdx.x / kFilterTileW);
  const bool valid = w < A.W && h < A.H;
  const int64_t s = A.step;
  uint32_t tested = 0, accepted = 0;
  if (valid) {
    const int64_t pi = h * A.W + w;
    const float4 *gp = reinterpret_cast<const float4 *>(A.guide + pi);
    const float4 p0 = gp[0], p1 = gp[1];
    const int32_t geom_p = __float_as_int(p0.w), prim_p = __float_as_int(p1.w);
    if (!(geom_p >= 0 || prim_p >= 0)) {
#pragma unroll
      for (int c = 0; c < CH; ++c) A.out[pi * CH + c] = A.in[pi * CH + c];
    } else {
      const f3 Np = mk(p0.x, p0.y, p0.z), Pp = mk(p1.x, p1.y, p1.z);
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = 0.f;
      float ws = 0.f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qh = h + dy * s;
        if (qh < 0 || qh >= A.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const int64_t qw = w + dx * s;
          if (qw < 0 || qw >= A.W) continue;
          const int64_t qi = qh * A.W + qw;
          const float k = K1[dx + 2] * K1[dy + 2];
          if (dx != 0 || dy != 0) {
            ++tested;
            const float4 *gq = reinterpret_cast<const float4 *>(A.guide + qi);
            const float4 q0 = gq[0], q1 = gq[1];
            const int32_t geom_q = __float_as_int(q0.w), prim_q = __float_as_int(q1.w);
            if (!(geom_q >= 0 || prim_q >= 0)) continue;
            if (A.same_object && !(geom_q == geom_p && (geom_p >= 0 || prim_q == prim_p))) continue;
            if (!(dot(Np, mk(q0.x, q0.y, q0.z)) >= A.normal_cos)) continue;
            const f3 df = mk(q1.x, q1.y, q1.z) - Pp;
            if (!(fabsf(dot(df, Np)) <= A.plane_dist)) continue;
            ++accepted;
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) acc[c] = acc[c] + k * A.in[qi * CH + c];
          ws = ws + k;
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) A.out[pi * CH + c] = acc[c] / ws;
    }
  }
  // stats: wave reductions, then one ordinary global atomic per wave and counter that has something to add
  const unsigned long long nt = filter_wave_sum(tested), na = filter_wave_sum(accepted);
  if ((threadIdx.x & 63) == 0) {
    if (nt) atomicAdd(&A.stats[1], nt);
    if (na) atomicAdd(&A.stats[2], na);
  }
}

} // namespace esc

extern "C" int esc_launch_filter_pack(const esc::FilterPackParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_filter_pack, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

// tiles: tiles_x * ceil(H / kFilterTileH), checked by the caller to fit one launch
extern "C" int esc_launch_filter_atrous(const esc::FilterParams *p, int channels, int64_t tiles, hipStream_t stream) {
  if (tiles <= 0) return 0;
  if (channels == 3)
    hipLaunchKernelGGL((esc::k_filter_atrous<3>), dim3((unsigned)tiles), dim3(256), 0, stream, *p);
  else
    hipLaunchKernelGGL((esc::k_filter_atrous<1>), dim3((unsigned)tiles), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
