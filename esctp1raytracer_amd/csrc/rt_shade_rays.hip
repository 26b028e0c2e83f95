// rt_shade_rays.hip -- scan_row's body (main.cpp:698-791) on rays of the caller's own, the camera's
// primary rays as data, and the small steps of supersampled rendering.
//
//   k_camera_rays  camera.h:31-34 get_ray at s = (w + dx) / (W - 1), t = (h + dy) / (H - 1): with
//                  dx = dy = 0 these are primary_dir's (rt_kernels.hip) operations, bit for bit
//   k_shade_rays   per ray (o, d): closest hit (k_query's kClosest sweep), the normal
//                  (main.cpp:723-738, quirk S1; the sphere extension with the ray's own o), then per
//                  light: the light sample (quirk S2), the shadow ray (main.cpp:757-766), occlusion()
//                  with the carried t (quirk S3) and Phong (main.cpp:768-788)
//   k_ss_accumulate / k_ss_finish   acc += rgb_k; image = acc / spp; u8 = quantise(image)
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt).
// Every shadow ray (hit, L, t) goes through the precondition gate (a)-(d) of rt_query.hip like a
// query ray: one that fails it runs the reference loop in index order.  The lights before the last
// need the occluder of the lowest original index (its t2 moves the next light's hit point) and take
// the kFirst sweep (rt_query_sweep.h); the last light's occluder is never read again, so any
// occluder ends that ray (kAny).  DESIGN.md §3.12.
//
// One ray per lane, 256-thread workgroups, 64-bit ray indices.  The kernel reads only per-scene
// tables: no camera state, tile or light lists, render counters or recorded frame.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_camera_ray.h"
#include "rt_shade_body.h"

namespace esc {

__global__ __launch_bounds__(256) void k_shade_rays(const ShadeParams P) {
  const QueryParams &p = P.q;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.n;
  f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
  if (valid) {
    o = mk(p.orig[3 * i], p.orig[3 * i + 1], p.orig[3 * i + 2]);
    d = mk(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
  }

#define SHADE_BODY_SEED P.seed
#define SHADE_BODY_PIXEL (P.pixel_base + (uint32_t)i)
#define SHADE_BODY_HIT_OUTPUTS
#include "rt_shade_body.inc"
#undef SHADE_BODY_HIT_OUTPUTS
#undef SHADE_BODY_PIXEL
#undef SHADE_BODY_SEED

  if (valid) {
    P.rgb[3 * i] = r;
    P.rgb[3 * i + 1] = g;
    P.rgb[3 * i + 2] = b;
    if (P.rgb8) {
      P.rgb8[3 * i] = quantise_channel(r);
      P.rgb8[3 * i + 1] = quantise_channel(g);
      P.rgb8[3 * i + 2] = quantise_channel(b);
    }
  }
  // stats: wave reductions, then one ordinary global atomic per wave and counter
  const unsigned long long rays = __popcll(__builtin_amdgcn_ballot_w64(valid));
  const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(has_hit));
  const unsigned long long shadow = wave_sum64(n_shadow);
  const unsigned long long exact = wave_sum64(n_exact);
  tests = wave_sum64(tests);
  if ((threadIdx.x & 63) == 0 && rays) {
    atomicAdd(&P.stats[0], rays);
    atomicAdd(&P.stats[1], hits);
    atomicAdd(&P.stats[2], shadow);
    atomicAdd(&P.stats[3], exact);
    atomicAdd(&P.stats[4], tests);
  }
}

// camera.h:31-34 with the sub-pixel offset added before the divide (see the header)
__global__ __launch_bounds__(256) void k_camera_rays(const CameraRayParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const int64_t pix = p.pix0 + i;
  const int h = (int)(pix / p.W), w = (int)(pix % p.W);
  const float dx = p.offsets ? p.offsets[2 * i] : p.dx;
  const float dy = p.offsets ? p.offsets[2 * i + 1] : p.dy;
  const f3 origin = mk(p.origin[0], p.origin[1], p.origin[2]);
  const f3 dir = camera_ray_dir(origin, p.llc, p.horizontal, p.vertical, p.W, p.H, w, h, dx, dy);
  p.orig[3 * i] = origin.x;
  p.orig[3 * i + 1] = origin.y;
  p.orig[3 * i + 2] = origin.z;
  p.dir[3 * i] = dir.x;
  p.dir[3 * i + 1] = dir.y;
  p.dir[3 * i + 2] = dir.z;
}

// acc = 0; acc += rgb_k, per value (first: the 0 is the accumulator's start)
__global__ __launch_bounds__(256) void k_ss_accumulate(float *acc, const float *rgb, int64_t n, int first) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  acc[i] = (first ? 0.f : acc[i]) + rgb[i];
}

// image = acc / spp; u8 = quantise(image) (main.cpp:676-682)
__global__ __launch_bounds__(256) void k_ss_finish(float *img, uint8_t *u8, int64_t n, float spp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = img[i] / spp;
  img[i] = v;
  if (u8) u8[i] = quantise_channel(v);
}

} // namespace esc

static dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" int esc_launch_shade_rays(const esc::ShadeParams *p, hipStream_t stream) {
  if (p->q.n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_shade_rays, grid_of(p->q.n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_camera_rays(const esc::CameraRayParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_camera_rays, grid_of(p->n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_ss_accumulate(float *acc, const float *rgb, int64_t n, int first, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_ss_accumulate, grid_of(n), dim3(256), 0, stream, acc, rgb, n, first);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_ss_finish(float *img, uint8_t *u8, int64_t n, float spp, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_ss_finish, grid_of(n), dim3(256), 0, stream, img, u8, n, spp);
  return (int)hipGetLastError();
}
