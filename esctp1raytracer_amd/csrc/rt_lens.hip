// rt_lens.hip -- the frame's primary rays through a thin lens, as data (esc_lens_rays / esc_render_lens,
// DESIGN.md §3.22; the definition is in include/esctp1_rt.h at esc_lens_options).
//
//   k_lens_rays   ray i is pixel pix0 + i of the frame with a sub-pixel offset, as in k_camera_rays, and lens
//                 sample k of the pixel's set of the context's lens table (points of the unit disk, data):
//                     p  = ((llc + horizontal*s) + vertical*t) - origin          (camera_ray_point)
//                     o' = origin + off,  off = U*(l.x*aperture) + V*(l.y*aperture)
//                     d' = normalize(p*focus_dist - off)
//                 The set is mix_hi32(seed, pixel, kLensLight) mod S and does not depend on k.  With aperture == 0
//                 (wave-uniform: it is a parameter) the ray is k_camera_rays', by the same statements
//                 (rt_camera_ray.h), and the table is not read.
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt), and only
// + - * / and sqrt.  One ray per lane, 256-thread workgroups, 64-bit ray indices; no LDS, no atomics.  The
// table (at most 32 KB) is read through the vector path: two floats per lane at the lane's set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_camera_ray.h"
#include "rt_lens.h"
#include "rt_transmit.h"

namespace esc {

__global__ __launch_bounds__(256) void k_lens_rays(const LensRayParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const int64_t pix = p.pix0 + i;
  const int h = (int)(pix / p.W), w = (int)(pix % p.W);
  const float dx = p.offsets ? p.offsets[2 * i] : p.dx;
  const float dy = p.offsets ? p.offsets[2 * i + 1] : p.dy;
  const f3 origin = mk(p.origin[0], p.origin[1], p.origin[2]);
  f3 o = origin, d;
  if (p.aperture == 0.f) {
    d = camera_ray_dir(origin, p.llc, p.horizontal, p.vertical, p.W, p.H, w, h, dx, dy);
  } else {
    const f3 pt = camera_ray_point(origin, p.llc, p.horizontal, p.vertical, p.W, p.H, w, h, dx, dy);
    const uint32_t set = mix_hi32(p.seed, (uint32_t)pix, kLensLight) % (uint32_t)p.sets;
    const float *l = p.table + 2 * ((int64_t)set * p.samples + p.sample);
    const float lx = l[0], ly = l[1];
    const f3 off = ld3(p.U) * (lx * p.aperture) + ld3(p.V) * (ly * p.aperture);
    o = origin + off;
    d = normalize(pt * p.focus_dist - off);
  }
  p.orig[3 * i] = o.x;
  p.orig[3 * i + 1] = o.y;
  p.orig[3 * i + 2] = o.z;
  p.dir[3 * i] = d.x;
  p.dir[3 * i + 1] = d.y;
  p.dir[3 * i + 2] = d.z;
}

} // namespace esc

extern "C" int esc_launch_lens_rays(const esc::LensRayParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_lens_rays, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
