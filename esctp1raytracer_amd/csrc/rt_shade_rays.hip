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

__global__ __launch_bounds__(256) void k_shade_rays(const ShadeParams P) {
  const QueryParams &p = P.q;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.n;
  f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
  if (valid) {
    o = mk(p.orig[3 * i], p.orig[3 * i + 1], p.orig[3 * i + 2]);
    d = mk(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
  }

  // ---- main.cpp:715-722 closest hit, t from FLT_MAX
  QLane s;
  lane_init(s, o, d, FLT_MAX);
  uint32_t n_exact; // this lane's rays (primary, shadow) that took the exact sweep
  {
    RayTF rt;
    RayF rs;
    const bool elig = filter_gate(p, valid, o, d, FLT_MAX, rt, rs);
    const bool need = valid && !elig;
    sweep<kClosest>(p, elig, need, rs, rt, s);
    n_exact = need ? 1u : 0u;
  }
  unsigned long long tests = s.tests;
  const bool has_hit = valid && s.id >= 0;
  if (valid) {
    int32_t geom = -1, prim = -1;
    if (s.id >= 0 && s.id < p.n_tri) {
      geom = p.tri[s.id].geom;
      prim = p.tri[s.id].pad[0];
    } else if (s.id >= p.n_tri) {
      prim = s.id - p.n_tri;
    }
    if (P.t) P.t[i] = s.t;
    if (P.geom) P.geom[i] = geom;
    if (P.prim) P.prim[i] = prim;
  }

  // ---- main.cpp:723-738 normal of the hit
  f3 N = mk(0.f, 0.f, 0.f);
  int mi = 0;
  if (has_hit) {
    if (s.id < p.n_tri) {
      const DevTri Tr = p.tri[s.id];
      N = normalize(cross(ld3(Tr.e1), ld3(Tr.e2))); // :728-731
      mi = Tr.geom;
      if (P.mat[mi].has_normals) { // :733-738 with u == 0 (quirk S1)
        const DevTriN Q = P.tri_n[s.id];
        const float u = 0.f, v = s.v;
        N = normalize((ld3(Q.n1) * u + ld3(Q.n2) * v) + ld3(Q.n0) * ((1.f - u) - v));
      }
    } else {
      const int k = s.id - p.n_tri;
      const DevSph S = p.sph[k];
      N = normalize((o + d * s.t) - mk(S.cx, S.cy, S.cz)); // extension
      mi = P.sph_mat[k];
    }
  }

  // ---- main.cpp:740-789 per-light shading
  float t = s.t;
  float r = 0.f, g = 0.f, b = 0.f; // vec3 default ctor, main.cpp:557-558
  const float nl = (float)P.n_lights;
  uint32_t n_shadow = 0;
  for (int li = 0; li < P.n_lights; ++li) {
    const DevLight Lt = P.lights[li];
    f3 ro = mk(0.f, 0.f, 0.f), rL = mk(0.f, 0.f, 0.f);
    if (has_hit) {
      // x % 1 == 0: a one-face light needs no draw
      const uint32_t face = (P.face_mode == 0) ? (uint32_t)P.fixed_face
                            : (Lt.n_faces == 1) ? 0u
                                                : face_hash(P.seed, P.pixel_base + (uint32_t)i, (uint32_t)li,
                                                            (uint32_t)Lt.n_faces);
      const f3 Pt = ld3(P.light_points + 4 * (Lt.first_point + (int)face)); // quirk S2
      ro = o + d * (t - FLT_EPSILON); // :757-758
      rL = Pt - ro;                   // :759
      const float len = length(rL);   // :761
      t = len - FLT_EPSILON;          // :764
      rL = normalize(rL);             // :766
    }
    bool occluded = false;
    if (P.shadows) { // :772 occlusion(hit, L, t)
      QLane a;
      lane_init(a, ro, rL, t);
      RayTF rt;
      RayF rs;
      const bool elig = filter_gate(p, has_hit, ro, rL, t, rt, rs);
      const bool need = has_hit && !elig;
      if (li + 1 < P.n_lights)
        sweep<kFirst>(p, elig, need, rs, rt, a);
      else
        sweep<kAny>(p, elig, need, rs, rt, a);
      occluded = has_hit && a.occ;
      if (occluded) t = a.t; // occlusion() wrote the occluder's t2 through its reference (quirk S3)
      n_shadow += has_hit ? 1u : 0u;
      n_exact += need ? 1u : 0u;
      tests += a.tests;
    }
    if (has_hit && !occluded) phong_add(P.mat[mi], N, rL, nl, r, g, b); // :768-788
  }

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
  const float is = ((float)w + dx) / (float)(p.W - 1);
  const float it = ((float)h + dy) / (float)(p.H - 1);
  const f3 dir = normalize(((ld3(p.llc) + ld3(p.horizontal) * is) + ld3(p.vertical) * it) - origin);
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
