// rt_gbuffer.hip -- the G-buffer of rays and frames: per ray the shading normal, the hit position, the hit
// material's kd and what esc_intersect_rays gives (esc_gbuffer_rays / esc_render_gbuffer, DESIGN.md §3.20;
// the definition is in include/esctp1_rt.h at esc_gbuffer_rays).  These are the guides of the edge-stopping
// filter of rt_filter.hip.
//
//   k_gbuffer<false>  rays from the caller's arrays
//   k_gbuffer<true>   ray i is pixel i of the frame, made in-lane by camera_ray_dir (rt_camera_ray.h): the
//                     bits of k_camera_rays with no offsets
//   per ray: the first half of k_ambient (rt_ambient.hip) -- the closest hit (k_query's kClosest sweep, bound
//   FLT_MAX), the normal of rt_shade_body.inc (main.cpp:723-738, quirk S1; the sphere extension with the
//   ray's own o), NOT flipped towards the ray -- then position = o + d*t and the material's kd.  A miss
//   writes +0 to all three, t = FLT_MAX and geom = prim = -1.
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt), and only
// + - * / and sqrt.  One ray per lane, 256-thread workgroups, 64-bit ray indices.  The kernels read only
// per-scene tables.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_camera_ray.h"
#include "rt_gbuffer.h"
#include "rt_shade_body.h"

namespace esc {

template <bool CAMERA>
__global__ __launch_bounds__(256) void k_gbuffer(const GBufferParams A) {
  const QueryParams &p = A.q;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.n;
  f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
  if (valid) {
    if (CAMERA) {
      const int h = (int)(i / A.W), w = (int)(i % A.W);
      o = mk(A.origin[0], A.origin[1], A.origin[2]);
      d = camera_ray_dir(o, A.llc, A.horizontal, A.vertical, A.W, A.H, w, h, 0.f, 0.f);
    } else {
      o = mk(p.orig[3 * i], p.orig[3 * i + 1], p.orig[3 * i + 2]);
      d = mk(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
    }
  }

  // ---- main.cpp:715-722 closest hit, t from FLT_MAX (rt_shade_body.inc)
  QLane s;
  lane_init(s, o, d, FLT_MAX);
  RayTF rt;
  RayF rs;
  const bool elig = filter_gate(p, valid, o, d, FLT_MAX, rt, rs);
  const bool need = valid && !elig;
  sweep<kClosest>(p, elig, need, rs, rt, s);
  const bool has_hit = valid && s.id >= 0;
  if (valid) {
    int32_t geom = -1, prim = -1;
    if (s.id >= 0 && s.id < p.n_tri) {
      geom = p.tri[s.id].geom;
      prim = p.tri[s.id].pad[0];
    } else if (s.id >= p.n_tri) {
      prim = s.id - p.n_tri;
    }
    if (A.t) A.t[i] = s.t;
    if (A.geom) A.geom[i] = geom;
    if (A.prim) A.prim[i] = prim;
  }

  // ---- main.cpp:723-738 normal of the hit (rt_shade_body.inc), the position and the material
  f3 N = mk(0.f, 0.f, 0.f), P = mk(0.f, 0.f, 0.f), kd = mk(0.f, 0.f, 0.f);
  if (has_hit) {
    int mi;
    if (s.id < p.n_tri) {
      const DevTri Tr = p.tri[s.id];
      N = normalize(cross(ld3(Tr.e1), ld3(Tr.e2))); // :728-731
      mi = Tr.geom;
      if (A.mat[Tr.geom].has_normals) {             // :733-738 with u == 0 (quirk S1)
        const DevTriN Q = A.tri_n[s.id];
        const float u = 0.f, v = s.v;
        N = normalize((ld3(Q.n1) * u + ld3(Q.n2) * v) + ld3(Q.n0) * ((1.f - u) - v));
      }
    } else {
      const DevSph S = p.sph[s.id - p.n_tri];
      N = normalize((o + d * s.t) - mk(S.cx, S.cy, S.cz)); // extension
      mi = A.sph_mat[s.id - p.n_tri];
    }
    P = o + d * s.t;
    kd = ld3(A.mat[mi].kd);
  }
  if (valid) {
    if (A.normal) {
      A.normal[3 * i] = N.x;
      A.normal[3 * i + 1] = N.y;
      A.normal[3 * i + 2] = N.z;
    }
    if (A.position) {
      A.position[3 * i] = P.x;
      A.position[3 * i + 1] = P.y;
      A.position[3 * i + 2] = P.z;
    }
    if (A.albedo) {
      A.albedo[3 * i] = kd.x;
      A.albedo[3 * i + 1] = kd.y;
      A.albedo[3 * i + 2] = kd.z;
    }
  }

  // stats: wave reductions, then one ordinary global atomic per wave and counter that has something to add
  if (A.stats) {
    const unsigned long long rays = __popcll(__builtin_amdgcn_ballot_w64(valid));
    const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(has_hit));
    const unsigned long long exact = __popcll(__builtin_amdgcn_ballot_w64(need));
    const unsigned long long tests = wave_sum64(s.tests);
    if ((threadIdx.x & 63) == 0 && rays) {
      atomicAdd(&A.stats[0], rays);
      if (hits) atomicAdd(&A.stats[1], hits);
      if (exact) atomicAdd(&A.stats[2], exact);
      if (tests) atomicAdd(&A.stats[3], tests);
    }
  }
}

} // namespace esc

extern "C" int esc_launch_gbuffer(const esc::GBufferParams *p, int camera, hipStream_t stream) {
  if (p->q.n <= 0) return 0;
  const dim3 grid((unsigned)((p->q.n + 255) / 256));
  if (camera) hipLaunchKernelGGL((esc::k_gbuffer<true>), grid, dim3(256), 0, stream, *p);
  else hipLaunchKernelGGL((esc::k_gbuffer<false>), grid, dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
