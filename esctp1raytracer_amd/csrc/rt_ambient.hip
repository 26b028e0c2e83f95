// rt_ambient.hip -- ambient occlusion: how much of the hemisphere above a ray's hit point is open
// (esc_ambient_rays / esc_render_ambient; the definition is in include/esctp1_rt.h at
// esc_ambient_options), the modulation of an image by that visibility (esc_modulate), and sky lighting: what
// the open samples see of the environment cube (esc_skylight_rays / esc_render_skylight / esc_add_light,
// DESIGN.md §3.19; the definition is in include/esctp1_rt.h at esc_skylight_rays).
//
//   k_ambient<false, SKY>  rays from the caller's arrays
//   k_ambient<true, SKY>   ray i is pixel i of the frame, made in-lane by camera_ray_dir (rt_camera_ray.h):
//                          the bits of k_camera_rays with no offsets
//   per ray: the closest hit (k_query's kClosest sweep, bound FLT_MAX), the normal of rt_shade_body.inc
//   (main.cpp:723-738, quirk S1; the sphere extension with the ray's own o), k_trace's bounce origin
//   P = (o + d*t) + Nf*bias, a branch-free tangent frame about Nf, the table's set chosen by mix_hi32
//   (rt_transmit.h) with light index 0xFFFFFFFE, then K sample rays (P, w_k, radius) through the any-hit
//   sweep, each an ordinary ray to the precondition gate (a)-(d) of rt_query.hip.  A wave without a hit
//   skips the sample loop.  No ray goes through memory: the K sample rays of a hit live in registers.
//   SKY: every open sample adds env(w_k) (env_lookup of rt_environ.h: four 16-byte loads) to three fp32
//   accumulators of its lane, in sample order; sky = s / K and light = kd * sky are written per ray.  Without
//   SKY none of that code exists: the two instantiations are the kernels they were.
//   k_modulate        out = fl(rgb * vis) per channel, and its PPM quantisation
//   k_add_light       out = fl(rgb + light) per channel, and its PPM quantisation
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt), and
// only + - * / and sqrt (SKY: and the lookup's floorf): no device transcendental.  The sample directions are
// data (the table), and so are the texels.
// One ray per lane, 256-thread workgroups, 64-bit ray indices.  The kernels read only per-scene tables
// and the context's sample table (SKY: and its environment cube).
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_ambient.h"
#include "rt_camera_ray.h"
#include "rt_shade_body.h"
#include "rt_transmit.h"

namespace esc {

template <bool CAMERA, bool SKY>
__global__ __launch_bounds__(256) void k_ambient(const AmbientParams A) {
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
  uint32_t n_exact; // this lane's rays (primary, sample) that took the exact sweep
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
    if (A.t) A.t[i] = s.t;
    if (A.geom) A.geom[i] = geom;
    if (A.prim) A.prim[i] = prim;
  }

  int32_t count = A.samples; // a miss: every sample is open
  uint32_t n_occ = 0;
  float sr = 0.f, sg_ = 0.f, sb = 0.f; // SKY: the sum of env(w_k) over the open samples, k ascending
  int mi = 0;                          // SKY: the hit's material
  if (__builtin_amdgcn_ballot_w64(has_hit)) {
    // ---- main.cpp:723-738 normal of the hit (rt_shade_body.inc)
    f3 N = mk(0.f, 0.f, 0.f);
    if (has_hit) {
      if (s.id < p.n_tri) {
        const DevTri Tr = p.tri[s.id];
        N = normalize(cross(ld3(Tr.e1), ld3(Tr.e2))); // :728-731
        if constexpr (SKY) mi = Tr.geom;
        if (A.mat[Tr.geom].has_normals) {             // :733-738 with u == 0 (quirk S1)
          const DevTriN Q = A.tri_n[s.id];
          const float u = 0.f, v = s.v;
          N = normalize((ld3(Q.n1) * u + ld3(Q.n2) * v) + ld3(Q.n0) * ((1.f - u) - v));
        }
      } else {
        const DevSph S = p.sph[s.id - p.n_tri];
        N = normalize((o + d * s.t) - mk(S.cx, S.cy, S.cz)); // extension
        if constexpr (SKY) mi = A.sph_mat[s.id - p.n_tri];
      }
    }
    // ---- k_trace's bounce origin
    const float sn = dot(d, N);
    const f3 Nf = (sn > 0.f) ? mk(-N.x, -N.y, -N.z) : N;
    const f3 P = (o + d * s.t) + Nf * A.bias;
    // ---- the tangent frame about Nf: |sg + Nf.z| >= 1, so there is no special case
    const float sg = copysignf(1.f, Nf.z);
    const float a = -1.f / (sg + Nf.z);
    const float b = (Nf.x * Nf.y) * a;
    const f3 T = mk(1.f + (sg * (Nf.x * Nf.x)) * a, sg * b, -(sg * Nf.x));
    const f3 B = mk(b, sg + (Nf.y * Nf.y) * a, -Nf.y);
    // ---- the set of this ray; a lane without a hit reads nothing
    const uint32_t set = mix_hi32(A.seed, A.pixel_base + (uint32_t)i, kAmbientLight) % (uint32_t)A.sets;
    const float *tab = A.table + 3 * (int64_t)A.row_samples * (int64_t)set;
    count = has_hit ? 0 : count;
    for (int k = 0; k < A.samples; ++k) {
      f3 l = mk(0.f, 0.f, 1.f);
      if (has_hit) l = ld3(tab + 3 * k);
      const f3 w = normalize((T * l.x + B * l.y) + Nf * l.z);
      QLane q;
      lane_init(q, P, w, A.radius);
      RayTF rt;
      RayF rs;
      const bool elig = filter_gate(p, has_hit, P, w, A.radius, rt, rs);
      const bool need = has_hit && !elig;
      sweep<kAny>(p, elig, need, rs, rt, q);
      const bool occluded = has_hit && q.occ;
      count += (has_hit && !occluded) ? 1 : 0;
      if constexpr (SKY) {
        if (has_hit && !occluded) {
          float er, eg, eb;
          env_lookup(A.env.texels, A.env.res, w.x, w.y, w.z, er, eg, eb);
          sr += er;
          sg_ += eg;
          sb += eb;
        }
      }
      n_occ += occluded ? 1u : 0u;
      n_exact += need ? 1u : 0u;
      tests += q.tests;
    }
  }
  if (valid) {
    if (!SKY || A.vis) A.vis[i] = (float)count / (float)A.samples; // SKY: vis is optional
    if (A.count) A.count[i] = count;
    if constexpr (SKY) {
      // a miss: the sums are +0 and so are sky and light
      const float kf = (float)A.samples;
      const float yr = sr / kf, yg = sg_ / kf, yb = sb / kf;
      if (A.sky) {
        A.sky[3 * i] = yr;
        A.sky[3 * i + 1] = yg;
        A.sky[3 * i + 2] = yb;
      }
      if (A.light) {
        f3 kd = mk(0.f, 0.f, 0.f);
        if (has_hit) kd = ld3(A.mat[mi].kd);
        A.light[3 * i] = has_hit ? kd.x * yr : 0.f;
        A.light[3 * i + 1] = has_hit ? kd.y * yg : 0.f;
        A.light[3 * i + 2] = has_hit ? kd.z * yb : 0.f;
      }
    }
  }

  // stats: wave reductions, then one ordinary global atomic per wave and counter that has something to
  // add (rt_trace.hip says what same-address atomics cost on light scenes)
  if (A.stats) {
    const unsigned long long rays = __popcll(__builtin_amdgcn_ballot_w64(valid));
    const unsigned long long hits = __popcll(__builtin_amdgcn_ballot_w64(has_hit));
    const unsigned long long occ = wave_sum64(n_occ);
    const unsigned long long exact = wave_sum64(n_exact);
    tests = wave_sum64(tests);
    if ((threadIdx.x & 63) == 0 && rays) {
      atomicAdd(&A.stats[0], rays);
      if (hits) atomicAdd(&A.stats[1], hits);
      if (occ) atomicAdd(&A.stats[2], occ);
      if (exact) atomicAdd(&A.stats[3], exact);
      if (tests) atomicAdd(&A.stats[4], tests);
    }
  }
}

// out = fl(rgb * vis) per channel; u8 = quantise(out) (main.cpp:676-682)
__global__ __launch_bounds__(256) void k_modulate(const ModulateParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const float v = p.vis[i];
  const float r = p.rgb[3 * i] * v, g = p.rgb[3 * i + 1] * v, b = p.rgb[3 * i + 2] * v;
  if (p.out) {
    p.out[3 * i] = r;
    p.out[3 * i + 1] = g;
    p.out[3 * i + 2] = b;
  }
  if (p.out8) {
    p.out8[3 * i] = quantise_channel(r);
    p.out8[3 * i + 1] = quantise_channel(g);
    p.out8[3 * i + 2] = quantise_channel(b);
  }
}

// out = fl(rgb + light) per channel; u8 = quantise(out) (main.cpp:676-682)
__global__ __launch_bounds__(256) void k_add_light(const AddLightParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const float r = p.rgb[3 * i] + p.light[3 * i], g = p.rgb[3 * i + 1] + p.light[3 * i + 1],
              b = p.rgb[3 * i + 2] + p.light[3 * i + 2];
  if (p.out) {
    p.out[3 * i] = r;
    p.out[3 * i + 1] = g;
    p.out[3 * i + 2] = b;
  }
  if (p.out8) {
    p.out8[3 * i] = quantise_channel(r);
    p.out8[3 * i + 1] = quantise_channel(g);
    p.out8[3 * i + 2] = quantise_channel(b);
  }
}

} // namespace esc

static dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" int esc_launch_ambient(const esc::AmbientParams *p, int camera, int sky, hipStream_t stream) {
  if (p->q.n <= 0) return 0;
  if (sky && camera)
    hipLaunchKernelGGL((esc::k_ambient<true, true>), grid_of(p->q.n), dim3(256), 0, stream, *p);
  else if (sky)
    hipLaunchKernelGGL((esc::k_ambient<false, true>), grid_of(p->q.n), dim3(256), 0, stream, *p);
  else if (camera)
    hipLaunchKernelGGL((esc::k_ambient<true, false>), grid_of(p->q.n), dim3(256), 0, stream, *p);
  else
    hipLaunchKernelGGL((esc::k_ambient<false, false>), grid_of(p->q.n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_add_light(const esc::AddLightParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_add_light, grid_of(p->n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}

extern "C" int esc_launch_modulate(const esc::ModulateParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_modulate, grid_of(p->n), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
