// rt_query.hip -- batched ray queries on rays of the caller's own: the two functions the reference's
// render loop is built from, on arbitrary (origin, direction, bound) triples.
//
//   k_query<false>  closest hit   == intersect() / cpp_intersect() (main.cpp:176-192, 302-312) with
//                                    the sphere extension after every triangle (oracle closest_hit)
//   k_query<true>   occlusion     == occlusion() (main.cpp:314-329) with the sphere extension
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide / sqrt):
// every t, u, v that reaches an output is the reference's own fp32 / f64 arithmetic on the exact
// records; the filters below only decide WHETHER that arithmetic runs for a pair.
//
// One ray per lane, 256-thread workgroups, 64-bit ray indices.  A ray takes the FILTERED sweep when
// it meets every precondition of the shadow-form filter statements (rt_brute.h), else the EXACT
// sweep (every primitive in index order, t carried, as the reference loop):
//   (a) origin and direction finite with every coordinate below 2^60 in magnitude (rt_brute.h
//       "FILTERS": the input range of every error bound there);
//   (b) the origin within rho_max of g in the 1-norm (the `far` test of make_ray_tri_filter): the
//       margins of DevTriPairF / DevTriPairPF and the group radii hold for such origins only;
//   (c) |d|^2 within 7.5u of 1 (evaluated exactly: three exact f64 products, one f64 rounding),
//       so the real |d|^2 is within 8u of 1 -- the hypothesis of the sphere-group radius
//       (rt_brute.h, "|L|^2 within 8u of 1") and the "unit to a few ulp" of the filters.  The
//       reference's normalize() leaves |d|^2 within about 7u of 1 (one rounding in each of the dot
//       product's five operations, the sqrt and the three divides), so its directions pass;
//   (d) tmax is not NaN (with a NaN bound the reference accepts the FIRST candidate in index order
//       whatever its t, which only the index-order sweep reproduces).
//
// PROOF OBLIGATION: the shadow-form statements are statements about the ray's LINE.  Each was
// re-read for a use of the segment bound tb (the shadow ray's `len - eps`):
//   - pair4_any_filter_pk (sphere filter): "not disc < 0  ==>  q' >= 0".  disc is the reference's
//     discriminant; the derivation bounds the roundings of b and cc (in |a|, |c|, r2) and never
//     mentions t.  Holds for every t.
//   - tripair2_any_filter_pk (triangle filter): from u2 >= eps, v2 >= eps, u2 + v2 <= 1 and |un|,
//     |vn| <= |det| (1 + 4u), i.e. from the barycentric rejects alone; the margin M is built from
//     |e1|, |e2|, |v0 - g| and rho_max.  No t.
//   - tripair2_any_prefilter_pk (triangle pre-filter): an accept puts the line's meeting point X*
//     with the plane within rho of the triangle, or has |det*| < tau.  X* is a point of the line,
//     found from the barycentric rejects; t2 plays no part.  No t.
//   - group records, spheres: R = rgeo + 0x1.6p-10 (rho_max + |C - g| + rgeo) bounds the LINE's
//     distance from C for every member the reference does not reject at `disc < 0` (|w_i| <=
//     rho_max (1+u) + |C - g| + rgeo by (b)).  No t.
//   - group records, triangles: (S_t) the line passes C~ within R, or (E_t) |d . a| <= kappa';
//     both follow from the pre-filter's statement per member and the static cone.  No t.
// So every filter holds for unbounded t, and the query ray takes all of them.
// The sweeps do not prune by t at all (t2 of a nearly parallel ray is off by up to a sixth,
// DESIGN.md §3.9): every group some live lane may touch is opened.
//
// Closest hit in an order other than the index order: the reference keeps the first of equal t
// (strict `t2 >= t` reject), so its result is the smallest (t2, index) pair among the pairs that
// pass every reject except the bound, with t2 < tmax.  accept_free() keeps exactly that, index =
// [0, n_tri) for triangles, n_tri + k for sphere k (rt_brute.h Hit::idx).  t2 is never NaN on this
// path: |det| >= eps, and the numerators are finite for finite records and a ray that meets (a)-(c).
// Occlusion: the answer is "some pair passes with t2 < tmax", which no order changes; the first
// accept ends the ray.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_query_sweep.h"

namespace esc {

template <bool OCC>
__global__ __launch_bounds__(256) void k_query(const QueryParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.n;
  QLane s;
  s.o = mk(0.f, 0.f, 0.f);
  s.L = mk(0.f, 0.f, 0.f);
  s.tmax = FLT_MAX;
  if (valid) {
    s.o = mk(p.orig[3 * i], p.orig[3 * i + 1], p.orig[3 * i + 2]);
    s.L = mk(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
    if (p.tmax) s.tmax = p.tmax[i];
  }
  s.t = s.tmax;
  s.u = s.v = 0.f;
  s.id = -1;
  s.occ = false;
  s.tests = 0;
  bool far;
  const RayTF rt = make_ray_tri_filter(s.o, s.L, p.g, p.rho_max, far);
  const RayF rs = make_ray_filter(s.o, s.L, p.g);
  const double dd = ((double)s.L.x * s.L.x + (double)s.L.y * s.L.y) + (double)s.L.z * s.L.z;
  const bool finite = coord_ok(s.o.x) && coord_ok(s.o.y) && coord_ok(s.o.z) && coord_ok(s.L.x) &&
                      coord_ok(s.L.y) && coord_ok(s.L.z);
  const bool unit = fabs(dd - 1.0) <= 7.5 * 0x1p-24;
  const bool elig = valid && !p.exact_only && finite && !far && unit && !(s.tmax != s.tmax);
  s.live = elig;
  if (__builtin_amdgcn_ballot_w64(elig)) {
    if (p.n_tri > 0) {
      if (p.tg.n_grp > 0) tri_groups<OCC ? kAny : kClosest>(p, rs, rt, s);
      else tri_linear<OCC ? kAny : kClosest>(p, rs, rt, s);
    }
    if (p.n_sph > 0) {
      if (p.sg.n_grp > 0) sph_groups<OCC ? kAny : kClosest>(p, rs, s);
      else sph_linear<OCC ? kAny : kClosest>(p, rs, s);
    }
  }
  const bool need = valid && !elig;
  s.live = false;
  exact_sweep<OCC ? kAny : kClosest>(p, need, s);

  if (valid) {
    if (OCC) {
      p.occ[i] = s.occ ? 1 : 0;
    } else {
      int32_t geom = -1, prim = -1;
      float u = 0.f, v = 0.f;
      if (s.id >= 0 && s.id < p.n_tri) {
        geom = p.tri[s.id].geom;
        prim = p.tri[s.id].pad[0];
        u = s.u;
        v = s.v;
      } else if (s.id >= p.n_tri) {
        prim = s.id - p.n_tri;
      }
      p.t[i] = s.t;
      p.geom[i] = geom;
      p.prim[i] = prim;
      if (p.uv) {
        p.uv[2 * i] = u;
        p.uv[2 * i + 1] = v;
      }
    }
  }
  // stats: one wave reduction, then one ordinary global atomic per wave and counter
  unsigned long long tests = s.tests;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tests += __shfl_xor(tests, off, 64);
  const unsigned long long rays = __popcll(__builtin_amdgcn_ballot_w64(valid));
  const unsigned long long exact = __popcll(__builtin_amdgcn_ballot_w64(need));
  if ((threadIdx.x & 63) == 0 && rays) {
    atomicAdd(&p.stats[0], rays);
    atomicAdd(&p.stats[1], exact);
    atomicAdd(&p.stats[2], tests);
  }
}

} // namespace esc

extern "C" int esc_launch_query(const esc::QueryParams *p, int occlusion, hipStream_t stream) {
  if (p->n <= 0) return 0;
  const dim3 grid((unsigned)((p->n + 255) / 256));
  if (occlusion)
    hipLaunchKernelGGL(esc::k_query<true>, grid, dim3(256), 0, stream, *p);
  else
    hipLaunchKernelGGL(esc::k_query<false>, grid, dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
