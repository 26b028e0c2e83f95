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

#include "rt_device.h"
#include "rt_math.h"
#include "rt_brute.h"
#include "rt_query.h"

namespace esc {
namespace {

struct QLane {
  f3 o, L;
  float tmax;
  float t, u, v;   // closest hit so far; t starts at tmax (main.cpp:715)
  int32_t id;      // -1 none; [0, n_tri) triangle; n_tri + k sphere k
  bool live;       // on the filtered sweep and still looking
  bool occ;
  uint32_t tests;  // (ray, primitive) pairs that ran the reference arithmetic
};

DEVINL int ld_orig(const int32_t *orig, int k) { // wave-uniform: a scalar load
  typedef const int32_t __attribute__((address_space(4))) *ConstI;
  return ((ConstI)(uintptr_t)orig)[k];
}

// ray_triangle.h:14-46, every reject but the bound (main.cpp order of operations)
DEVINL bool ref_tri(const DevTri &T, f3 o, f3 L, float &t2, float &u2, float &v2) {
  const f3 e1 = ld3(T.e1), e2 = ld3(T.e2);
  const f3 pv = cross(L, e2);        // :18
  const float det = dot(e1, pv);     // :21
  const f3 tv = o - ld3(T.v0);       // :29
  const float un = dot(tv, pv);      // :32
  const f3 qv = cross(tv, e1);       // :37
  const float vn = dot(L, qv);       // :40
  const float tn = dot(e2, qv);      // :45
  return tri_exact_nb_uv(det, un, vn, tn, t2, u2, v2);
}
// the sphere extension (oracle orc_intersect_sphere), every reject but the bound
DEVINL bool ref_sph(const DevSph &S, f3 o, f3 L, float &t2) {
  const f3 oc = o - mk(S.cx, S.cy, S.cz);
  const float b = dot(oc, L);
  const float disc = b * b - (dot(oc, oc) - S.r2);
  return sph_exact_nb(b, disc, t2);
}

// an accepted pair of the filtered sweep (any order): see the header
template <bool OCC>
DEVINL void accept_free(QLane &s, int id, float t2, float u2, float v2) {
  if (OCC) {
    if (t2 < s.tmax) {
      s.occ = true;
      s.live = false;
    }
  } else if (t2 < s.t || (t2 == s.t && s.id >= 0 && id < s.id)) {
    s.t = t2;
    s.u = u2;
    s.v = v2;
    s.id = id;
  }
}

// 4 triangles = 2 pair records: pre-filter, then (if any live lane passes it) the filter, then the
// reference arithmetic for each lane whose own flags pass.  ex / orig: the 4 exact records and their
// original indices (orig == nullptr: id0 + i).
template <bool OCC>
DEVINL void tri4(const TriPairPF (&P)[2], const DevTriPairF *f, const DevTri *ex, const int32_t *orig,
                 int id0, const RayF &rs, const RayTF &rt, QLane &s) {
  v2f q[2], g[2];
  tripair2_any_prefilter_pk(P, rs, q, g);
  bool pre[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    pre[2 * j] = __float_as_int(q[j].x) >= 0 || fabsf(g[j].x) <= 1.f;
    pre[2 * j + 1] = __float_as_int(q[j].y) >= 0 || fabsf(g[j].y) <= 1.f;
  }
  if (!ANY_LANE_RARE(s.live && (pre[0] || pre[1] || pre[2] || pre[3]))) return;
  const SmemFetch<TriPairF> recf{reinterpret_cast<const TriPairF *>(f)};
  const TriPairF F[2] = {recf(0), recf(1)};
  v2f A[2], B[2], C[2];
  tripair2_any_filter_pk(F, rt, A, B, C);
  bool cand[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    cand[2 * j] = s.live && pre[2 * j] &&
                  (__float_as_int(A[j].x) | __float_as_int(B[j].x) | __float_as_int(C[j].x)) >= 0;
    cand[2 * j + 1] = s.live && pre[2 * j + 1] &&
                      (__float_as_int(A[j].y) | __float_as_int(B[j].y) | __float_as_int(C[j].y)) >= 0;
  }
  const SmemFetch<DevTri> rece{ex};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!__builtin_amdgcn_ballot_w64(cand[i])) continue;
    const DevTri T = rece(i);
    const int id = orig ? ld_orig(orig, i) : id0 + i;
    if (cand[i] && s.live) {
      ++s.tests;
      float t2, u2, v2;
      if (ref_tri(T, s.o, s.L, t2, u2, v2)) accept_free<OCC>(s, id, t2, u2, v2);
    }
  }
}

// 8 spheres = 4 pair records: the filter, then the reference arithmetic per candidate lane
template <bool OCC>
DEVINL void sph8(const DevSphPairF *f, const DevSph *ex, const int32_t *orig, int id0, const RayF &rf,
                 QLane &s) {
  const SmemFetch<PairF> recf{reinterpret_cast<const PairF *>(f)};
  PairF F[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) F[i] = recf(i);
  v2f q[4];
  pair4_any_filter_pk(F, rf, q);
  bool cand[8];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cand[2 * j] = s.live && __float_as_int(q[j].x) >= 0;
    cand[2 * j + 1] = s.live && __float_as_int(q[j].y) >= 0;
    any |= cand[2 * j] || cand[2 * j + 1];
  }
  if (!ANY_LANE_RARE(any)) return;
  const SmemFetch<DevSph> rece{ex};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!__builtin_amdgcn_ballot_w64(cand[i])) continue;
    const DevSph S = rece(i);
    const int id = orig ? id0 + ld_orig(orig, i) : id0 + i;
    if (cand[i] && s.live) {
      ++s.tests;
      float t2;
      if (ref_sph(S, s.o, s.L, t2)) accept_free<OCC>(s, id, t2, 0.f, 0.f);
    }
  }
}

// the reference arithmetic on triangles [k0, k1) / spheres [k0, k1) for the live lanes (short tails)
template <bool OCC>
DEVINL void tri_tail(const QueryParams &p, int k0, int k1, QLane &s) {
  const SmemFetch<DevTri> rec{p.tri};
  for (int k = k0; k < k1; ++k) {
    const DevTri T = rec(k);
    if (s.live) {
      ++s.tests;
      float t2, u2, v2;
      if (ref_tri(T, s.o, s.L, t2, u2, v2)) accept_free<OCC>(s, k, t2, u2, v2);
    }
  }
}
template <bool OCC>
DEVINL void sph_tail(const QueryParams &p, int k0, int k1, QLane &s) {
  const SmemFetch<DevSph> rec{p.sph};
  for (int k = k0; k < k1; ++k) {
    const DevSph S = rec(k);
    if (s.live) {
      ++s.tests;
      float t2;
      if (ref_sph(S, s.o, s.L, t2)) accept_free<OCC>(s, p.n_tri + k, t2, 0.f, 0.f);
    }
  }
}

// ---- triangles: linear sweep over the index-order pair tables (no groups: small scenes) ----------
template <bool OCC>
DEVINL void tri_linear(const QueryParams &p, const RayF &rs, const RayTF &rt, QLane &s) {
  const SmemFetch<TriPairPF> recp{reinterpret_cast<const TriPairPF *>(p.tri2_pf)};
  const int n4 = p.n_tri & ~3;
  for (int k = 0; k < n4; k += 4) {
    if (OCC && !__builtin_amdgcn_ballot_w64(s.live)) return;
    const TriPairPF P[2] = {recp(k >> 1), recp((k >> 1) + 1)};
    tri4<OCC>(P, p.tri2_f + (k >> 1), p.tri + k, nullptr, k, rs, rt, s);
  }
  tri_tail<OCC>(p, n4, p.n_tri, s); // < 4 left: straight to the reference arithmetic
}

// ---- triangles: the three group levels of rt_brute.h anyhit_tri_groups_filter, every opened group
// visited (the "lights before the last" mode), closest-hit accumulator ---------------------------
template <bool OCC>
DEVINL void tri_groups(const QueryParams &p, const RayF &rs, const RayTF &rt, QLane &s) {
  const TriGroups &G = p.tg;
  const TriPairPF *g2 = reinterpret_cast<const TriPairPF *>(G.grp2_pf);
  const SmemFetch<TriPairPF> recg{g2}, recu{g2 + (G.n_grp >> 1)},
      recy{g2 + ((G.n_grp + G.n_sup) >> 1)};
  const SmemFetch<TriPairPF> recp{reinterpret_cast<const TriPairPF *>(G.sorted2_pf)};
  const int32_t *orig = reinterpret_cast<const int32_t *>(G.orig);
  // 2 pair records = 4 bounding spheres + cones: the ones some live lane may touch
  auto open_mask = [&](const TriPairPF(&R)[2]) -> uint32_t {
    v2f q[2], g[2];
    tripair2_any_prefilter_pk(R, rs, q, g);
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool c0 = s.live && (__float_as_int(q[j].x) >= 0 || fabsf(g[j].x) <= 1.f);
      const bool c1 = s.live && (__float_as_int(q[j].y) >= 0 || fabsf(g[j].y) <= 1.f);
      if (__builtin_amdgcn_ballot_w64(c0)) mask |= 1u << (2 * j);
      if (__builtin_amdgcn_ballot_w64(c1)) mask |= 2u << (2 * j);
    }
    return mask;
  };
  auto members = [&](int gi) { // sorted triangles [8 gi, 8 gi + 8) = pair records [4 gi, 4 gi + 4)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 4 * gi + 2 * h;
      const TriPairPF P[2] = {recp(r), recp(r + 1)};
      tri4<OCC>(P, G.sorted2_f + r, G.sorted + 8 * gi + 4 * h, orig + 8 * gi + 4 * h, 0, rs, rt, s);
    }
  };
  auto groups = [&](int su) {
    for (int q4 = 0; q4 < kTriSuper; q4 += 4) {
      const int r = (kTriSuper * su + q4) >> 1;
      const TriPairPF R[2] = {recg(r), recg(r + 1)};
      uint32_t mask = open_mask(R);
      while (mask) {
        const int j = __builtin_ctz(mask);
        mask &= mask - 1;
        members(kTriSuper * su + q4 + j);
      }
    }
  };
  auto supers = [&](int y) {
    for (int q4 = 0; q4 < kTriHyper; q4 += 4) {
      const int r = (kTriHyper * y + q4) >> 1;
      const TriPairPF R[2] = {recu(r), recu(r + 1)};
      uint32_t mask = open_mask(R);
      while (mask) {
        const int j = __builtin_ctz(mask);
        mask &= mask - 1;
        groups(kTriHyper * y + q4 + j);
      }
    }
  };
  for (int y = 0; y < G.n_hyp; y += 4) { // n_hyp is a multiple of kTriGroupStep = 4
    if (OCC && !__builtin_amdgcn_ballot_w64(s.live)) return;
    const TriPairPF R[2] = {recy(y >> 1), recy((y >> 1) + 1)};
    uint32_t mask = open_mask(R);
    while (mask) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1;
      supers(y + j);
    }
  }
}

// ---- spheres: linear sweep over the index-order pair tables ----------------------------------
template <bool OCC>
DEVINL void sph_linear(const QueryParams &p, const RayF &rf, QLane &s) {
  const int n_rec = (p.n_sph + 1) >> 1;
  const int r4 = n_rec & ~3;
  for (int r = 0; r < r4; r += 4) {
    if (OCC && !__builtin_amdgcn_ballot_w64(s.live)) return;
    sph8<OCC>(p.sph2_f + r, p.sph + 2 * r, nullptr, p.n_tri + 2 * r, rf, s);
  }
  sph_tail<OCC>(p, 2 * r4, p.n_sph, s);
}

// ---- spheres: the three group levels of rt_brute.h anyhit_sph_groups_filter ------------------
template <bool OCC>
DEVINL void sph_groups(const QueryParams &p, const RayF &rf, QLane &s) {
  const SphGroups &G = p.sg;
  const PairF *g2 = reinterpret_cast<const PairF *>(G.grp2_f);
  const SmemFetch<PairF> recg{g2}, recu{g2 + (G.n_grp >> 1)}, recy{g2 + ((G.n_grp + G.n_sup) >> 1)};
  const int32_t *orig = reinterpret_cast<const int32_t *>(G.orig);
  // 4 pair records = 8 bounding spheres: the ones some live lane may touch
  auto open_mask = [&](const SmemFetch<PairF> &rec, int r0) -> uint32_t {
    PairF R[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) R[i] = rec(r0 + i);
    v2f q[4];
    pair4_any_filter_pk(R, rf, q);
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (__builtin_amdgcn_ballot_w64(s.live && __float_as_int(q[j].x) >= 0)) mask |= 1u << (2 * j);
      if (__builtin_amdgcn_ballot_w64(s.live && __float_as_int(q[j].y) >= 0)) mask |= 2u << (2 * j);
    }
    return mask;
  };
  auto members = [&](int gi) {
    sph8<OCC>(G.sorted2_f + 4 * gi, G.sorted + 8 * gi, orig + 8 * gi, p.n_tri, rf, s);
  };
  auto groups = [&](int su) {
    uint32_t mask = open_mask(recg, 4 * su);
    while (mask) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1;
      members(8 * su + j);
    }
  };
  auto supers = [&](int y) {
    uint32_t mask = open_mask(recu, 4 * y);
    while (mask) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1;
      groups(8 * y + j);
    }
  };
  for (int y0 = 0; y0 < G.n_hyp; y0 += 8) { // n_hyp is a multiple of kSphGroupStep = 8
    if (OCC && !__builtin_amdgcn_ballot_w64(s.live)) return;
    uint32_t mask = open_mask(recy, y0 >> 1);
    while (mask) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1;
      supers(y0 + j);
    }
  }
}

// ---- the exact sweep: the reference loop itself for the lanes in `need` ----------------------
template <bool OCC>
DEVINL void exact_sweep(const QueryParams &p, bool need, QLane &s) {
  if (!__builtin_amdgcn_ballot_w64(need)) return;
  const SmemFetch<DevTri> rt{p.tri};
  for (int k = 0; k < p.n_tri; ++k) {
    if (OCC && (k & 31) == 0 && !__builtin_amdgcn_ballot_w64(need && !s.occ)) return;
    const DevTri T = rt(k);
    if (need && !(OCC && s.occ)) {
      ++s.tests;
      float t2, u2, v2;
      if (ref_tri(T, s.o, s.L, t2, u2, v2) && !(t2 >= s.t)) { // ray_triangle.h:49-54
        if (OCC) {
          s.occ = true;
        } else {
          s.t = t2;
          s.u = u2;
          s.v = v2;
          s.id = k;
        }
      }
    }
  }
  const SmemFetch<DevSph> rs{p.sph};
  for (int k = 0; k < p.n_sph; ++k) {
    if (OCC && (k & 31) == 0 && !__builtin_amdgcn_ballot_w64(need && !s.occ)) return;
    const DevSph S = rs(k);
    if (need && !(OCC && s.occ)) {
      ++s.tests;
      float t2;
      if (ref_sph(S, s.o, s.L, t2) && !(t2 >= s.t)) {
        if (OCC) {
          s.occ = true;
        } else {
          s.t = t2;
          s.u = s.v = 0.f;
          s.id = p.n_tri + k;
        }
      }
    }
  }
}

DEVINL bool coord_ok(float x) { return fabsf(x) < 0x1p60f; } // false for NaN and +-inf

} // namespace

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
      if (p.tg.n_grp > 0) tri_groups<OCC>(p, rs, rt, s);
      else tri_linear<OCC>(p, rs, rt, s);
    }
    if (p.n_sph > 0) {
      if (p.sg.n_grp > 0) sph_groups<OCC>(p, rs, s);
      else sph_linear<OCC>(p, rs, s);
    }
  }
  const bool need = valid && !elig;
  s.live = false;
  exact_sweep<OCC>(p, need, s);

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
