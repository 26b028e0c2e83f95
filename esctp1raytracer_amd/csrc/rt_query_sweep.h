// rt_query_sweep.h -- the sweeps of the batched ray queries, shared by k_query (rt_query.hip) and
// k_shade_rays (rt_shade_rays.hip).  One ray per lane; the preconditions (a)-(d) of the filtered
// sweep and the proof that its filters hold for the ray's whole line are written at the top of
// rt_query.hip.  Three accumulators:
//   kClosest  the smallest (t2, original index) pair with t2 < tmax: intersect() (main.cpp:176-192)
//   kAny      some pair with t2 < tmax: occlusion() (main.cpp:314-329) when its t2 is not read again
//   kFirst    the pair of the smallest ORIGINAL INDEX with t2 < tmax, and its t2: occlusion() when the
//             caller reads the t it writes back (quirk S3, the shadow rays of every light but the
//             last).  The reference returns at its first accept in index order; every pair before it
//             failed a reject or had t2 >= tmax (the bound is the caller's t, unchanged until that
//             accept), so the accept is the lowest index among the pairs that pass with t2 < tmax,
//             whatever order they are visited in.  The sweep keeps the ray looking (no early exit)
//             and keeps that minimum.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device.h"
#include "rt_math.h"
#include "rt_brute.h"
#include "rt_query.h"

namespace esc {
namespace {

constexpr int kClosest = 0;
constexpr int kAny = 1;
constexpr int kFirst = 2;


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
template <int MODE>
DEVINL void accept_free(QLane &s, int id, float t2, float u2, float v2) {
  if (MODE == kAny) {
    if (t2 < s.tmax) {
      s.occ = true;
      s.live = false;
    }
  } else if (MODE == kFirst) {
    if (t2 < s.tmax && (s.id < 0 || id < s.id)) {
      s.occ = true;
      s.t = t2;
      s.id = id;
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
template <int MODE>
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
      if (ref_tri(T, s.o, s.L, t2, u2, v2)) accept_free<MODE>(s, id, t2, u2, v2);
    }
  }
}

// 8 spheres = 4 pair records: the filter, then the reference arithmetic per candidate lane
template <int MODE>
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
      if (ref_sph(S, s.o, s.L, t2)) accept_free<MODE>(s, id, t2, 0.f, 0.f);
    }
  }
}

// the reference arithmetic on triangles [k0, k1) / spheres [k0, k1) for the live lanes (short tails)
template <int MODE>
DEVINL void tri_tail(const QueryParams &p, int k0, int k1, QLane &s) {
  const SmemFetch<DevTri> rec{p.tri};
  for (int k = k0; k < k1; ++k) {
    const DevTri T = rec(k);
    if (s.live) {
      ++s.tests;
      float t2, u2, v2;
      if (ref_tri(T, s.o, s.L, t2, u2, v2)) accept_free<MODE>(s, k, t2, u2, v2);
    }
  }
}
template <int MODE>
DEVINL void sph_tail(const QueryParams &p, int k0, int k1, QLane &s) {
  const SmemFetch<DevSph> rec{p.sph};
  for (int k = k0; k < k1; ++k) {
    const DevSph S = rec(k);
    if (s.live) {
      ++s.tests;
      float t2;
      if (ref_sph(S, s.o, s.L, t2)) accept_free<MODE>(s, p.n_tri + k, t2, 0.f, 0.f);
    }
  }
}

// ---- triangles: linear sweep over the index-order pair tables (no groups: small scenes) ----------
template <int MODE>
DEVINL void tri_linear(const QueryParams &p, const RayF &rs, const RayTF &rt, QLane &s) {
  const SmemFetch<TriPairPF> recp{reinterpret_cast<const TriPairPF *>(p.tri2_pf)};
  const int n4 = p.n_tri & ~3;
  for (int k = 0; k < n4; k += 4) {
    if (MODE == kAny && !__builtin_amdgcn_ballot_w64(s.live)) return;
    const TriPairPF P[2] = {recp(k >> 1), recp((k >> 1) + 1)};
    tri4<MODE>(P, p.tri2_f + (k >> 1), p.tri + k, nullptr, k, rs, rt, s);
  }
  tri_tail<MODE>(p, n4, p.n_tri, s); // < 4 left: straight to the reference arithmetic
}

// ---- triangles: the three group levels of rt_brute.h anyhit_tri_groups_filter, every opened group
// visited (the "lights before the last" mode), closest-hit accumulator ---------------------------
template <int MODE>
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
      tri4<MODE>(P, G.sorted2_f + r, G.sorted + 8 * gi + 4 * h, orig + 8 * gi + 4 * h, 0, rs, rt, s);
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
    if (MODE == kAny && !__builtin_amdgcn_ballot_w64(s.live)) return;
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
template <int MODE>
DEVINL void sph_linear(const QueryParams &p, const RayF &rf, QLane &s) {
  const int n_rec = (p.n_sph + 1) >> 1;
  const int r4 = n_rec & ~3;
  for (int r = 0; r < r4; r += 4) {
    if (MODE == kAny && !__builtin_amdgcn_ballot_w64(s.live)) return;
    sph8<MODE>(p.sph2_f + r, p.sph + 2 * r, nullptr, p.n_tri + 2 * r, rf, s);
  }
  sph_tail<MODE>(p, 2 * r4, p.n_sph, s);
}

// ---- spheres: the three group levels of rt_brute.h anyhit_sph_groups_filter ------------------
template <int MODE>
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
    sph8<MODE>(G.sorted2_f + 4 * gi, G.sorted + 8 * gi, orig + 8 * gi, p.n_tri, rf, s);
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
    if (MODE == kAny && !__builtin_amdgcn_ballot_w64(s.live)) return;
    uint32_t mask = open_mask(recy, y0 >> 1);
    while (mask) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1;
      supers(y0 + j);
    }
  }
}

// ---- the exact sweep: the reference loop itself for the lanes in `need` ----------------------
template <int MODE>
DEVINL void exact_sweep(const QueryParams &p, bool need, QLane &s) {
  if (!__builtin_amdgcn_ballot_w64(need)) return;
  const SmemFetch<DevTri> rt{p.tri};
  for (int k = 0; k < p.n_tri; ++k) {
    if (MODE != kClosest && (k & 31) == 0 && !__builtin_amdgcn_ballot_w64(need && !s.occ)) return;
    const DevTri T = rt(k);
    if (need && !(MODE != kClosest && s.occ)) {
      ++s.tests;
      float t2, u2, v2;
      if (ref_tri(T, s.o, s.L, t2, u2, v2) && !(t2 >= s.t)) { // ray_triangle.h:49-54
        if (MODE == kAny) {
          s.occ = true;
        } else if (MODE == kFirst) {
          s.occ = true;
          s.t = t2;
          s.id = k;
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
    if (MODE != kClosest && (k & 31) == 0 && !__builtin_amdgcn_ballot_w64(need && !s.occ)) return;
    const DevSph S = rs(k);
    if (need && !(MODE != kClosest && s.occ)) {
      ++s.tests;
      float t2;
      if (ref_sph(S, s.o, s.L, t2) && !(t2 >= s.t)) {
        if (MODE == kAny) {
          s.occ = true;
        } else if (MODE == kFirst) {
          s.occ = true;
          s.t = t2;
          s.id = p.n_tri + k;
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

// the precondition gate (a)-(d) of rt_query.hip for the ray (o, L) with bound tmax: true = a live ray
// (`valid`) that may take the filtered sweep.  rt / rs receive the ray's filter forms.
DEVINL bool filter_gate(const QueryParams &p, bool valid, f3 o, f3 L, float tmax, RayTF &rt, RayF &rs) {
  bool far;
  rt = make_ray_tri_filter(o, L, p.g, p.rho_max, far);
  rs = make_ray_filter(o, L, p.g);
  const double dd = ((double)L.x * L.x + (double)L.y * L.y) + (double)L.z * L.z;
  const bool finite = coord_ok(o.x) && coord_ok(o.y) && coord_ok(o.z) && coord_ok(L.x) && coord_ok(L.y) &&
                      coord_ok(L.z);
  const bool unit = fabs(dd - 1.0) <= 7.5 * 0x1p-24;
  return valid && !p.exact_only && finite && !far && unit && !(tmax != tmax);
}

} // namespace
} // namespace esc
