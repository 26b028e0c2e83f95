// rt_shade_body.inc -- scan_row's body (main.cpp:698-791) for the ray of one lane, as program text that
// k_shade_rays (rt_shade_rays.hip) and k_trace (rt_trace.hip) include inside their kernel bodies.  It is
// text and not a function because k_shade_rays has to keep its instruction stream: through a
// __forceinline__ function the same statements come out with another register allocation.
//
// The includer provides   const ShadeParams &P;  const QueryParams &p = P.q;  bool valid;  f3 o, d;
//   #define SHADE_BODY_SEED   face_hash's seed           #define SHADE_BODY_PIXEL  face_hash's pixel id
//   #define SHADE_BODY_HIT_OUTPUTS (optional): the closest hit goes to P.t / P.geom / P.prim at index i
// and finds afterwards    QLane s (s.t: the closest hit's t of main.cpp:715-722, s.id: the primitive or -1),
//   bool has_hit;  f3 N;  int mi (normal and material of the hit);  float r, g, b (the colour);
//   uint32_t n_shadow, n_exact;  unsigned long long tests (the counts of esc_shade_stats).
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
#ifdef SHADE_BODY_HIT_OUTPUTS
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
#endif

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
                                                : face_hash(SHADE_BODY_SEED, SHADE_BODY_PIXEL, (uint32_t)li,
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

