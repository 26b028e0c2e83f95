// scene_tables.cpp -- staging a scene into flat records and the per-scene tables computed from them
// (scene_tables.h).  Host only.  Every expression here is part of the arithmetic contract of the
// filters (rt_brute.h): operand order, double / float casts and constants are what the proofs
// quote, and the file is compiled with -ffp-contract=off like the rest of the library.
#include "scene_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "accel_build.h"

namespace esc {

// ---- staging ------------------------------------------------------------------------------------
namespace {

esc::DevMat dev_material(const esc::Material &m, bool has_normals) {
  esc::DevMat d;
  std::memset(&d, 0, sizeof(d));
  std::memcpy(d.ka, m.ka, 12);
  std::memcpy(d.kd, m.kd, 12);
  std::memcpy(d.ks, m.ks, 12);
  std::memcpy(d.ke, m.ke, 12);
  d.Ns = m.Ns;
  d.has_normals = has_normals ? 1 : 0;
  d.spec_free = esc::material_spec_free(d.ks, d.Ns);
  return d;
}

esc::DevTri dev_triangle(const float *v0, const float *v1, const float *v2, int geom) {
  esc::DevTri t;
  std::memset(&t, 0, sizeof(t));
  for (int i = 0; i < 3; i++) {
    t.v0[i] = v0[i];
    t.e1[i] = v1[i] - v0[i]; // ray_triangle.h:14
    t.e2[i] = v2[i] - v0[i]; // ray_triangle.h:15
  }
  t.geom = geom;
  return t;
}

void push_light_point(Staged &s, const float *v) {
  // main.cpp:753-754 with v0 = v1 = v2: P = v0 + ((v1-v0)*r1 + (v2-v0)*r2) = v0 + (+0)
  s.light_points.push_back(v[0] + 0.0f);
  s.light_points.push_back(v[1] + 0.0f);
  s.light_points.push_back(v[2] + 0.0f);
  s.light_points.push_back(0.0f);
}

void push_transmission(Staged &s, const esc::Transmission &t) {
  s.transmit.insert(s.transmit.end(), t.tf, t.tf + 3);
  s.transmit.push_back(t.ni);
}

} // namespace

int stage_scene(const esc_scene &scene, Staged &s) {
  bool any_normals = false;
  for (const auto &g : scene.geometry) any_normals |= !g.normals.empty();
  s.n_geom = (int)scene.geometry.size();
  for (size_t gi = 0; gi < scene.geometry.size(); gi++) { // main.cpp:179-180 order
    const esc::Geometry &g = scene.geometry[gi];
    const bool hn = !g.normals.empty();
    s.mat.push_back(dev_material(g.object_material, hn));
    push_transmission(s, g.transmission);
    for (size_t f = 0; f < g.n_faces(); f++) {
      const uint32_t *face = &g.face_index[3 * f];
      s.tri.push_back(dev_triangle(&g.vertex[3 * face[0]], &g.vertex[3 * face[1]],
                                   &g.vertex[3 * face[2]], (int)gi));
      s.tri.back().pad[0] = (int32_t)f; // face index within the geometry: the ray queries' prim
      if (any_normals) {
        esc::DevTriN n;
        std::memset(&n, 0, sizeof(n));
        if (hn) {
          std::memcpy(n.n0, &g.normals[3 * face[0]], 12);
          std::memcpy(n.n1, &g.normals[3 * face[1]], 12);
          std::memcpy(n.n2, &g.normals[3 * face[2]], 12);
        }
        s.tri_n.push_back(n);
      }
    }
  }
  for (size_t k = 0; k < scene.spheres.size(); k++) {
    const esc::Sphere &sp = scene.spheres[k];
    esc::DevSph d;
    d.cx = sp.cx;
    d.cy = sp.cy;
    d.cz = sp.cz;
    d.r2 = sp.r * sp.r;
    s.sph.push_back(d);
    s.sph_mat.push_back(s.n_geom + (int)k);
    s.mat.push_back(dev_material(scene.sphere_materials[k], false));
    push_transmission(s, k < scene.sphere_transmission.size() ? scene.sphere_transmission[k] : esc::Transmission());
  }
  for (size_t li : scene.light_sources) { // main.cpp:740-748
    const esc::Geometry &g = scene.geometry[li];
    if (g.n_faces() == 0) {
      set_error("light geometry has no faces: light.vertex[faceID] (main.cpp:748) has nothing "
                "to sample");
      return ESC_ERR_INVALID;
    }
    if (g.n_faces() > g.n_vertices()) {
      set_error("light geometry has more faces than vertices: light.vertex[faceID] "
                "(main.cpp:748) would read out of range");
      return ESC_ERR_INVALID;
    }
    esc::DevLight L;
    L.first_point = (int)(s.light_points.size() / 4);
    L.n_faces = (int)g.n_faces();
    for (size_t k = 0; k < g.n_faces(); k++) push_light_point(s, &g.vertex[3 * k]);
    s.lights.push_back(L);
  }
  return ESC_OK;
}

int stage_flat(int32_t nt, const ispc_triangle *tris, int32_t nl, const ispc_light *lights,
               int32_t nlt, const ispc_triangle *ltris, Staged &s) {
  int max_geom = -1;
  bool any_normals = false;
  for (int i = 0; i < nt; i++) {
    if (tris[i].geom_id < 0) {
      set_error("ispc_triangle.geom_id < 0");
      return ESC_ERR_INVALID;
    }
    max_geom = std::max(max_geom, (int)tris[i].geom_id);
    any_normals |= tris[i].has_normals != 0;
  }
  s.n_geom = max_geom + 1;
  s.mat.resize((size_t)s.n_geom);
  std::memset(s.mat.data(), 0, s.mat.size() * sizeof(esc::DevMat));
  for (int g = 0; g < s.n_geom; g++) push_transmission(s, esc::Transmission()); // the seam carries none
  for (int i = 0; i < nt; i++) {
    const ispc_triangle &t = tris[i];
    s.tri.push_back(dev_triangle(t.vertices[0], t.vertices[1], t.vertices[2], t.geom_id));
    s.tri.back().pad[0] = i; // index in triangles[]: the ray queries' prim
    esc::DevMat &m = s.mat[(size_t)t.geom_id]; // material is replicated per triangle
    std::memcpy(m.ka, t.ka, 12);
    std::memcpy(m.kd, t.kd, 12);
    std::memcpy(m.ks, t.ks, 12);
    std::memcpy(m.ke, t.ke, 12);
    m.Ns = t.Ns;
    m.has_normals = t.has_normals ? 1 : 0;
    m.spec_free = esc::material_spec_free(m.ks, m.Ns);
    if (any_normals) {
      esc::DevTriN n;
      std::memset(&n, 0, sizeof(n));
      if (t.has_normals) {
        std::memcpy(n.n0, t.normals[0], 12);
        std::memcpy(n.n1, t.normals[1], 12);
        std::memcpy(n.n2, t.normals[2], 12);
      }
      s.tri_n.push_back(n);
    }
  }
  for (int li = 0; li < nl; li++) {
    const ispc_light &L = lights[li];
    esc::DevLight D;
    D.first_point = (int)(s.light_points.size() / 4);
    if (L.num_light_faces < 1 || !L.light_faces) {
      // the face draw of main.cpp:743-748 is `% face count`; an empty light has no sample point
      set_error("ispc_light.num_light_faces must be >= 1 and light_faces non-null");
      return ESC_ERR_INVALID;
    }
    D.n_faces = L.num_light_faces;
    // the scalar path's light.vertex[k], k < n_faces, is corner k%3 of light face k/3
    for (int k = 0; k < L.num_light_faces; k++) {
      const int fi = L.light_faces[k / 3];
      if (fi < 0 || fi >= nlt) {
        set_error("ispc_light.light_faces index out of range");
        return ESC_ERR_INVALID;
      }
      push_light_point(s, ltris[fi].vertices[k % 3]);
    }
    s.lights.push_back(D);
  }
  return ESC_OK;
}

// ---- the tables ---------------------------------------------------------------------------------
namespace {

constexpr float kInf = __builtin_huge_valf();

// a bound computed in double, rounded UP to fp32
float round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafterf(f, kInf);
  return f;
}

// ... and a filter record's km: a non-finite centre or radius gives km = NaN, and the x86 default
// NaN is NEGATIVE: read as an int32 it would say "never a candidate"; +inf says "always one" (the
// exact code decides)
float round_up_km(double km) {
  const float kf = round_up(km);
  return kf != kf ? kInf : kf;
}

const DevSph kPadSph = {0.f, 0.f, 0.f, -kInf}; // cc = +inf: never hit

void pair_half(DevSphPair &P, int h, const DevSph &q) {
  P.cx[h] = q.cx;
  P.cy[h] = q.cy;
  P.cz[h] = q.cz;
  P.r2[h] = q.r2;
}

// one half of a shadow filter record (rt_brute.h, proof next to pair4_any_filter_pk): the centre
// relative to g, km rounded UP from double
void filter_half(DevSphPairF &F, int h, const float g[3], double cx, double cy, double cz, double r2) {
  const float c[3] = {(float)(cx - g[0]), (float)(cy - g[1]), (float)(cz - g[2])};
  const double c2 = (double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2];
  const double km = r2 - c2 + 0x1p-16 * (c2 + std::fabs(r2)) + 0x1p-120;
  F.cx[h] = c[0];
  F.cy[h] = c[1];
  F.cz[h] = c[2];
  F.km[h] = round_up_km(km);
}

void filter_pad_half(DevSphPairF &F, int h) {
  F.cx[h] = F.cy[h] = F.cz[h] = 0.f;
  F.km[h] = -kInf; // q' = -inf: never a candidate
}

// filter form of a triangle table for shadow rays (rt_brute.h "Triangle FILTERS"), in double,
// margins rounded up
std::vector<DevTriPairF> build_tri2f(const std::vector<DevTri> &src, const float g[3], double rho) {
  std::vector<DevTriPairF> tri2f((src.size() + 1) / 2);
  for (size_t j = 0; j < tri2f.size(); j++)
    for (int h = 0; h < 2; h++) {
      DevTriPairF &F = tri2f[j];
      const size_t k = 2 * j + h;
      float *f[15] = {&F.n1x[h], &F.n1y[h], &F.n1z[h], &F.e1x[h], &F.e1y[h], &F.e1z[h], &F.e2x[h],
                      &F.e2y[h], &F.e2z[h], &F.k1x[h], &F.k1y[h], &F.k1z[h], &F.k2x[h], &F.k2y[h],
                      &F.k2z[h]};
      if (k >= src.size()) {
        for (float *x : f) *x = 0.f;
        F.M[h] = -1.f; // A = 0*0 + M < 0: never a candidate
        continue;
      }
      const DevTri &t = src[k];
      const float v[3] = {(float)((double)t.v0[0] - g[0]), (float)((double)t.v0[1] - g[1]),
                          (float)((double)t.v0[2] - g[2])};
      const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]},
                   vd[3] = {v[0], v[1], v[2]};
      auto cross = [](const double *a, const double *b, double *o) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
      };
      double n1[3], k1[3], k2[3];
      cross(e2, e1, n1);
      cross(e1, vd, k1);
      cross(e2, vd, k2);
      for (int a = 0; a < 3; a++) {
        *f[a] = (float)n1[a];
        *f[3 + a] = t.e1[a];
        *f[6 + a] = t.e2[a];
        *f[9 + a] = (float)k1[a];
        *f[12 + a] = (float)k2[a];
      }
      const double a1 = std::fabs(e1[0]) + std::fabs(e1[1]) + std::fabs(e1[2]);
      const double a2 = std::fabs(e2[0]) + std::fabs(e2[1]) + std::fabs(e2[2]);
      const double av = std::fabs(vd[0]) + std::fabs(vd[1]) + std::fabs(vd[2]);
      const double p12 = a1 * a2;
      const double M = 0x1p-17 * p12 * (p12 + (a1 + a2) * (av + rho)) + 0x1p-120;
      F.M[h] = round_up(M);
    }
  return tri2f;
}

// pre-filter form of a triangle table for shadow rays (rt_brute.h "Triangle pre-filter"):
// bounding sphere (G, R) in DevSphPairF form + the normal scaled by 1 / tau', in double
std::vector<DevTriPairPF> build_tri2pf(const std::vector<DevTri> &src, const float g[3], double rho) {
  std::vector<DevTriPairPF> tri2pf((src.size() + 1) / 2);
  for (size_t j = 0; j < tri2pf.size(); j++)
    for (int h = 0; h < 2; h++) {
      DevTriPairPF &F = tri2pf[j];
      const size_t k = 2 * j + h;
      F.cx[h] = F.cy[h] = F.cz[h] = 0.f;
      F.gx[h] = F.gy[h] = F.gz[h] = F.pad[h] = 0.f;
      F.km[h] = -kInf; // pad half: never a candidate, never "nearly parallel" ...
      if (k >= src.size()) {
        F.gx[h] = 4.f; // ... (|L . (4,4,4)| >= 4 / sqrt(3) > 1 for a unit L)
        F.gy[h] = 4.f;
        F.gz[h] = 4.f;
        continue;
      }
      F.km[h] = kInf; // sliver: always a candidate (g'' = 0 too)
      const DevTri &t = src[k];
      const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]};
      double G[3], s3[3], r0 = 0, r1 = 0, r2 = 0, l1 = 0, l2 = 0, a1 = 0, a2 = 0, av = 0;
      for (int a = 0; a < 3; a++) {
        s3[a] = (e1[a] + e2[a]) / 3.0;
        G[a] = (double)t.v0[a] + s3[a];
        r0 += s3[a] * s3[a];
        r1 += (e1[a] - s3[a]) * (e1[a] - s3[a]);
        r2 += (e2[a] - s3[a]) * (e2[a] - s3[a]);
        l1 += e1[a] * e1[a];
        l2 += e2[a] * e2[a];
        a1 += std::fabs(e1[a]);
        a2 += std::fabs(e2[a]);
        av += std::fabs((double)(float)((double)t.v0[a] - g[a]));
      }
      const double rad = std::sqrt(std::max(r0, std::max(r1, r2)));
      const double emax = std::sqrt(std::max(l1, l2));
      if (!(rad > 0x1p-10 * emax)) continue;
      const double u = 0x1p-24, at = rho + av, p12 = a1 * a2;
      const double tau = 3.2 * u * (10.04 * at * a2 + 5.04 * at * a1 + 20.1 * p12) * emax / rad;
      const double taup = (tau + 10.1 * u * p12) * 1.00001 + 0x1p-120;
      const double R = 2.0 * rad + 8.0 * u * (at + a1 + a2);
      const float c[3] = {(float)(G[0] - g[0]), (float)(G[1] - g[1]), (float)(G[2] - g[2])};
      const double c2 = (double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2];
      const double R2 = R * R * 1.00001;
      const double km = R2 - c2 + 0x1p-16 * (c2 + R2) + 0x1p-120;
      F.cx[h] = c[0];
      F.cy[h] = c[1];
      F.cz[h] = c[2];
      F.km[h] = round_up_km(km);
      const double n1[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2],
                            e2[0] * e1[1] - e2[1] * e1[0]};
      F.gx[h] = (float)(n1[0] / taup);
      F.gy[h] = (float)(n1[1] / taup);
      F.gz[h] = (float)(n1[2] / taup);
    }
  return tri2pf;
}

// one half of a triangle group's shadow record (rt_device.h TriGroups grp2_pf): the bounding
// sphere in DevSphPairF form and the cone axis over kappa
void tri_group_shadow_half(DevTriPairPF &F, int h, const DevTriGroup &G, const float g[3], double rho) {
  F.cx[h] = F.cy[h] = F.cz[h] = 0.f;
  F.gx[h] = F.gy[h] = F.gz[h] = F.pad[h] = 0.f;
  if (G.rgeo < 0.f) { // pad group: never a candidate, never "nearly parallel"
    F.km[h] = -kInf;
    F.gx[h] = F.gy[h] = F.gz[h] = 0x1p60f;
    return;
  }
  F.km[h] = kInf; // always open unless the bounds below are usable
  if (G.always != 0.f) return;
  const float c[3] = {(float)((double)G.cx - g[0]), (float)((double)G.cy - g[1]),
                      (float)((double)G.cz - g[2])};
  const double c1 = std::fabs((double)G.cx - g[0]) + std::fabs((double)G.cy - g[1]) +
                    std::fabs((double)G.cz - g[2]);
  const double at = rho + c1 + (double)G.rext; // >= |O - v0_t|_1 for every member and ray in range
  const double kappa = ((double)G.smax + (double)G.b0 + (double)G.b1 * at + 0x1p-20) * 1.0001;
  if (!(kappa < 1.0)) return;
  const double R = (double)G.rgeo + 0x1p-21 * at + 0x1p-60;
  const double c2 = (double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2];
  const double R2 = R * R * 1.00001;
  const double km = R2 - c2 + 0x1p-16 * (c2 + R2) + 0x1p-120;
  if (!std::isfinite(km)) return;
  F.cx[h] = c[0];
  F.cy[h] = c[1];
  F.cz[h] = c[2];
  F.km[h] = round_up(km);
  F.gx[h] = (float)((double)G.ax / kappa);
  F.gy[h] = (float)((double)G.ay / kappa);
  F.gz[h] = (float)((double)G.az / kappa);
}

} // namespace

void build_scene_tables(const Staged &s, SceneTables &t) {
  t = SceneTables();
  // pair-interleaved copy of the sphere table (rt_device.h DevSphPair)
  t.sph2.resize((s.sph.size() + 1) / 2);
  for (size_t k = 0; k < 2 * t.sph2.size(); k++)
    pair_half(t.sph2[k >> 1], (int)(k & 1), k < s.sph.size() ? s.sph[k] : kPadSph);
  // g = middle of the box of everything (sphere centres, triangle corners, light points); rho_max
  // = twice the 1-norm radius of that box around g: every primary hit point, hence every first
  // shadow-ray origin, lies inside it; origins further out (quirk S3 can start a later light's ray
  // beyond the scene) take the exact path
  float *g = t.g;
  double rho = 0.0;
  {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto grow = [&](double x, double y, double z) {
      const double c[3] = {x, y, z};
      for (int a = 0; a < 3; a++) {
        lo[a] = std::min(lo[a], c[a]);
        hi[a] = std::max(hi[a], c[a]);
      }
    };
    for (const auto &q : s.sph) {
      const double r = std::sqrt(std::max(0.0, (double)q.r2));
      grow(q.cx - r, q.cy - r, q.cz - r);
      grow(q.cx + r, q.cy + r, q.cz + r);
    }
    for (const auto &tr : s.tri) {
      grow(tr.v0[0], tr.v0[1], tr.v0[2]);
      grow((double)tr.v0[0] + tr.e1[0], (double)tr.v0[1] + tr.e1[1], (double)tr.v0[2] + tr.e1[2]);
      grow((double)tr.v0[0] + tr.e2[0], (double)tr.v0[1] + tr.e2[1], (double)tr.v0[2] + tr.e2[2]);
    }
    if (lo[0] <= hi[0]) {
      for (int a = 0; a < 3; a++) {
        g[a] = (float)(0.5 * (lo[a] + hi[a]));
        rho += std::max(hi[a] - (double)g[a], (double)g[a] - lo[a]);
      }
      rho = 2.0 * rho + 1e-30;
      // the box itself, grown by 5 % of its size and rounded outwards: the region the light lists'
      // reach is computed for (rt_lists.h "Light lists"; every first shadow-ray origin is inside)
      const double grow_by = 0.05 * ((hi[0] - lo[0]) + (hi[1] - lo[1]) + (hi[2] - lo[2])) + 1e-30;
      for (int a = 0; a < 3; a++) {
        t.scene_lo[a] = std::nextafterf((float)(lo[a] - grow_by), -kInf);
        t.scene_hi[a] = std::nextafterf((float)(hi[a] + grow_by), kInf);
      }
    }
  }
  t.rho_max = (float)rho;
  t.tri2_f = build_tri2f(s.tri, g, rho);
  // filter form of the pair table for shadow rays: centres relative to g
  t.sph2_f.resize(t.sph2.size());
  for (size_t k = 0; k < 2 * t.sph2_f.size(); k++) {
    if (k >= s.sph.size())
      filter_pad_half(t.sph2_f[k >> 1], (int)(k & 1));
    else
      filter_half(t.sph2_f[k >> 1], (int)(k & 1), g, s.sph[k].cx, s.sph[k].cy, s.sph[k].cz, s.sph[k].r2);
  }
  t.tri2_pf = build_tri2pf(s.tri, g, rho);
  // the LAST light's sweep order (ESC_RENDER_INDEX_ORDER switches it off): spheres by decreasing
  // solid angle r^2 / |c - P|^2 seen from its first sample point P.  Same records, permuted pair
  // tables (exact + filter); from 256 spheres up.
  if (!s.lights.empty() && s.sph.size() >= 256) {
    const float *P = &s.light_points[4 * (size_t)s.lights.back().first_point];
    std::vector<int> ord(s.sph.size());
    std::vector<double> key(s.sph.size());
    for (size_t k = 0; k < s.sph.size(); k++) {
      ord[k] = (int)k;
      const double dx = (double)s.sph[k].cx - P[0], dy = (double)s.sph[k].cy - P[1],
                   dz = (double)s.sph[k].cz - P[2];
      key[k] = (double)s.sph[k].r2 / std::max(dx * dx + dy * dy + dz * dz, 1e-300);
    }
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return key[a] > key[b]; });
    t.sph2_ord.resize(t.sph2.size());
    t.sph2_f_ord.resize(t.sph2_f.size());
    for (size_t pos = 0; pos < 2 * t.sph2.size(); pos++) {
      const size_t j = pos >> 1;
      const int h = (int)(pos & 1);
      if (pos < ord.size()) {
        const size_t k = (size_t)ord[pos];
        const DevSphPairF &F = t.sph2_f[k >> 1];
        pair_half(t.sph2_ord[j], h, s.sph[k]);
        t.sph2_f_ord[j].cx[h] = F.cx[k & 1];
        t.sph2_f_ord[j].cy[h] = F.cy[k & 1];
        t.sph2_f_ord[j].cz[h] = F.cz[k & 1];
        t.sph2_f_ord[j].km[h] = F.km[k & 1];
      } else { // the pad half of an odd count stays last
        pair_half(t.sph2_ord[j], h, kPadSph);
        filter_pad_half(t.sph2_f_ord[j], h);
      }
    }
  }
  DevIdx4 pad_i;
  pad_i.v[0] = pad_i.v[1] = pad_i.v[2] = pad_i.v[3] = INT32_MAX / 2;
  // sphere groups of the primary pass (rt_device.h SphGroups): spatial order, runs of kSphGroup,
  // padded to whole sweep steps
  if ((int)s.sph.size() >= kSphGroupMinSpheres) {
    std::vector<int32_t> order;
    constexpr size_t kBig = (size_t)kSphGroup * kSphSuper; // spheres per super-group
    constexpr size_t kHuge = kBig * kSphHyper;             // ... per hyper-group
    group_order(s.sph, kSphGroup, (int)kBig, (int)kHuge, order);
    const size_t n_hyp_real = (s.sph.size() + kHuge - 1) / kHuge;
    const size_t n_hyp = (n_hyp_real + kSphGroupStep - 1) / kSphGroupStep * kSphGroupStep;
    const size_t n_sup = n_hyp * kSphHyper;
    const size_t n_grp = n_sup * kSphSuper;
    t.sg_sorted.assign(n_grp * kSphGroup, kPadSph);
    DevSphGroup pad_g;
    pad_g.cx = pad_g.cy = pad_g.cz = 0.f;
    pad_g.rgeo = -1.f;
    t.sg_grp.assign(n_grp + n_sup + n_hyp, pad_g); // groups, then super-groups, then hyper-groups
    t.sg_orig.assign(n_grp * kSphGroup / 4, pad_i);
    for (size_t k = 0; k < order.size(); k++) {
      t.sg_sorted[k] = s.sph[(size_t)order[k]];
      t.sg_orig[k >> 2].v[k & 3] = order[k];
    }
    const size_t run[3] = {(size_t)kSphGroup, kBig, kHuge}, off[3] = {0, n_grp, n_grp + n_sup};
    for (int lv = 0; lv < 3; lv++)
      for (size_t first = 0; first < order.size(); first += run[lv])
        t.sg_grp[off[lv] + first / run[lv]] =
            group_bounds(s.sph, order.data() + first, (int)std::min(run[lv], order.size() - first));
    t.sg_n_grp = (int32_t)n_grp;
    t.sg_n_sup = (int32_t)n_sup;
    t.sg_n_hyp = (int32_t)n_hyp;
  }
  // ... and the same groups for shadow rays: pair tables relative to g
  t.sg_sorted2.resize(t.sg_sorted.size() / 2);
  t.sg_sorted2_f.resize(t.sg_sorted.size() / 2);
  t.sg_grp2_f.resize(t.sg_grp.size() / 2);
  for (size_t k = 0; k < t.sg_sorted.size(); k++) {
    const DevSph &q = t.sg_sorted[k];
    const int h = (int)(k & 1);
    pair_half(t.sg_sorted2[k >> 1], h, q); // pad: -inf, never hit
    if (q.r2 == -kInf)
      filter_pad_half(t.sg_sorted2_f[k >> 1], h);
    else
      filter_half(t.sg_sorted2_f[k >> 1], h, g, q.cx, q.cy, q.cz, q.r2);
  }
  for (size_t k = 0; k < t.sg_grp.size(); k++) {
    const DevSphGroup &G = t.sg_grp[k];
    const int h = (int)(k & 1);
    if (G.rgeo < 0.f) {
      filter_pad_half(t.sg_grp2_f[k >> 1], h);
      continue;
    }
    const double dx = (double)G.cx - g[0], dy = (double)G.cy - g[1], dz = (double)G.cz - g[2];
    const double R = (double)G.rgeo +
                     0x1.6p-10 * (rho + std::sqrt(dx * dx + dy * dy + dz * dz) + (double)G.rgeo) + 0x1p-60;
    filter_half(t.sg_grp2_f[k >> 1], h, g, G.cx, G.cy, G.cz, R * R * 1.00001);
  }
  // triangle groups (rt_device.h TriGroups): spatial order, groups of 8, super-groups of kTriSuper
  // groups, padded to whole sweep steps; the shadow forms of the sorted triangles and of the groups
  if ((int)s.tri.size() >= kTriGroupMinTris) {
    constexpr size_t kBig = (size_t)kTriGroup * kTriSuper;
    constexpr size_t kHuge = kBig * kTriHyper;
    std::vector<int32_t> order;
    group_order(s.tri, kTriGroup, (int)kBig, (int)kHuge, order);
    const size_t n_hyp_real = (s.tri.size() + kHuge - 1) / kHuge;
    const size_t n_hyp = (n_hyp_real + kTriGroupStep - 1) / kTriGroupStep * kTriGroupStep;
    const size_t n_sup = n_hyp * kTriHyper;
    const size_t n_grp = n_sup * kTriSuper;
    DevTri pad_t;
    std::memset(&pad_t, 0, sizeof(pad_t));
    t.tg_sorted.assign(n_grp * kTriGroup, pad_t);
    DevTriGroup pad_g;
    std::memset(&pad_g, 0, sizeof(pad_g));
    pad_g.rgeo = -1.f;
    pad_g.slack = 1.f;
    t.tg_grp.assign(n_grp + n_sup + n_hyp, pad_g);
    // shadow rays take the plain trade-off (slack 1) at every level: their cones are static, the
    // sine term dominates them and a thinner tau band buys nothing, while the larger radii cost
    std::vector<DevTriGroup> tg_grp1(t.tg_grp.size(), pad_g);
    t.tg_orig.assign(n_grp * kTriGroup / 4, pad_i);
    for (size_t k = 0; k < order.size(); k++) {
      t.tg_sorted[k] = s.tri[(size_t)order[k]];
      t.tg_orig[k >> 2].v[k & 3] = order[k];
    }
    const size_t run[3] = {(size_t)kTriGroup, kBig, kHuge}, off[3] = {0, n_grp, n_grp + n_sup};
    const float slack[3] = {kTriSlackGroup, kTriSlackSuper, kTriSlackHyper};
    for (int lv = 0; lv < 3; lv++)
      for (size_t first = 0; first < order.size(); first += run[lv]) {
        const int count = (int)std::min(run[lv], order.size() - first);
        const size_t j = off[lv] + first / run[lv];
        t.tg_grp[j] = tri_group_bounds(s.tri, order.data() + first, count, slack[lv]);
        tg_grp1[j] = tri_group_bounds(s.tri, order.data() + first, count);
      }
    t.tg_n_grp = (int32_t)n_grp;
    t.tg_n_sup = (int32_t)n_sup;
    t.tg_n_hyp = (int32_t)n_hyp;
    t.tg_sorted2_f = build_tri2f(t.tg_sorted, g, rho);
    t.tg_sorted2_pf = build_tri2pf(t.tg_sorted, g, rho);
    t.tg_grp2_pf.resize(t.tg_grp.size() / 2);
    for (size_t k = 0; k < tg_grp1.size(); k++)
      tri_group_shadow_half(t.tg_grp2_pf[k >> 1], (int)(k & 1), tg_grp1[k], g, rho);
  }
  for (size_t i = 0; i + 3 < s.transmit.size(); i += 4) { // the kernel's test (rt_transmit.h)
    const float *tr = &s.transmit[i];
    t.any_transmissive |= (tr[0] > 0.f || tr[1] > 0.f || tr[2] > 0.f) && tr[3] > 0.f;
  }
  for (size_t i = 0; i < s.lights.size(); i++)
    t.min_light_faces = (i == 0) ? s.lights[i].n_faces
                                 : std::min(t.min_light_faces, (int)s.lights[i].n_faces);
}

// DESIGN.md 3.9 "Frames that need no fallback", statement (I): the names below are the proof's.
// Everything in double; each comparison leans to "no".
bool shadow_origins_inside(const float origin[3], const float lo[3], const float hi[3], const DevTri *tri,
                           size_t n_tri, int n_lights) {
  if (n_lights != 1) return false; // quirk S3: a later light's ray starts wherever the previous t left it
  double S = 0.0, A = 0.0, M2 = 0.0, oinf = 0.0;
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(origin[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(lo[a] <= hi[a]))
      return false;
    S += (double)hi[a] - (double)lo[a];
    A = std::max(A, std::max(std::fabs((double)lo[a]), std::fabs((double)hi[a])));
    const double far = std::max(std::fabs((double)origin[a] - lo[a]), std::fabs((double)origin[a] - hi[a]));
    M2 += far * far;
    oinf = std::max(oinf, std::fabs((double)origin[a]));
  }
  const double M = std::sqrt(M2);            // the camera's distance from the farthest corner of the box
  const double m = S / 26.0 - 0x1p-22 * A;   // the margin: 0.05 of the ungrown extents' sum, S = 1.3 of it
  if (!(m > 0.0) || !std::isfinite(M)) return false;
  const double e_fp = 0x1p-20 * (1.0 + M + m + oinf); // fl(origin + dir (t - eps)), the tails' casts
  const double e_sph = 0x1p-8 * M;                    // a sphere's root: sqrt(66 u) max(|w|, r) + 4u ...
  double e_tri = 0.0;
  const double cu = 0x1p-20; // 16 u: what a numerator or det is off by, over the product of its lengths
  for (size_t i = 0; i < n_tri; i++) {
    const DevTri &T = tri[i];
    double e1[3], e2[3], w[3], n[3];
    for (int a = 0; a < 3; a++) {
      e1[a] = T.e1[a];
      e2[a] = T.e2[a];
      w[a] = (double)origin[a] - (double)T.v0[a];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double L1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    const double L2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    if (L1 == 0.0 && L2 == 0.0) continue; // a pad: det is exactly 0, never accepted
    const double A2 = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double W = 1.0001 * std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double hA2 = std::fabs(w[0] * n[0] + w[1] * n[1] + w[2] * n[2]); // h A2 = |w . (e1 x e2)|
    const double Q = cu * W * L1 * L2;
    const double Dmin = std::min(0.5 * A2 - cu * L1 * L2, (0.86 * hA2 - 3.0 * Q) / (1.0001 * (L1 + L2 + W)));
    if (!(Dmin > 0.0)) return false; // a sliver, or the camera (nearly) in the triangle's plane
    e_tri = std::max(e_tri, 4.01 * Q / Dmin);
  }
  return e_fp + std::max(e_sph, e_tri) <= m;
}

} // namespace esc
