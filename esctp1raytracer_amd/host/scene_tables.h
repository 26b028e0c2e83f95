// scene_tables.h -- host side of a scene upload: staging a scene into the flat HBM records
// (rt_device.h), and every per-scene table the brute-force kernels read that is computed from them
// (pair tables, the shadow filters' forms relative to the scene point g, the last light's sweep
// order, the sphere and triangle groups).  Pure host arithmetic, the statements the proofs in
// rt_brute.h rest on: rt_capi.cpp only uploads what comes out of here, and esc_scene_table shows the
// same bytes to tests on a machine without a GPU.
#pragma once
#include <cstdint>
#include <vector>

#include "../csrc/rt_device.h"
#include "scene.h"

namespace esc {

// host-side image of the HBM tables, filled by either staging front-end
struct Staged {
  std::vector<DevTri> tri;
  std::vector<DevTriN> tri_n; // empty when no geometry has normals
  std::vector<DevSph> sph;
  std::vector<int32_t> sph_mat;
  std::vector<DevMat> mat;
  std::vector<float> transmit; // 4 per entry of mat: tf[3], ni
  std::vector<DevLight> lights;
  std::vector<float> light_points; // xyz0
  int n_geom = 0;
};

// ESC_OK, or ESC_ERR_INVALID with the message set (a light without sample points, a bad index)
int stage_scene(const esc_scene &scene, Staged &s);
int stage_flat(int32_t nt, const ispc_triangle *tris, int32_t nl, const ispc_light *lights,
               int32_t nlt, const ispc_triangle *ltris, Staged &s);

// what a scene upload computes from the staged records; one member per device table
struct SceneTables {
  std::vector<DevSphPair> sph2;                    // rt_device.h DevSphPair
  std::vector<DevSphPairF> sph2_f;                 // shadow filter form (rt_brute.h "FILTERS")
  std::vector<DevSphPair> sph2_ord;                // the last light's sweep order: empty below 256
  std::vector<DevSphPairF> sph2_f_ord;             // spheres or without a light
  std::vector<DevTriPairF> tri2_f;                 // rt_brute.h "Triangle FILTERS"
  std::vector<DevTriPairPF> tri2_pf;               // rt_brute.h "Triangle pre-filter"
  std::vector<DevSph> sg_sorted;                   // rt_device.h SphGroups: empty below
  std::vector<DevSphGroup> sg_grp;                 // kSphGroupMinSpheres
  std::vector<DevIdx4> sg_orig;
  std::vector<DevSphPair> sg_sorted2;
  std::vector<DevSphPairF> sg_sorted2_f, sg_grp2_f;
  std::vector<DevTri> tg_sorted;                   // rt_device.h TriGroups: empty below
  std::vector<DevTriGroup> tg_grp;                 // kTriGroupMinTris
  std::vector<DevIdx4> tg_orig;
  std::vector<DevTriPairF> tg_sorted2_f;
  std::vector<DevTriPairPF> tg_sorted2_pf, tg_grp2_pf;
  float g[3] = {0, 0, 0};                          // the scene point the shadow filters work around
  float rho_max = 0.f;                             // origins further from g take the exact path
  float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0}; // grown scene box (light lists)
  int32_t sg_n_grp = 0, sg_n_sup = 0, sg_n_hyp = 0;
  int32_t tg_n_grp = 0, tg_n_sup = 0, tg_n_hyp = 0;
  bool any_transmissive = false; // some entry of Staged::transmit passes the kernel's test
  int min_light_faces = 0;       // smallest face count among the lights (bounds ESC_FACE_FIXED)
};

void build_scene_tables(const Staged &s, SceneTables &t);

// A sufficient condition (DESIGN.md 3.9 "Frames that need no fallback") for: every shadow-ray origin
// fl(origin + dir (t - eps)) of a camera at `origin`, over every unit direction and every primary hit the
// kernels accept, lies in [lo, hi] = SceneTables::scene_lo / scene_hi.  It looks at the camera's distance
// from the box, the box's size and the camera's height over each triangle's plane.  false: not proved
// (too far away, nearly in a triangle's plane, more than one light, something not finite).
bool shadow_origins_inside(const float origin[3], const float lo[3], const float hi[3], const DevTri *tri,
                           size_t n_tri, int n_lights);

} // namespace esc
