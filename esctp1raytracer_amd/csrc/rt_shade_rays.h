// rt_shade_rays.h -- parameter blocks of the shading of caller-supplied rays (esc_shade_rays), the
// camera-ray generator (esc_camera_rays) and the supersampling steps (esc_render_supersampled).
// Shared by rt_shade_rays.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

#include "rt_device.h"
#include "rt_query.h"

namespace esc {

struct ShadeParams {
  QueryParams q;              // n, orig, dir and the per-scene sweep tables; q.tmax / outputs unused
  float *rgb;                 // n x 3
  uint8_t *rgb8;              // n x 3, or nullptr
  float *t;                   // n, or nullptr (each of the three)
  int32_t *geom, *prim;
  const DevTriN *tri_n;       // vertex normals (nullptr when no geometry has them)
  const DevMat *mat;
  const int32_t *sph_mat;
  const DevLight *lights;
  const float *light_points;  // xyz0 per light face (quirk S2)
  int32_t n_lights;
  int32_t shadows;
  int32_t face_mode;          // ESC_FACE_*
  int32_t fixed_face;
  uint64_t seed;
  uint32_t pixel_base;        // face_hash pixel of ray i: pixel_base + i (mod 2^32)
  int32_t pad;
  unsigned long long *stats;  // esc_shade_stats: rays, hit_rays, shadow_rays, exact_rays, exact_tests
};

struct CameraRayParams {
  float origin[3], llc[3], horizontal[3], vertical[3];
  int32_t W, H;
  int64_t pix0;               // ray i is pixel pix0 + i of the frame: h = pix / W, w = pix % W
  int64_t n;
  const float *offsets;       // n x 2 (dx, dy), or nullptr: (dx, dy) below for every ray
  float dx, dy;
  float *orig, *dir;          // n x 3 each
};

} // namespace esc
