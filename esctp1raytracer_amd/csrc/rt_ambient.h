// rt_ambient.h -- parameter blocks of ambient occlusion (esc_ambient_rays / esc_render_ambient), of sky
// lighting (esc_skylight_rays / esc_render_skylight: the same kernel with SKY), of the modulation of an
// image by a visibility (esc_modulate) and of the addition of a light to an image (esc_add_light).  Shared
// by rt_ambient.hip (device) and rt_capi.cpp (host).
#pragma once
#include <stdint.h>

#include "rt_device.h"
#include "rt_environ.h"
#include "rt_query.h"

namespace esc {

constexpr int kAmbientStats = 5;           // rays, hit_rays, occluded_samples, exact_rays, exact_tests
constexpr int kAmbientMaxDim = 64;         // sets and samples of a table: 1..64 each
constexpr uint32_t kAmbientLight = 0xFFFFFFFEu; // the hash's light index: no light, and not rt_transmit.h's

struct AmbientParams {
  // q.n, the per-scene sweep tables and exact_only; q.orig / q.dir are the caller's rays (the frame
  // variant makes its rays in-lane and leaves them null); q.tmax and q's outputs are unused
  QueryParams q;
  float *vis;                 // n (SKY: or nullptr)
  int32_t *count;             // n, or nullptr (each of the four)
  float *t;
  int32_t *geom, *prim;
  const DevTriN *tri_n;       // vertex normals (nullptr when no geometry has them)
  const DevMat *mat;
  const float *table;         // the context's table: sets x row_samples x 3 floats, local directions about +z
  int32_t samples, sets;      // K and S of this call: the first K samples of the first S sets
  int32_t row_samples;        // samples per set of the table as uploaded (the row stride, >= samples)
  float radius, bias;
  uint64_t seed;
  uint32_t pixel_base;        // the hash's pixel of ray i: pixel_base + i (mod 2^32)
  // the frame variant: ray i is pixel i of the W x H frame (h = i / W, w = i % W)
  int32_t W, H;
  float origin[3], llc[3], horizontal[3], vertical[3];
  unsigned long long *stats;  // kAmbientStats counters (zeroed per call), or nullptr: nothing is counted
  // sky lighting (the SKY instantiations only; the others never read these)
  EnvParams env;              // the context's cube
  float *sky, *light;         // n x 3 each, or nullptr (not both)
  const int32_t *sph_mat;     // material index of sphere k (already offset by n_geom)
};

struct ModulateParams {
  int64_t n;                  // pixels
  const float *rgb;           // n x 3
  const float *vis;           // n
  float *out;                 // n x 3 (may be rgb itself), or nullptr
  uint8_t *out8;              // n x 3, or nullptr
};

struct AddLightParams {
  int64_t n;                  // pixels
  const float *rgb;           // n x 3
  const float *light;         // n x 3
  float *out;                 // n x 3 (may be rgb itself), or nullptr
  uint8_t *out8;              // n x 3, or nullptr
};

} // namespace esc
