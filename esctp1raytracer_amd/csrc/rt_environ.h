// rt_environ.h -- the environment cube map (esc_set_environment): the parameter blocks
// and the lookup env(d) of include/esctp1_rt.h, host + device.  Shared by rt_environ.hip and rt_trace.hip
// (device) and rt_capi.cpp (host), which exposes the lookup to the CPU tests (esc_environment_lookup_host):
// what the tests hold to the numpy restatement is this very code, the rt_tile_math.h pattern.
//
// Same arithmetic contract as rt_kernels.hip (-ffp-contract=off, correctly rounded divide): + - * /,
// floorf and compares only, one rounding per written operation.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace esc {

constexpr int kEnvMaxRes = 1024; // ESC_ENV_MAX_RES: 6 * 1024^2 records of 16 bytes are 100 MB

// one texel of the device copy: rgb plus a pad word, so that a lane fetches it with one 16-byte load
// (global_load_dwordx4) and a lookup costs four loads, not twelve.  Repacked on the host at set time.
struct alignas(16) EnvTexel {
  float r, g, b, pad;
};

struct EnvParams {
  const EnvTexel *texels; // [face][j][i], face = 2 * axis + (negative ? 1 : 0); nullptr: no environment
  int32_t res;            // R, texels per side
  int32_t pad;
};

struct EnvRaysParams { // k_environment_rays
  EnvParams env;
  int64_t n;
  const float *dirs; // n x 3
  float *rgb;        // n x 3, or nullptr
  uint8_t *rgb8;     // n x 3, or nullptr
};

#define ENV_HD __host__ __device__ __forceinline__

// x = ((u * 0.5 + 0.5) * R) - 0.5 -> the two texel indices (clamped at the face border) and the weight
ENV_HD void env_axis(float u, int32_t R, int32_t &i0, int32_t &i1, float &f) {
  const float x = ((u * 0.5f + 0.5f) * (float)R) - 0.5f; // in [-0.5, R - 0.5]
  const float x0 = floorf(x);
  f = x - x0;
  const int32_t k = (int32_t)x0; // -1 .. R - 1
  i0 = k < 0 ? 0 : (k > R - 1 ? R - 1 : k);
  i1 = k + 1 < 0 ? 0 : (k + 1 > R - 1 ? R - 1 : k + 1);
}

ENV_HD float env_mix(float t00, float t01, float t10, float t11, float fx, float fy) {
  const float c0 = t00 + (t01 - t00) * fx;
  const float c1 = t10 + (t11 - t10) * fx;
  return c0 + (c1 - c0) * fy;
}

// env(d): bilinear inside the face the direction's largest component picks, no filtering across faces.
// (0, 0, 0) for a direction with a NaN, an infinite largest component, or all zeros.
ENV_HD void env_lookup(const EnvTexel *t, int32_t R, float dx, float dy, float dz, float &r, float &g,
                       float &b) {
  r = g = b = 0.f;
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az) ? 1 : 2;
  const float c = axis == 0 ? dx : axis == 1 ? dy : dz;
  const float a = axis == 0 ? dy : axis == 1 ? dz : dx;
  const float bb = axis == 0 ? dz : axis == 1 ? dx : dy;
  const float m = fabsf(c);
  const bool defined = dx == dx && dy == dy && dz == dz && m > 0.f && m <= FLT_MAX;
  if (!defined) return;
  const float u = a / m, v = bb / m;
  int32_t i0, i1, j0, j1;
  float fx, fy;
  env_axis(u, R, i0, i1, fx);
  env_axis(v, R, j0, j1, fy);
  const EnvTexel *face = t + (size_t)(2 * axis + (c < 0.f ? 1 : 0)) * (size_t)R * (size_t)R;
  const EnvTexel t00 = face[(size_t)j0 * R + i0], t01 = face[(size_t)j0 * R + i1];
  const EnvTexel t10 = face[(size_t)j1 * R + i0], t11 = face[(size_t)j1 * R + i1];
  r = env_mix(t00.r, t01.r, t10.r, t11.r, fx, fy);
  g = env_mix(t00.g, t01.g, t10.g, t11.g, fx, fy);
  b = env_mix(t00.b, t01.b, t10.b, t11.b, fx, fy);
}

} // namespace esc
