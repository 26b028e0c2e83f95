// rt_environ.hip -- env(d) for directions of the caller's own (esc_environment_rays):
// background plates, and the lookup of rt_environ.h on its own, without tracing.  One direction per
// lane, 64-bit indices.  Same arithmetic contract as rt_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_environ.h"
#include "rt_shade.h"

namespace esc {

__global__ __launch_bounds__(256) void k_environment_rays(const EnvRaysParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  float r, g, b; // an undefined direction: zeros
  env_lookup(p.env.texels, p.env.res, p.dirs[3 * i], p.dirs[3 * i + 1], p.dirs[3 * i + 2], r, g, b);
  if (p.rgb) {
    p.rgb[3 * i] = r;
    p.rgb[3 * i + 1] = g;
    p.rgb[3 * i + 2] = b;
  }
  if (p.rgb8) {
    p.rgb8[3 * i] = quantise_channel(r);
    p.rgb8[3 * i + 1] = quantise_channel(g);
    p.rgb8[3 * i + 2] = quantise_channel(b);
  }
}

} // namespace esc

extern "C" int esc_launch_environment_rays(const esc::EnvRaysParams *p, hipStream_t stream) {
  if (p->n <= 0) return 0;
  hipLaunchKernelGGL(esc::k_environment_rays, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
