// rt_camera_ray.h -- camera.h:31-34 get_ray with a sub-pixel offset, for one pixel: the operations of
// k_camera_rays (rt_shade_rays.hip), shared with the kernels that make a camera ray in-lane instead of
// reading it from memory (rt_adaptive.hip).  One copy of these statements, so that both give the same
// bits; with dx = dy = 0 they are primary_dir's (rt_kernels.hip).
#pragma once
#include "rt_math.h"

namespace esc {
namespace {

// direction of the frame's ray through (w + dx, h + dy): s = (w + dx) / (W - 1), t = (h + dy) / (H - 1)
DEVINL f3 camera_ray_dir(f3 origin, const float *llc, const float *horizontal, const float *vertical, int W,
                         int H, int w, int h, float dx, float dy) {
  const float is = ((float)w + dx) / (float)(W - 1);
  const float it = ((float)h + dy) / (float)(H - 1);
  return normalize(((ld3(llc) + ld3(horizontal) * is) + ld3(vertical) * it) - origin);
}

} // namespace
} // namespace esc
