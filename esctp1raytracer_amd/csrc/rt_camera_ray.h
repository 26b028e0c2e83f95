// rt_camera_ray.h -- camera.h:31-34 get_ray with a sub-pixel offset, for one pixel: the operations of
// k_camera_rays (rt_shade_rays.hip), shared with the kernels that make a camera ray in-lane instead of
// reading it from memory (rt_adaptive.hip) or send it through a lens (rt_lens.hip).  One copy of these
// statements, so that all give the same bits; with dx = dy = 0 they are primary_dir's (rt_kernels.hip).
#pragma once
#include "rt_math.h"

namespace esc {
namespace {

// the point of the image plane the frame's ray through (w + dx, h + dy) aims at, relative to the origin:
// s = (w + dx) / (W - 1), t = (h + dy) / (H - 1).  Its component along the view axis is 1 (camera.h:16-29)
DEVINL f3 camera_ray_point(f3 origin, const float *llc, const float *horizontal, const float *vertical, int W,
                           int H, int w, int h, float dx, float dy) {
  const float is = ((float)w + dx) / (float)(W - 1);
  const float it = ((float)h + dy) / (float)(H - 1);
  return ((ld3(llc) + ld3(horizontal) * is) + ld3(vertical) * it) - origin;
}

// direction of that ray
DEVINL f3 camera_ray_dir(f3 origin, const float *llc, const float *horizontal, const float *vertical, int W,
                         int H, int w, int h, float dx, float dy) {
  return normalize(camera_ray_point(origin, llc, horizontal, vertical, W, H, w, h, dx, dy));
}

} // namespace
} // namespace esc
