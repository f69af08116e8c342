// flow_warp's per-pixel sampling (arch.py:3068-3099), the one definition that flow_warp_kernel (pointwise.hip) and
// flow_warp_frames_kernel (sequence.hip) share: the two kernels differ in where an image and its motion field come from, never
// in what a pixel computes.
#pragma once
#include "common.h"

// Four channels of output pixel (x, y) of one image: the bilinear sample at (x + mv_x, y + mv_y), zeros outside,
// align_corners=True, with the same normalise / un-normalise arithmetic as F.grid_sample.
//   img: the image's pixel (0, 0) at the thread's channel group, pixel pitch ldi floats; m: the image's [2][H][W] planes (x, y);
//   wm, hm: max(W - 1, 1), max(H - 1, 1) as floats.
__device__ __forceinline__ f32x4 flow_warp_sample(const float* __restrict__ img, int ldi, const float* __restrict__ m, int x, int y,
                                                  int H, int W, float wm, float hm) {
  const float fx = m[(long long)y * W + x], fy = m[(long long)(H + y) * W + x];
  const float nx = 2.0f * ((float)x + fx) / wm - 1.0f;
  const float ny = 2.0f * ((float)y + fy) / hm - 1.0f;
  const float sx = ((nx + 1.f) / 2.f) * (float)(W - 1);
  const float sy = ((ny + 1.f) / 2.f) * (float)(H - 1);
  // a sample at or beyond one pixel outside the image has no corner inside it: the result is 0 (grid_sample, zeros
  // padding).  Decided in floating point BEFORE any conversion to int -- the reference's mv2mvs leaves x / 0 = inf in the
  // motion field (test_LD_22_FPS.py:106-110) and float -> int of inf / NaN is undefined
  if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return f32x4{0.f, 0.f, 0.f, 0.f};
  const float x0f = floorf(sx), y0f = floorf(sy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float tx = sx - x0f, ty = sy - y0f;
  const float w00 = (1.f - tx) * (1.f - ty), w01 = tx * (1.f - ty), w10 = (1.f - tx) * ty, w11 = tx * ty;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
  if (y0 >= 0 && y0 < H) {
    if (xa) acc += *reinterpret_cast<const f32x4*>(img + ((long long)y0 * W + x0) * ldi) * w00;
    if (xb) acc += *reinterpret_cast<const f32x4*>(img + ((long long)y0 * W + x0 + 1) * ldi) * w01;
  }
  if (y0 + 1 >= 0 && y0 + 1 < H) {
    if (xa) acc += *reinterpret_cast<const f32x4*>(img + ((long long)(y0 + 1) * W + x0) * ldi) * w10;
    if (xb) acc += *reinterpret_cast<const f32x4*>(img + ((long long)(y0 + 1) * W + x0 + 1) * ldi) * w11;
  }
  return acc;
}
