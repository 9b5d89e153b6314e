// ssrlcv_amd/csrc/bilinear_u8.h -- the one bilinear sample of a uint8 image (include/ssrlcv_hip.h "rectification", the warp's
// sample): the warp of rectify.hip and the ortho-image of ortho.hip return the same byte for the same (sx, sy).  Every operation
// is rounded on its own (the files are built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// src has pitch sw; (sx, sy) is finite; a position outside the image is clamped to its border
__device__ __forceinline__ uint32_t bilinear_u8(const uint8_t* __restrict__ src, int sw, int sh, float sx, float sy) {
  sx = fminf(fmaxf(sx, 0.0f), (float)(sw - 1));
  sy = fminf(fmaxf(sy, 0.0f), (float)(sh - 1));
  const int x0 = min((int)floorf(sx), max(sw - 2, 0)), x1 = min(x0 + 1, sw - 1);
  const int y0 = min((int)floorf(sy), max(sh - 2, 0)), y1 = min(y0 + 1, sh - 1);
  const float fx = sx - (float)x0, fy = sy - (float)y0;
  const uint8_t* r0 = src + (size_t)y0 * sw;
  const uint8_t* r1 = src + (size_t)y1 * sw;
  const float a = (float)r0[x0], b = (float)r0[x1], c = (float)r1[x0], d = (float)r1[x1];
  const float top = a + fx * (b - a);
  const float bot = c + fx * (d - c);
  const float v = top + fy * (bot - top);
  return (uint32_t)floorf(v + 0.5f);  // 0 .. 255
}
