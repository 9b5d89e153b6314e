// ssrlcv_amd/csrc/sift_sampling.h -- the SIFT sampling expressions whose rounding sequence is part of the result: the
// orientation histogram and its peaks (computeThetas, src/FeatureFactory.cu:1004-1112) and the descriptor votes and bytes
// (fillDescriptors, src/SIFT_FeatureFactory.cu:475-549).
//
// THE RULE: a result-defining sampling expression is written once, here.  The per-kernel exports of keypoints.hip
// (k_x_gradients, k_x_thetas, k_x_descriptors) and the dense path (dense.hip) are built from these functions, so "dense =
// chain of exports" holds by construction for everything below.  A kernel that restates one of them for speed (k_polar,
// k_thetas, the body of k_descriptors) says at the restatement which function it restates, and is held to it by the tests.
// Every expression keeps its parentheses, its operand order, IEEE divisions, and __builtin_fmaf only where the caller
// writes it; the library is built with -ffp-contract=off and nothing here relies on anything else for its rounding.
#pragma once
#include "device_math.h"

namespace svf {

constexpr float pi = SSRLCV_PI_F;
constexpr float twoPi = 2.0f * pi;
constexpr float rad10 = pi / 18.0f;  // one of the 36 orientation bins (FeatureFactory.cu:1029)
constexpr float rad45 = pi / 4.0f;   // one of the 8 descriptor directions (SIFT_FeatureFactory.cu:489)
constexpr int kMaxPeaks = 8;         // maxOrientations of the ABI

// ---- orientation side (src/FeatureFactory.cu:1004-1112; the gradient: calculatePixelGradients, src/Image.cu:1583-1598)

// central differences of the level `at(flat index)`; a border pixel takes the stencil of its inner neighbour
template <typename At>
__device__ __forceinline__ float2 gradient_taps(int x, int y, int W, int H, At at) {
  int xc0 = x + 1, xc1 = x - 1, yc0 = y + 1, yc1 = y - 1;
  if (xc1 == -1) { xc0 += 1; xc1 += 1; }
  else if (xc0 == W) { xc0 -= 1; xc1 -= 1; }
  if (yc1 == -1) { yc0 += 1; yc1 += 1; }
  else if (yc0 == H) { yc0 -= 1; yc1 -= 1; }
  return make_float2(at((size_t)y * W + xc0) - at((size_t)y * W + xc1), at((size_t)yc0 * W + x) - at((size_t)yc1 * W + x));
}
// {magnitude, raw atan2} of a gradient (:1040-1043, SIFT_FeatureFactory.cu:508-509)
__device__ __forceinline__ float2 polar_of(float2 g) {
  return make_float2(sqrtf((g.x * g.x) + (g.y * g.y)), sv_atan2f(g.y, g.x));
}
// histogram bin of a raw atan2 (:1040-1041).  The quotient can come out as 36: such a sample votes nowhere.
__device__ __forceinline__ int orientation_bin(float atan2) {
  const float angle = fmodf(atan2 + twoPi, twoPi);
  return (int)floorf(angle / rad10);
}
// half width of the orientation window in pixels (:1024)
__host__ __device__ __forceinline__ float orientation_window(float sigma, float lambda, float pixelWidth) {
  return ceilf(sigma * 3.0f * lambda / pixelWidth);
}
// Gaussian weight of the sample at offset (tx, ty) from the key point (:1028, :1043)
__device__ __forceinline__ float orientation_weight_denom(float sigma, float lambda) { return 2.0f * lambda * lambda * sigma * sigma; }
__device__ __forceinline__ float orientation_weight(float tx, float ty, float denom) { return sv_expf(-((tx * tx) + (ty * ty)) / denom); }
// Peaks of the 36-bin histogram hist(bin) (:1050-1100): threshold, circular-neighbour tests, parabolic offset, and the
// reference's insertion loop into bx (magnitudes, descending) / by (angles).  A slot with bx == 0 holds no peak.
template <typename Hist>
__device__ __forceinline__ void pick_orientations(Hist hist, int regNumOrient, float threshold, float (&bx)[kMaxPeaks], float (&by)[kMaxPeaks]) {
  float maxHist = 0.0f;
  for (int i = 0; i < 36; ++i)
    if (hist(i) > maxHist) maxHist = hist(i);
  maxHist *= threshold;
  for (int i = 0; i < kMaxPeaks; ++i) { bx[i] = 0.0f; by[i] = 0.0f; }
  for (int b = 0; b < 36; ++b) {
    const float hb = hist(b), hp = hist(b == 0 ? 35 : b - 1), hn = hist(b == 35 ? 0 : b + 1);
    if (hb < maxHist || hb < hp || hb < hn || hb < bx[regNumOrient - 1]) continue;
    float tx = hb;
    float ty = (hp - hn) / (hp - (2.0f * hb) + hn);
    ty *= (pi / 36.0f);
    ty += (b * rad10);
    ty = fmodf(ty + twoPi, twoPi);
    for (int i = 0; i < regNumOrient; ++i) {
      if (tx > bx[i]) {
        for (int ii = i; ii < regNumOrient; ++ii) {
          const float sx = bx[ii], sy = by[ii];
          bx[ii] = tx;
          by[ii] = ty;
          tx = sx;
          ty = sy;
        }
      }
    }
  }
}

// ---- descriptor side (src/SIFT_FeatureFactory.cu:475-549)

// half width of the descriptor window in pixels (:487)
__host__ __device__ __forceinline__ float descriptor_window(float sigma, float lambda, float pixelWidth) {
  return ceilf(sigma * lambda / pixelWidth);
}
// 2^k, the fixed-point scale of the votes: a bin receives at most (windowWidth + 2)^2 votes of at most sqrt(2), and k is
// the largest power with that bound times 2^k below 2^31
__device__ __forceinline__ float vote_scale(float windowWidth) {
  int boundExp;
  (void)frexpf(1.4143f * ((windowWidth + 2.0f) * (windowWidth + 2.0f)), &boundExp);
  return ldexpf(1.0f, 31 - boundExp);
}
// what a descriptor's samples share (:487-498)
struct DescriptorFrame { float windowWidth, binWidth, c, s, voteScale; };
__device__ __forceinline__ DescriptorFrame descriptor_frame(float sigma, float theta, float lambda, float pixelWidth) {
  DescriptorFrame f;
  f.windowWidth = descriptor_window(sigma, lambda, pixelWidth);
  f.binWidth = f.windowWidth / 2.0f;
  f.c = sv_cosf(-theta);
  f.s = sv_sinf(-theta);
  f.voteScale = vote_scale(f.windowWidth);
  return f;
}
// window offset (x, y) in the key point's rotated frame (:503-505); false: outside the window, the sample is skipped
__device__ __forceinline__ bool rotate_sample(const DescriptorFrame& f, float x, float y, float& cx, float& cy) {
  cx = (x * f.c) + (y * f.s);
  cy = (-x * f.s) + (y * f.c);
  return !(fabsf(cx) > f.windowWidth || fabsf(cy) > f.windowWidth);
}
// Gaussian weight of the sample at (cx, cy) (:508) and its direction relative to the key point's (:509)
__device__ __forceinline__ float sample_weight(const DescriptorFrame& f, float cx, float cy) {
  return sv_expf(-((cx * cx) + (cy * cy)) / (2.0f * f.windowWidth * f.windowWidth));
}
__device__ __forceinline__ float relative_angle(float atan2, float theta) { return fmodf(atan2 - theta + twoPi, twoPi); }
// cell (nx, ny) of the 4 x 4 grid against the sample (:511-514): does it vote there, and hx, hy in units of binWidth
__device__ __forceinline__ bool cell_offsets(const DescriptorFrame& f, int nx, int ny, float cx, float cy, float& hx, float& hy) {
  hx = ((float)nx * 0.5f - 0.75f) * f.windowWidth;
  hy = ((float)ny * 0.5f - 0.75f) * f.windowWidth;
  const float rx = (hx * f.c) + (hy * f.s), ry = (-hx * f.s) + (hy * f.c);
  hx = fabsf(rx - cx);
  hy = fabsf(ry - cy);
  const bool passes = hx <= f.binWidth && hy <= f.binWidth;
  hx = hx / f.binWidth;
  hy = hy / f.binWidth;
  return passes;
}
// direction k of the 8 against the sample's relative angle (:515-517): does it vote there, and the offset in units of 45 degrees
__device__ __forceinline__ bool direction_offset(float ang, int k, float& angle) {
  angle = fabsf(ang - ((float)k * rad45));
  const bool passes = angle < rad45;
  angle /= rad45;
  return passes;
}
// the vote (:518-521) as the integer nearest to temp * 2^k, halves up: integer sums do not depend on the order
__device__ __forceinline__ unsigned vote_fixed(float hx, float hy, float angle, float mag, float voteScale) {
  const float temp = (1.0f - hx) * (1.0f - hy) * (1.0f - angle) * mag;
  const float q = temp * voteScale, f = floorf(q);
  return (unsigned)f + ((q - f) >= 0.5f ? 1u : 0u);
}
// normalise, clamp at 0.2, and the norm of the clamped vector (:529-541).  Lane l of a wave holds bins l and l + 64 (in
// [nx][ny][k] order); both norms are balanced trees: pairs 64 apart first, then sv::wave_sum's butterfly.
__device__ __forceinline__ float normalise_pair(float& v0, float& v1) {
  float sq = sqrtf(sv::wave_sum((v0 * v0) + (v1 * v1)));
  v0 = v0 / sq;
  v1 = v1 / sq;
  v0 = v0 > 0.2f ? 0.2f : v0;
  v1 = v1 > 0.2f ? 0.2f : v1;
  return sqrtf(sv::wave_sum((v0 * v0) + (v1 * v1)));
}
__device__ __forceinline__ uint8_t descriptor_byte(float v, float sq) { return (uint8_t)roundf(255.0f * v / sq); }
// where bin[nx][ny][k] (element = (nx * 4 + ny) * 8 + k) goes in Feature::values: (ny * 4 + nx) * 8 + k (:542)
__device__ __forceinline__ int descriptor_slot(int element) { return (((element >> 3) & 3) * 4 + (element >> 5)) * 8 + (element & 7); }

}  // namespace svf
