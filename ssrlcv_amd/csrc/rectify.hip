// ssrlcv_amd/csrc/rectify.hip -- rectification of a camera pair for the dense stereo of stereo.hip: two homographies from two
// Image::Camera records (host, double), the bilinear warp that makes the rectified pair, the mask that removes the disparities
// whose windows touched replicated border, and the way back: Match records through the homographies into source pixels.
// The contract is include/ssrlcv_hip.h "rectification"; tests/rectify_ref.py restates it operation by operation.
//
//   k_warp_u8             a lane owns FOUR neighbouring output pixels of one row and writes them as one dword.  Where the row
//                         does not start on a dword boundary (dst + y dstW is odd for an odd pitch) the pixels before the
//                         first boundary go out bytewise from the row's lane 0, and so do the pixels of a group the row ends
//                         in.  Every pixel's X, Y, W come from its own (x, y), never from a running increment: an increment
//                         would change bits.  The four taps are plain byte loads through the cache: a rectifying homography is
//                         close to a similarity, so the 256 pixels of a wave read a few neighbouring source rows.
//   k_stereo_mask         one pixel per lane, 8 homography evaluations
//   k_matches_homography  one record per lane
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ssrlcv_hip.h"
#include "bilinear_u8.h"
#include "camera_host.h"
#include "device_math.h"

namespace {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kMaxSide = 1u << 24;
constexpr float kFltMax = 3.4028234663852886e38f;

struct Homography {
  float h[9];
};

// the contract's evaluation: every product and sum rounded on its own (the file is built with -ffp-contract=off)
__device__ __forceinline__ bool h_mapped(const Homography& H, float x, float y, float& sx, float& sy) {
  const float X = (H.h[0] * x + H.h[1] * y) + H.h[2];
  const float Y = (H.h[3] * x + H.h[4] * y) + H.h[5];
  const float W = (H.h[6] * x + H.h[7] * y) + H.h[8];
  sx = __fdiv_rn(X, W);
  sy = __fdiv_rn(Y, W);
  return W > 0.0f && fabsf(sx) <= kFltMax && fabsf(sy) <= kFltMax;  // a NaN fails every comparison
}

__device__ __forceinline__ bool h_inside(const Homography& H, float x, float y, float xmax, float ymax) {
  float sx, sy;
  if (!h_mapped(H, x, y, sx, sy)) return false;
  return sx >= 0.0f && sx <= xmax && sy >= 0.0f && sy <= ymax;
}

__device__ __forceinline__ uint32_t warp_pixel(const uint8_t* __restrict__ src, int sw, int sh, const Homography& H, uint32_t x, uint32_t y) {
  float sx, sy;
  if (!h_mapped(H, (float)x, (float)y, sx, sy)) return 0u;
  return bilinear_u8(src, sw, sh, sx, sy);
}

// items = rows x lanesPerRow; item (y, 0) is the row's unaligned head (0 .. 3 pixels), item (y, j >= 1) its j-th aligned group
__global__ __launch_bounds__(256) void k_warp_u8(const uint8_t* __restrict__ src, int sw, int sh, Homography H, uint8_t* __restrict__ dst,
                                                 uint32_t dw, uint32_t lanesPerRow, uint32_t items) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u) {
    const uint32_t y = i / lanesPerRow, j = i - y * lanesPerRow;
    uint8_t* row = dst + (size_t)y * dw;
    uint32_t head = (uint32_t)((4u - ((uintptr_t)row & 3u)) & 3u);
    if (head > dw) head = dw;
    if (j == 0) {
      for (uint32_t x = 0; x < head; ++x) row[x] = (uint8_t)warp_pixel(src, sw, sh, H, x, y);
      continue;
    }
    const uint32_t xa = head + 4u * (j - 1u);
    if (xa >= dw) continue;
    if (dw - xa >= 4u) {
      uint32_t v = warp_pixel(src, sw, sh, H, xa, y);
      v |= warp_pixel(src, sw, sh, H, xa + 1u, y) << 8;
      v |= warp_pixel(src, sw, sh, H, xa + 2u, y) << 16;
      v |= warp_pixel(src, sw, sh, H, xa + 3u, y) << 24;
      *reinterpret_cast<uint32_t*>(row + xa) = v;  // row + xa is on a dword boundary
    } else {
      for (uint32_t x = xa; x < dw; ++x) row[x] = (uint8_t)warp_pixel(src, sw, sh, H, x, y);
    }
  }
}

__global__ __launch_bounds__(256) void k_stereo_mask(float* __restrict__ disparity, uint32_t* __restrict__ cost, uint32_t w, uint32_t n, int r,
                                                     Homography Hl, Homography Hr, float xmax, float ymax) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const float delta = disparity[p];
    if (__float_as_uint(delta) == kNaN) continue;
    const uint32_t y = p / w, x = p - y * w;
    const float xm = (float)((int)x - r), xp = (float)((int)x + r), ym = (float)((int)y - r), yp = (float)((int)y + r);
    bool keep = h_inside(Hl, xm, ym, xmax, ymax) && h_inside(Hl, xp, ym, xmax, ymax) && h_inside(Hl, xm, yp, xmax, ymax) &&
                h_inside(Hl, xp, yp, xmax, ymax);
    if (keep) {
      const float xr = (float)x - delta;
      const float half = (float)r + 0.5f;
      const float um = xr - half, up = xr + half;
      keep = h_inside(Hr, um, ym, xmax, ymax) && h_inside(Hr, up, ym, xmax, ymax) && h_inside(Hr, um, yp, xmax, ymax) &&
             h_inside(Hr, up, yp, xmax, ymax);
    }
    if (!keep) {
      disparity[p] = __uint_as_float(kNaN);
      if (cost) cost[p] = 0xFFFFFFFFu;
    }
  }
}

__global__ __launch_bounds__(256) void k_matches_homography(ssrlcv_match* __restrict__ matches, uint32_t n, Homography H0, Homography H1, int has0,
                                                            int has1) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  ssrlcv_match* m = matches + i;
  if (m->invalid != 0) return;
  bool ok = true;
  float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
  if (has0) ok = h_mapped(H0, m->keyPoints[0].loc.x, m->keyPoints[0].loc.y, x0, y0);
  if (has1) ok = h_mapped(H1, m->keyPoints[1].loc.x, m->keyPoints[1].loc.y, x1, y1) && ok;
  if (!ok) {
    m->invalid = 1;  // one byte: the padding behind it keeps its bytes
    return;
  }
  if (has0) {
    m->keyPoints[0].loc.x = x0;
    m->keyPoints[0].loc.y = y0;
  }
  if (has1) {
    m->keyPoints[1].loc.x = x1;
    m->keyPoints[1].loc.y = y1;
  }
}

// ---- host side
bool bad_image(uint32_t w, uint32_t h) { return w > kMaxSide || h > kMaxSide || (unsigned long long)w * h >= (1ull << 31); }

Homography load_h(const float* H) {
  Homography o;
  for (int i = 0; i < 9; ++i) o.h[i] = H ? H[i] : 0.0f;
  return o;
}

unsigned capped_blocks(uint32_t items) {
  const unsigned b = (unsigned)((items + 255u) / 256u);
  return b > 2048u ? 2048u : b;
}

using camera_host::euler_matrix;
using camera_host::finite_positive;
using camera_host::M3;
using camera_host::mul;
using camera_host::transpose;

M3 adjugate(const M3& a) {  // the inverse up to the determinant, which the normalisation divides out
  M3 o;
  o.m[0][0] = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
  o.m[0][1] = a.m[0][2] * a.m[2][1] - a.m[0][1] * a.m[2][2];
  o.m[0][2] = a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1];
  o.m[1][0] = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
  o.m[1][1] = a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0];
  o.m[1][2] = a.m[0][2] * a.m[1][0] - a.m[0][0] * a.m[1][2];
  o.m[2][0] = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
  o.m[2][1] = a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1];
  o.m[2][2] = a.m[0][0] * a.m[1][1] - a.m[0][1] * a.m[1][0];
  return o;
}
double det(const M3& a) {
  return a.m[0][0] * (a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1]) - a.m[0][1] * (a.m[1][0] * a.m[2][2] - a.m[1][2] * a.m[2][0]) +
         a.m[0][2] * (a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0]);
}
// K(fi) M K(fl)^-1 T(t, ty), its last entry 1.  K^-1 is applied by columns -- col0 / fl, col1 / fl, col2 - col0' cx - col1' cy --
// so that M = identity with fi = fl gives the identity exactly
bool compose(const M3& M, double fi, double fl, double cx, double cy, double t, double ty, M3& H) {
  M3 K = {{{fi, 0.0, cx}, {0.0, fi, cy}, {0.0, 0.0, 1.0}}};
  const M3 A = mul(K, M);
  for (int i = 0; i < 3; ++i) {
    const double c0 = A.m[i][0] / fl, c1 = A.m[i][1] / fl;
    const double c2 = (A.m[i][2] - c0 * cx) - c1 * cy;
    H.m[i][0] = c0;
    H.m[i][1] = c1;
    H.m[i][2] = (c2 + c0 * t) + c1 * ty;
  }
  const double last = H.m[2][2];
  if (!finite_positive(last)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) H.m[i][j] /= last;
  return true;
}
bool inverse_normalised(const M3& H, M3& G) {
  G = adjugate(H);
  const double d = det(H);
  if (!(d > 0.0)) {  // a negative determinant turns the adjugate's sign: the inverse's last entry has the sign of adj / det
    if (!(d < 0.0)) return false;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G.m[i][j] = -G.m[i][j];
  }
  const double last = G.m[2][2];
  if (!finite_positive(last)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) G.m[i][j] /= last;
  return true;
}

}  // namespace

extern "C" {

int ssrlcv_rectify_cameras_host(const ssrlcv_camera* left, const ssrlcv_camera* right, ssrlcv_rectification* out) {
  if (!left || !right || !out) return SSRLCV_ERR_INVALID_ARG;
  if (left->size.x != right->size.x || left->size.y != right->size.y || left->size.x == 0 || left->size.y == 0) return SSRLCV_ERR_INVALID_ARG;
  const ssrlcv_camera* cams[2] = {left, right};
  for (int i = 0; i < 2; ++i)
    if (!finite_positive((double)cams[i]->foc) || !finite_positive((double)cams[i]->fov.x)) return SSRLCV_ERR_INVALID_ARG;
  const double w = (double)left->size.x, h = (double)left->size.y;
  // 1, 2
  double f[2];
  M3 R[2];
  for (int i = 0; i < 2; ++i) {
    f[i] = camera_host::focal_pixels((double)cams[i]->foc, (double)cams[i]->fov.x, (double)cams[i]->size.x);
    if (!finite_positive(f[i])) return SSRLCV_ERR_INVALID_ARG;  // a field of view at a pole of tan
    R[i] = euler_matrix((double)cams[i]->cam_rot.x, (double)cams[i]->cam_rot.y, (double)cams[i]->cam_rot.z);
  }
  // 3
  const double b[3] = {(double)right->cam_pos.x - (double)left->cam_pos.x, (double)right->cam_pos.y - (double)left->cam_pos.y,
                       (double)right->cam_pos.z - (double)left->cam_pos.z};
  const double bn = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  if (!finite_positive(bn)) return SSRLCV_ERR_INVALID_ARG;
  const double xh[3] = {b[0] / bn, b[1] / bn, b[2] / bn};
  if (!(xh[0] * R[0].m[0][0] + xh[1] * R[0].m[1][0] + xh[2] * R[0].m[2][0] > 0.0)) return SSRLCV_ERR_INVALID_ARG;
  const double zs[3] = {R[0].m[0][2] + R[1].m[0][2], R[0].m[1][2] + R[1].m[1][2], R[0].m[2][2] + R[1].m[2][2]};
  double yh[3] = {zs[1] * xh[2] - zs[2] * xh[1], zs[2] * xh[0] - zs[0] * xh[2], zs[0] * xh[1] - zs[1] * xh[0]};
  const double yn = sqrt(yh[0] * yh[0] + yh[1] * yh[1] + yh[2] * yh[2]);
  if (!(yn >= 1e-6)) return SSRLCV_ERR_UNSUPPORTED;  // float32 angles resolve about 1e-7
  for (int i = 0; i < 3; ++i) yh[i] /= yn;
  const double zh[3] = {xh[1] * yh[2] - xh[2] * yh[1], xh[2] * yh[0] - xh[0] * yh[2], xh[0] * yh[1] - xh[1] * yh[0]};
  // 4: M = [xh yh zh] as columns
  const double m20 = xh[2] < -1.0 ? -1.0 : xh[2] > 1.0 ? 1.0 : xh[2];
  const float rot[3] = {(float)atan2(yh[2], zh[2]), (float)(-asin(m20)), (float)atan2(xh[1], xh[0])};
  const M3 Rn = euler_matrix((double)rot[0], (double)rot[1], (double)rot[2]);
  // 5
  double a[2][3];
  for (int i = 0; i < 2; ++i)
    for (int k = 0; k < 3; ++k) a[i][k] = Rn.m[0][k] * R[i].m[0][2] + Rn.m[1][k] * R[i].m[1][2] + Rn.m[2][k] * R[i].m[2][2];
  const double cos45 = 0.70710678118654752440;
  if (!(a[0][2] >= cos45) || !(a[1][2] >= cos45)) return SSRLCV_ERR_UNSUPPORTED;
  const double tl = rint(f[0] * a[0][0] / a[0][2]), tr = rint(f[0] * a[1][0] / a[1][2]);
  const double ty = rint(f[0] * (a[0][1] / a[0][2] + a[1][1] / a[1][2]) / 2.0);
  // 6
  const double t[2] = {tl, tr};
  M3 Hm[2], Gm[2];
  for (int i = 0; i < 2; ++i) {
    if (!compose(mul(transpose(R[i]), Rn), f[i], f[0], w / 2.0, h / 2.0, t[i], ty, Hm[i])) return SSRLCV_ERR_UNSUPPORTED;
    if (!inverse_normalised(Hm[i], Gm[i])) return SSRLCV_ERR_UNSUPPORTED;
  }
  // 7
  ssrlcv_rectification o;
  memset(&o, 0, sizeof o);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      o.Hl[3 * i + j] = (float)Hm[0].m[i][j];
      o.Hr[3 * i + j] = (float)Hm[1].m[i][j];
      o.Gl[3 * i + j] = (float)Gm[0].m[i][j];
      o.Gr[3 * i + j] = (float)Gm[1].m[i][j];
    }
  o.w = left->size.x;
  o.h = left->size.y;
  o.foc = (float)f[0];
  o.baseline = (float)bn;
  o.doffset = (float)(tl - tr);
  o.cx = (float)(w / 2.0 - tl);
  o.cy = (float)(h / 2.0 - ty);
  for (int i = 0; i < 3; ++i) o.cam_rot[i] = rot[i];
  *out = o;
  return SSRLCV_OK;
}

int ssrlcv_hip_warp_homography_u8(const uint8_t* src, uint32_t srcW, uint32_t srcH, const float* H_host, uint8_t* dst, uint32_t dstW,
                                  uint32_t dstH, ssrlcv_stream_t stream) {
  if (!H_host || srcW == 0 || srcH == 0 || bad_image(srcW, srcH) || bad_image(dstW, dstH)) return SSRLCV_ERR_INVALID_ARG;
  if (dstW == 0 || dstH == 0) return SSRLCV_OK;
  if (!src || !dst) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t lanesPerRow = (dstW + 3u) / 4u + 1u;  // the head and at most ceil(dstW / 4) groups
  const uint32_t items = lanesPerRow * dstH;           // below 2^29 + 2^25: dstW dstH < 2^31, dstH <= 2^24
  hipLaunchKernelGGL(k_warp_u8, dim3(capped_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, (int)srcW, (int)srcH, load_h(H_host), dst,
                     dstW, lanesPerRow, items);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_hip_stereo_mask_rectified(float* disparity, uint32_t* cost, uint32_t w, uint32_t h, uint32_t radius, const float* Hl_host,
                                     const float* Hr_host, uint32_t srcW, uint32_t srcH, ssrlcv_stream_t stream) {
  if (!Hl_host || !Hr_host || srcW == 0 || srcH == 0 || bad_image(srcW, srcH) || bad_image(w, h) || radius < 1 || radius > 15)
    return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!disparity) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t n = w * h;
  hipLaunchKernelGGL(k_stereo_mask, dim3(capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, disparity, cost, w, n, (int)radius,
                     load_h(Hl_host), load_h(Hr_host), (float)(srcW - 1), (float)(srcH - 1));
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_hip_matches_apply_homography(ssrlcv_match* matches, uint32_t n, const float* H0_host, const float* H1_host,
                                        ssrlcv_stream_t stream) {
  if (n == 0) return SSRLCV_OK;
  if (!matches) return SSRLCV_ERR_INVALID_ARG;
  if (!H0_host && !H1_host) return SSRLCV_OK;  // neither side moves
  hipLaunchKernelGGL(k_matches_homography, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, matches, n, load_h(H0_host),
                     load_h(H1_host), H0_host ? 1 : 0, H1_host ? 1 : 0);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
