// ssrlcv_amd/csrc/camera_host.h -- host arithmetic on Image::Camera records, in double: what ssrlcv_rectify_cameras_host
// (rectify.hip) and ssrlcv_dsm_ortho_view_host (ortho.hip) share, so that both read a camera the same way.
#pragma once
#include <math.h>

namespace camera_host {

// 3 x 3 double matrices, row-major
struct M3 {
  double m[3][3];
};
inline M3 mul(const M3& a, const M3& b) {
  M3 o;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return o;
}
inline M3 transpose(const M3& a) {
  M3 o;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.m[i][j] = a.m[j][i];
  return o;
}
// rotatePoint's matrix Rz(z) Ry(y) Rx(x)
inline M3 euler_matrix(double x, double y, double z) {
  const double cx = cos(x), sx = sin(x), cy = cos(y), sy = sin(y), cz = cos(z), sz = sin(z);
  M3 o = {{{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx}, {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx}, {-sy, cy * sx, cy * cx}}};
  return o;
}
inline bool finite_positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// the focal length in pixels, foc / dpix with dpix = foc tan(fov.x / 2) / (size.x / 2) ("rectification" builder, step 1)
inline double focal_pixels(double foc, double fovx, double sizex) {
  const double dpix = foc * tan(fovx / 2.0) / (sizex / 2.0);
  return foc / dpix;
}

}  // namespace camera_host
