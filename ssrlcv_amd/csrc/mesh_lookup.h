// ssrlcv_amd/csrc/mesh_lookup.h -- the MESH lookup of include/ssrlcv_hip.h "surface accuracy" item 1, its one definition: where a
// point of the frame lies in the reference's mesh, the plane of the triangle under it, and the difference to it.  accuracy.hip
// (k_dsm_difference) writes the difference; register.hip (k_register_terms) also needs the slopes of that triangle, which are the
// corner differences the plane was formed from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dsm_frame.h"

namespace dsm {

// (u, v, z) of a point in the frame (point_uvz; z finite) against the w x h map `height` triangulated by `cells`, pitch w - 1.
// True iff the point has a difference: it lies inside, the triangle under it was emitted and its plane's height r is finite; then
// d = z - r, and rs, rt are the chosen triangle's rise over one cell in s and in t, from the corner heights the plane read:
//   diagonal a-d   T0: rs = zd - zc, rt = zc - za      T1: rs = zb - za, rt = zd - zb
//   diagonal b-c   T0: rs = zb - za, rt = zc - za      T1: rs = zd - zc, rt = zd - zb
// Only the corners of the chosen triangle are read.
__device__ __forceinline__ bool mesh_difference(float u, float v, float z, const float* __restrict__ height, const uint8_t* __restrict__ cells, uint32_t w,
                                                uint32_t h, float& d, float& rs, float& rt) {
  if (w < 2u || h < 2u) return false;  // no cell of the mesh: no inside
  const float uu = u - 0.5f, vv = v - 0.5f;  // the mesh's vertices sit at cell centres
  const float fi = floorf(uu), fj = floorf(vv);
  if (!(fi >= 0.0f && fi < (float)(w - 1u) && fj >= 0.0f && fj < (float)(h - 1u))) return false;
  const uint32_t i = (uint32_t)fi, j = (uint32_t)fj;  // i <= w - 2, j <= h - 2: all four corners are cells of the map
  const float s = uu - fi, tt = vv - fj;
  const uint32_t byte = cells[j * (w - 1u) + i];
  const float* corner = height + (j * w + i);
  const float za = corner[0], zd = corner[w + 1u];  // a corner no emitted triangle names may be invalid: it is not used
  float r;
  bool emitted;
  if (!(byte & 4u)) {  // diagonal a-d: T0 = (a, c, d), T1 = (a, d, b)
    if (tt >= s) {
      const float zc = corner[w];
      emitted = byte & 1u;
      rs = zd - zc, rt = zc - za;
    } else {
      const float zb = corner[1];
      emitted = byte & 2u;
      rs = zb - za, rt = zd - zb;
    }
    r = za + ((s * rs) + (tt * rt));  // T0's contract order is (t rt) + (s rs): a float sum commutes
  } else {  // diagonal b-c: T0 = (a, c, b), T1 = (b, c, d)
    const float zb = corner[1], zc = corner[w];
    if (s + tt <= 1.0f) {
      emitted = byte & 1u;
      rs = zb - za, rt = zc - za;
      r = za + ((s * rs) + (tt * rt));
    } else {
      emitted = byte & 2u;
      rs = zd - zc, rt = zd - zb;
      r = zd + (((1.0f - s) * (zc - zd)) + ((1.0f - tt) * (zb - zd)));
    }
  }
  if (!emitted || !finite_bits(__float_as_uint(r))) return false;
  d = z - r;
  return true;
}

}  // namespace dsm
