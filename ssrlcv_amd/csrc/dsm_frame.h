// ssrlcv_amd/csrc/dsm_frame.h -- what the calls on a ground grid share on the host (include/ssrlcv_hip.h "surface model" frame and
// refusals): dsm.hip, ortho.hip, accuracy.hip and register.hip refuse the same frames and the same sizes, and dsm.hip,
// accuracy.hip and register.hip place a point in the frame with the same expression.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssrlcv_hip.h"

namespace dsm {

constexpr uint32_t kMaxSide = 1u << 24;  // (float)w is exact up to here

__host__ __device__ __forceinline__ bool finite_bits(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

inline bool finite_host(float v) {
  uint32_t bits;
  __builtin_memcpy(&bits, &v, 4);
  return finite_bits(bits);
}

inline bool frame_ok(const ssrlcv_dsm_frame* f) {
  if (!f) return false;
  for (int k = 0; k < 3; ++k)
    if (!finite_host(f->origin[k]) || !finite_host(f->ex[k]) || !finite_host(f->ey[k]) || !finite_host(f->ez[k])) return false;
  return finite_host(f->cell) && f->cell > 0.0f;
}

// a . e in the contract's order: ((q.x e.x) + (q.y e.y)) + (q.z e.z)
__device__ __forceinline__ float along(float qx, float qy, float qz, const float (&e)[3]) { return ((qx * e[0]) + (qy * e[1])) + (qz * e[2]); }

// "surface model" item 1 up to u, v and z: false for a point that is skipped (a non-finite component, or (0, 0, 0) with either
// sign of zero).  Whether z is finite and where (u, v) lies is the caller's test.
__device__ __forceinline__ bool point_uvz(const ssrlcv_float3& p, const ssrlcv_dsm_frame& f, float& u, float& v, float& z) {
  const uint32_t bx = __float_as_uint(p.x), by = __float_as_uint(p.y), bz = __float_as_uint(p.z);
  if (!finite_bits(bx) || !finite_bits(by) || !finite_bits(bz)) return false;
  if (((bx | by | bz) & 0x7FFFFFFFu) == 0u) return false;  // (0, 0, 0), either sign: "no result"
  const float qx = p.x - f.origin[0], qy = p.y - f.origin[1], qz = p.z - f.origin[2];
  u = __fdiv_rn(along(qx, qy, qz, f.ex), f.cell);
  v = __fdiv_rn(along(qx, qy, qz, f.ey), f.cell);
  z = along(qx, qy, qz, f.ez);
  return true;
}

inline bool too_many_cells(uint32_t w, uint32_t h) { return (unsigned long long)w * h >= (1ull << 31); }
inline bool too_long_a_side(uint32_t w, uint32_t h) { return w > kMaxSide || h > kMaxSide; }

}  // namespace dsm
