// ssrlcv_amd/csrc/dsm_frame.h -- what the calls on a ground grid share on the host (include/ssrlcv_hip.h "surface model" frame and
// refusals): dsm.hip and ortho.hip refuse the same frames and the same sizes.
#pragma once
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

inline bool too_many_cells(uint32_t w, uint32_t h) { return (unsigned long long)w * h >= (1ull << 31); }
inline bool too_long_a_side(uint32_t w, uint32_t h) { return w > kMaxSide || h > kMaxSide; }

}  // namespace dsm
