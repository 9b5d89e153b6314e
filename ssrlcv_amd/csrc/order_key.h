// ssrlcv_amd/csrc/order_key.h -- the float order as an integer order, and a sorting network over such keys in registers: the
// median and hole-filling kernels of disparity_filter.hip and the surface model of dsm.hip select by rank with them
// (include/ssrlcv_hip.h "disparity post-filters" item 4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int32_t order_key(uint32_t bits) {  // the float order as an integer order, total, -0 below +0
  const int32_t b = (int32_t)bits;
  return b >= 0 ? b : b ^ 0x7FFFFFFF;  // its own inverse
}

__device__ __forceinline__ void compare_exchange(int32_t& a, int32_t& b) {
  const int32_t lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

// Batcher's odd-even merge sort of N = 2^k registers: every index is a compile-time constant once the loops are unrolled, and
// the exchanges with the constant INT32_MAX entries behind the window's (2M + 1)^2 fold away
template <int N>
__device__ __forceinline__ void sort_network(int32_t (&a)[N]) {
#pragma unroll
  for (int lp = 0; (1 << lp) < N; ++lp) {
    const int p = 1 << lp;
#pragma unroll
    for (int lk = lp; lk >= 0; --lk) {
      const int k = 1 << lk;
#pragma unroll
      for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p)) compare_exchange(a[i + j], a[i + j + k]);
        }
      }
    }
  }
}
