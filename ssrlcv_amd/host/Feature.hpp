// ssrlcv_amd/host/Feature.hpp -- Feature<D> and SIFT_Descriptor (include/Feature.cuh:31-94, src/Feature.cu:7-42).
#pragma once
#include <cfloat>
#include "cuda_vec_types.hpp"
#include "ssrlcv_types.h"

namespace ssrlcv {

template <typename D>
struct Feature {
  int parent;    ///< parent image ID
  float2 loc;    ///< location on parent image
  D descriptor;  ///< descriptor of feature
  Feature() : parent(-1), loc{-1.0f, -1.0f} {}
  Feature(float2 loc) : parent(-1), loc(loc) {}
  Feature(float2 loc, D descriptor) : parent(-1), loc(loc), descriptor(descriptor) {}
};

struct SIFT_Descriptor {
  float sigma;
  float theta;
  unsigned char values[128];
  SIFT_Descriptor() : sigma(0.0f), theta(0.0f) {}
  SIFT_Descriptor(float theta) : sigma(0.0f), theta(theta) {}
  SIFT_Descriptor(float theta, unsigned char v[128]) : sigma(0.0f), theta(theta) {
    for (int i = 0; i < 128; ++i) values[i] = v[i];
  }
  // squared L2 with early exit (src/Feature.cu:36-42); host-side helper for tests and the reference's comparators
  float distProtocol(const SIFT_Descriptor& b, const float& bestMatch = FLT_MAX) const {
    float dist = 0.0f;
    for (int i = 0; i < 128 && dist < bestMatch; ++i)
      dist += ((float)values[i] - b.values[i]) * ((float)values[i] - b.values[i]);
    return dist;
  }
};

static_assert(sizeof(Feature<SIFT_Descriptor>) == sizeof(ssrlcv_sift_feature), "Feature<SIFT_Descriptor> must be 152 B");

// Window_3x3 ... Window_31x31: a square of pixels around a location, compared by the sum of absolute differences.  Host-side
// types with a host helper, like SIFT_Descriptor's: the dense-stereo kernels (DisparityFactory.hpp, csrc/stereo.hip) never
// materialise a window -- they work from the two images directly -- so no device array of these exists.
template <int N>
struct Window_NxN {
  unsigned char values[N][N];
  Window_NxN() {
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) values[y][x] = 0;
  }
  // sum of absolute differences with early exit; exact in float (at most 961 * 255 < 2^24)
  float distProtocol(const Window_NxN<N>& b, const float& bestMatch = FLT_MAX) const {
    float dist = 0.0f;
    for (int y = 0; y < N && dist < bestMatch; ++y)
      for (int x = 0; x < N; ++x) dist += values[y][x] > b.values[y][x] ? (float)(values[y][x] - b.values[y][x]) : (float)(b.values[y][x] - values[y][x]);
    return dist;
  }
};
typedef Window_NxN<3> Window_3x3;
typedef Window_NxN<9> Window_9x9;
typedef Window_NxN<15> Window_15x15;
typedef Window_NxN<25> Window_25x25;
typedef Window_NxN<31> Window_31x31;
static_assert(sizeof(Window_3x3) == 9 && sizeof(Window_9x9) == 81 && sizeof(Window_15x15) == 225 && sizeof(Window_25x25) == 625 &&
              sizeof(Window_31x31) == 961, "Window_NxN holds N x N bytes");

}  // namespace ssrlcv
