// ssrlcv_amd/csrc/dsm.hip -- the surface model for gfx950: world-frame clouds rasterised into a height map on a ground grid, the
// maps of several pairs fused per cell, and the way back from cells to 3-D vertices in the mesh's numbering.  The contract is
// include/ssrlcv_hip.h "surface model"; tests/dsm_ref.py restates it.  A height map has the form of a disparity map (float[w h],
// pitch w, invalid = 0x7FC00000), so the median, speckle, fill and mesh calls take it unchanged.
//
//   k_dsm_scatter    a thread per point: the cell from a fixed-order float32 expression, then a 64-bit integer atomicMax on the
//                    cell's accumulator with (order key << 32) | (0xFFFFFFFF - index), the key complemented for MIN: the greatest
//                    (least) height wins, among equal keys the smallest index, whatever the arrival order.  0 = an empty cell: no
//                    index below UINT32_MAX packs to it.  The count map, if asked for, is an atomicAdd on a uint32.  Adjacent
//                    lanes of a wave that hold the same cell take their maximum and their number first and issue one of each.
//   k_dsm_unpack     a thread per cell: the accumulator back to the height's bits and the winner's index
//   k_dsm_fuse       a thread per cell: the valid entries of up to 8 maps as integer keys through the sorting network of the
//                    median filter; the spread test is one float subtraction; the result is one of the inputs
//   DsmKeep / DsmEmit + compact.h   the valid cells in raster order, each as ((origin + a ex) + b ey) + z ez
// Integer max and integer add commute, so the maps are bit-equal run to run; nothing is added up in floating point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "compact.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "order_key.h"

namespace {

using dsm::finite_bits;
using dsm::frame_ok;
using dsm::too_long_a_side;
using dsm::too_many_cells;

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kPerThread = 16;  // compact.h: a wave owns a run of 1024 elements, a block 4096

// the cell of a point and its height above the frame's plane; false for a point that is skipped or outside
__device__ __forceinline__ bool point_cell(const ssrlcv_float3& p, const ssrlcv_dsm_frame& f, uint32_t& cell, float& z) {
  float u, v;
  if (!dsm::point_uvz(p, f, u, v, z)) return false;
  const float fi = floorf(u), fj = floorf(v);
  // on floats, before any conversion: a NaN and a huge value are outside, -0 is cell 0
  if (!(fi >= 0.0f && fi < (float)f.w && fj >= 0.0f && fj < (float)f.h)) return false;
  if (!finite_bits(__float_as_uint(z))) return false;
  cell = (uint32_t)fj * f.w + (uint32_t)fi;  // below w h < 2^31
  return true;
}

// (order key << 32) | (0xFFFFFFFF - index): the unsigned order of the word is "higher (MIN: lower) first, then the smaller index"
__device__ __forceinline__ unsigned long long pack(float z, uint32_t index, uint32_t rule) {
  uint32_t key = (uint32_t)order_key(__float_as_uint(z)) ^ 0x80000000u;
  if (rule) key = ~key;
  return ((unsigned long long)key << 32) | (unsigned long long)(kNone - index);
}

__global__ __launch_bounds__(256) void k_dsm_scatter(const ssrlcv_float3* __restrict__ points, uint32_t n, ssrlcv_dsm_frame f, uint32_t rule,
                                                     unsigned long long* __restrict__ acc, uint32_t* __restrict__ count) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  uint32_t cell = kNone;
  float z = 0.0f;
  const bool in = t < n && point_cell(points[t], f, cell, z);
  // Lanes of a wave that hold the same cell merge over runs of adjacent lanes, and the last lane of a run issues the atomics: a
  // dense cloud arrives in the raster order of its image, so neighbouring lanes fall into the same cell.  Against one atomic a
  // point this took 0.09-0.7 of the time on the raster cloud, 1/64 on a one-cell grid and the same time on a shuffled cloud;
  // a plain load that skips a hopeless atomic won only on shuffled clouds without a count map (profiles/dsm_bench.txt).
  const unsigned lane = threadIdx.x & 63u;
  if (!in) cell = kNone;
  const uint32_t before = __shfl_up(cell, 1, 64), after = __shfl_down(cell, 1, 64);
  uint32_t start = (lane == 0u || before != cell) ? lane : 0u;  // the first lane of my run: a max-scan of the heads
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(start, o, 64);
    if (lane >= (unsigned)o) start = max(start, y);
  }
  unsigned long long best = in ? pack(z, t, rule) : 0ull;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(best, o, 64);
    if (lane >= start + (unsigned)o) best = max(best, y);
  }
  if (in && (lane == 63u || after != cell)) {
    atomicMax(acc + cell, best);
    if (count) atomicAdd(count + cell, lane - start + 1u);
  }
}

__global__ __launch_bounds__(256) void k_dsm_unpack(const unsigned long long* __restrict__ acc, uint32_t cells, uint32_t rule,
                                                    uint32_t* __restrict__ height, uint32_t* __restrict__ source) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= cells) return;
  const unsigned long long a = acc[c];
  uint32_t bits = kNaN, index = kNone;
  if (a != 0ull) {
    uint32_t key = (uint32_t)(a >> 32);
    if (rule) key = ~key;
    bits = (uint32_t)order_key(key ^ 0x80000000u);
    index = kNone - (uint32_t)a;
  }
  height[c] = bits;
  if (source) source[c] = index;
}

struct FuseMaps {
  const uint32_t* map[8];
};

__global__ __launch_bounds__(256) void k_dsm_fuse(FuseMaps maps, uint32_t m, uint32_t cells, uint32_t minViews, float maxSpread, uint32_t rule,
                                                  uint32_t* __restrict__ out, uint8_t* __restrict__ views) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= cells) return;
  int32_t a[8];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t bits = (uint32_t)k < m ? maps.map[k][c] : kNaN;
    const bool valid = bits != kNaN;
    n += valid ? 1 : 0;
    a[k] = valid ? order_key(bits) : INT32_MAX;
  }
  uint32_t result = kNaN;
  if (n > 0 && (uint32_t)n >= minViews) {
    sort_network<8>(a);  // the valid keys first: a key of INT32_MAX that is a value ties with the padding and sorts the same
    const int want = rule == 0u ? 0 : rule == 1u ? (n - 1) / 2 : n - 1;
    int32_t key = a[0], top = a[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      key = want == k ? a[k] : key;
      top = n - 1 == k ? a[k] : top;
    }
    const float lo = __uint_as_float((uint32_t)order_key((uint32_t)a[0])), hi = __uint_as_float((uint32_t)order_key((uint32_t)top));
    if (hi - lo <= maxSpread) result = (uint32_t)order_key((uint32_t)key);  // false for a NaN difference
  }
  out[c] = result;
  if (views) views[c] = (uint8_t)n;
}

struct DsmKeep {
  const uint32_t* height;
  __device__ uint32_t operator()(uint32_t c) const { return height[c] != kNaN ? 1u : 0u; }
};
struct DsmEmit {
  const float* height;
  ssrlcv_dsm_frame f;
  float* out;
  uint32_t capacity;
  __device__ void operator()(uint32_t c, int, uint32_t dst) const {
    if (dst >= capacity) return;
    const uint32_t j = c / f.w, i = c - j * f.w;
    const float a = ((float)i + 0.5f) * f.cell, b = ((float)j + 0.5f) * f.cell, z = height[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)dst * 3 + k] = ((f.origin[k] + (a * f.ex[k])) + (b * f.ey[k])) + (z * f.ez[k]);
  }
};

// ---- host side
size_t accumulator_bytes(uint32_t w, uint32_t h) { return align256((size_t)w * h * 8); }
size_t compaction_bytes(uint32_t n) { return align256(svc::workspace_words<1, kPerThread>(n) * 4); }
dim3 blocks_for(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

extern "C" {

size_t ssrlcv_hip_dsm_rasterize_workspace_bytes(uint32_t w, uint32_t h) {
  if (too_many_cells(w, h) || too_long_a_side(w, h)) return 0;
  return accumulator_bytes(w, h);
}

int ssrlcv_hip_dsm_rasterize(const ssrlcv_float3* points, uint32_t n, const ssrlcv_dsm_frame* frame, uint32_t rule, float* height, uint32_t* source,
                             uint32_t* count, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!frame_ok(frame) || rule > 1u) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t w = frame->w, h = frame->h;
  if (too_many_cells(w, h) || n == kNone) return SSRLCV_ERR_INVALID_ARG;
  if (too_long_a_side(w, h)) return SSRLCV_ERR_UNSUPPORTED;
  const uint32_t cells = w * h;
  if (cells == 0) return SSRLCV_OK;  // an empty grid: no map has an entry
  if (!height || !workspace || (!points && n != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < accumulator_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)workspace;
  SSRLCV_HIP_TRY(hipMemsetAsync(acc, 0, (size_t)cells * 8, st));
  if (count) SSRLCV_HIP_TRY(hipMemsetAsync(count, 0, (size_t)cells * 4, st));
  if (n) {
    hipLaunchKernelGGL(k_dsm_scatter, blocks_for(n), dim3(256), 0, st, points, n, *frame, rule, acc, count);
    SSRLCV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_dsm_unpack, blocks_for(cells), dim3(256), 0, st, acc, cells, rule, (uint32_t*)height, source);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_hip_dsm_fuse(const float* const* maps, uint32_t m, uint32_t w, uint32_t h, uint32_t minViews, float maxSpread, uint32_t rule, float* out,
                        uint8_t* views, ssrlcv_stream_t stream) {
  if (m == 0 || m > 8u || minViews == 0 || minViews > m || !(maxSpread >= 0.0f) || rule > 2u) return SSRLCV_ERR_INVALID_ARG;
  if (too_many_cells(w, h)) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t cells = w * h;
  if (cells == 0) return SSRLCV_OK;
  if (!maps || !out) return SSRLCV_ERR_INVALID_ARG;
  FuseMaps dev{};
  for (uint32_t k = 0; k < m; ++k) {
    if (!maps[k] || maps[k] == out) return SSRLCV_ERR_INVALID_ARG;
    dev.map[k] = (const uint32_t*)maps[k];
  }
  hipLaunchKernelGGL(k_dsm_fuse, blocks_for(cells), dim3(256), 0, (hipStream_t)stream, dev, m, cells, minViews, maxSpread, rule, (uint32_t*)out, views);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_dsm_points_workspace_bytes(uint32_t w, uint32_t h) {
  if (too_many_cells(w, h) || too_long_a_side(w, h)) return 0;
  return compaction_bytes(w * h);
}

int ssrlcv_hip_dsm_points(const float* height, const ssrlcv_dsm_frame* frame, ssrlcv_float3* out, uint32_t capacity, uint32_t* count_dev, void* workspace,
                          size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!frame_ok(frame) || too_many_cells(frame->w, frame->h)) return SSRLCV_ERR_INVALID_ARG;
  if (too_long_a_side(frame->w, frame->h)) return SSRLCV_ERR_UNSUPPORTED;
  if (!count_dev) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t cells = frame->w * frame->h;
  const hipStream_t st = (hipStream_t)stream;
  if (cells == 0) {  // an empty grid: no vertex, and nothing else is looked at
    SSRLCV_HIP_TRY(hipMemsetAsync(count_dev, 0, 4, st));
    return SSRLCV_OK;
  }
  if (!height || !workspace || (!out && capacity != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < compaction_bytes(cells)) return SSRLCV_ERR_WORKSPACE;
  DsmKeep keep{(const uint32_t*)height};
  DsmEmit emit{height, *frame, (float*)out, capacity};
  uint32_t* totals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(cells, keep, emit, (uint32_t*)workspace, &totals, st)));
  SSRLCV_HIP_TRY(hipMemcpyAsync(count_dev, totals + 1, 4, hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

}  // extern "C"
