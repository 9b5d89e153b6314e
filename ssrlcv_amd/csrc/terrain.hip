// ssrlcv_amd/csrc/terrain.hip -- grey-scale morphology of a height map, the progressive morphological ground filter on top of it
// and the map - map difference, for gfx950.  The contract is include/ssrlcv_hip.h "terrain filter"; tests/terrain_ref.py restates
// it.  Erosion and dilation are selections in the total order of "disparity post-filters" item 4: the output bits are input bits
// or the invalid pattern, so the kernels are held to the restatement bit for bit.
//
// A square window is separable: a row pass, then a column pass.  Each is a running minimum in van Herk / Gil-Werman form: the
// line is cut into segments of L = 2r + 1 cells, g is the running minimum from a segment's start, h the one back from its end,
// and the window [lo, lo + 2r] is h(lo) and, where it reaches the next segment, g(lo + 2r).  The work a cell is the same at every
// radius.  The first r cells of a line have a window clipped at its start: g of segment 0 alone.
//
//   keys           the keys of the valid values fill the int32 range but for one, the key of the invalid pattern, so no sentinel
//                  is free.  encode<kMax> closes that gap and leaves INT32_MAX as "no valid cell"; a dilation runs on the
//                  complement of its gap-closed key, so every pass is a minimum.
//   k_rows         a wave a row, 64 cells a step: g by a segmented scan over the lanes with a carry from the chunk before, stored;
//                  then the chunks backwards for h, each lane emitting the cell r ahead of it.  bits -> encoded keys
//   k_cols         a lane a column, a thread a segment of it: h down the segment into a scratch map, then up the segment with g of
//                  the next segment in a register, rows coalesced over the lanes.  The thread of segment 0 also emits the first r
//                  rows.  encoded keys -> bits, through an epilogue: plain, masked (OPEN and CLOSE keep holes) or the
//                  classification of the terrain call, which has Z_{k-1}(p) at hand
//   k_direct       radii 1 .. 8: both passes in one launch, a 64 x 16 tile and its halo of r cells in LDS as keys, the 2r + 1 taps
//                  of a row, then the 2r + 1 row minima of a column, through the same epilogues.  Bit-equal to the running minima
//                  by construction and 3 to 6 x faster at every one of these radii (profiles/terrain_bench.txt); its source and the
//                  epilogue's outputs are different maps
//   k_subtract     a thread a cell
// Every output word has one writer; a thread reads scratch words that it or its own wave wrote: no atomics, no block waits for
// another, bit-equal run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"
#include "order_key.h"

namespace svterrain {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr int32_t kInvKey = 0x7FC00000;  // order_key(kNaN): the one key no valid value has
constexpr int32_t kNothing = INT32_MAX;  // no valid cell

// of unsigned values: the unqualified min and max of two uint32_t pick the int overloads on the host, where UINT32_MAX is -1
__host__ __device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// the gap-closed key of a cell for a minimum (erosion) or, complemented, for a maximum (dilation)
template <bool kMax>
__device__ __forceinline__ int32_t encode(uint32_t bits) {
  if (bits == kNaN) return kNothing;
  const int32_t k = order_key(bits);
  return kMax ? ~(k + (k < kInvKey ? 1 : 0)) : k - (k > kInvKey ? 1 : 0);  // never INT32_MAX: k + 1 is never INT32_MIN
}
template <bool kMax>
__device__ __forceinline__ uint32_t decode(int32_t e) {
  if (e == kNothing) return kNaN;
  const int32_t c = kMax ? ~e : e;
  const int32_t k = kMax ? c - (c <= kInvKey ? 1 : 0) : c + (c >= kInvKey ? 1 : 0);
  return (uint32_t)order_key((uint32_t)k);
}

// ---- rows: grid (ceil(h / 4)), a wave a row
template <bool kMax>
__global__ __launch_bounds__(256) void k_rows(const uint32_t* __restrict__ in, int32_t* g, int32_t* __restrict__ out, uint32_t w, uint32_t h,
                                              uint32_t r) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t y = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (y >= h) return;  // the whole wave
  const uint32_t* src = in + y * w;
  int32_t* grow = g + y * w;
  int32_t* dst = out + y * w;
  const uint32_t L = 2u * r + 1u;  // r <= w - 1 < 2^31
  int32_t carry = kNothing;        // g of the cell before the chunk
  for (uint32_t base = 0; base < w; base += 64u) {  // w < 2^31: base + 64 cannot wrap
    const uint32_t x = base + lane;
    const uint32_t m = x % L;  // cells between the segment's start and x
    int32_t v = x < w ? encode<kMax>(src[x]) : kNothing;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const int32_t t = __shfl_up(v, d);
      if (lane >= d && m >= d) v = min(v, t);
    }
    if (m > lane) v = min(v, carry);  // the segment began before the chunk
    if (x < w) grow[x] = v;
    carry = __shfl(v, 63);
  }
  __threadfence();  // the wave reads below what its other lanes stored above
  carry = kNothing;  // h of the cell behind the chunk
  const uint32_t last = (w - 1u) & ~63u;
  for (uint32_t base = last;; base -= 64u) {
    const uint32_t x = base + lane;
    const uint32_t m = x % L;
    const uint32_t toEnd = x < w ? umin(2u * r - m, w - 1u - x) : 0u;  // cells between x and its segment's end, clipped at the row's
    int32_t v = x < w ? encode<kMax>(src[x]) : kNothing;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const int32_t t = __shfl_down(v, d);
      if (lane + d < 64u && toEnd >= d) v = min(v, t);
    }
    if (toEnd > 63u - lane) v = min(v, carry);  // the segment ends behind the chunk
    carry = __shfl(v, 0);
    if (x < w && w - 1u - x >= r) {  // the window [x, x + 2r] of the cell x + r, clipped at the row's end
      const uint32_t rest = w - 1u - x;
      if (m > 0u && rest > 2u * r - m) v = min(v, grow[rest < 2u * r ? w - 1u : x + 2u * r]);  // it reaches the next segment
      dst[x + r] = v;
    }
    if (base == 0) break;
  }
  for (uint32_t x = lane; x < r; x += 64u) dst[x] = grow[umin(x + r, w - 1u)];  // windows clipped at the row's start: inside segment 0
}

// ---- columns: grid (ceil(w / 256), min(segments, 65535))
struct Plain {
  uint32_t* out;
  __device__ __forceinline__ void operator()(size_t p, uint32_t bits) const { out[p] = bits; }
};
struct Masked {  // OPEN and CLOSE: a hole stays a hole
  uint32_t* out;
  const uint32_t* __restrict__ in;
  __device__ __forceinline__ void operator()(size_t p, uint32_t bits) const { out[p] = in[p] == kNaN ? kNaN : bits; }
};
struct Classify {  // level k of the terrain call: Z_k, and what d = Z_{k-1}(p) - O_k(p) > threshold flags
  const uint32_t* zPrev;  // Z_{k-1}; may be z: a cell is read and then written by one thread
  uint32_t* z;
  uint32_t* terrain;
  uint8_t* level;    // may be NULL
  uint32_t* opened;  // NULL but at the last level
  float threshold;
  uint32_t k;  // 1 ..
  __device__ __forceinline__ void operator()(size_t p, uint32_t bits) const {
    const uint32_t before = zPrev[p];
    const bool valid = before != kNaN;  // Z_{k-1} is valid exactly where the height is
    const uint32_t o = valid ? bits : kNaN;
    z[p] = o;
    if (opened) opened[p] = o;
    const bool flagged = valid && __uint_as_float(before) - __uint_as_float(o) > threshold;  // false for a NaN difference
    if (k == 1u) {
      terrain[p] = flagged ? kNaN : before;  // Z_0 is the height
      if (level) level[p] = !valid ? (uint8_t)255 : flagged ? (uint8_t)1 : (uint8_t)0;
    } else if (flagged) {
      terrain[p] = kNaN;
      if (level && level[p] == 0) level[p] = (uint8_t)k;
    }
  }
};

template <bool kMax, typename Epi>
__global__ __launch_bounds__(256) void k_cols(const int32_t* __restrict__ in, int32_t* hmap, uint32_t w, uint32_t h, uint32_t r, uint32_t segments,
                                              Epi epi) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= w) return;
  const uint32_t L = 2u * r + 1u;  // r <= h - 1 < 2^31
  for (uint32_t s = blockIdx.y; s < segments; s += gridDim.y) {
    const uint32_t y0 = s * L;  // below h
    const uint32_t e = h - 1u - y0 < 2u * r ? h - 1u : y0 + 2u * r;  // the segment's end, clipped at the column's
    int32_t run = kNothing;
    for (uint32_t y = e;; --y) {  // h, down to the segment's start
      run = min(run, in[(size_t)y * w + x]);
      hmap[(size_t)y * w + x] = run;
      if (y == y0) break;
    }
    run = kNothing;    // g of the next segment: the rows (e, top]
    uint32_t top = e;  // the window of the segment's first row ends at e
    for (uint32_t lo = y0; lo <= e && h - 1u - lo >= r; ++lo) {  // the window [lo, lo + 2r] of row lo + r, clipped at the column's end
      const uint32_t hi = h - 1u - lo < 2u * r ? h - 1u : lo + 2u * r;
      if (top < hi) run = min(run, in[(size_t)(++top) * w + x]);  // hi grows by one row a step at most
      epi((size_t)(lo + r) * w + x, decode<kMax>(min(hmap[(size_t)lo * w + x], run)));
    }
    if (s == 0u && r > 0u) {  // windows clipped at the column's start: g of segment 0, rows [0, min(y + r, h - 1)]
      run = kNothing;
      for (uint32_t y = 0; y <= r; ++y) run = min(run, in[(size_t)y * w + x]);  // r <= h - 1
      for (uint32_t y = 0; y < r; ++y) {
        epi((size_t)y * w + x, decode<kMax>(run));
        if (y + r + 1u < h) run = min(run, in[(size_t)(y + r + 1u) * w + x]);
      }
    }
  }
}

// ---- small radii: grid (tiles of 64 x 16 cells), R the radius itself; a cell outside the map is "nothing", which is the clipped window
constexpr uint32_t kDirectMaxRadius = 8;
template <bool kMax, int R, typename Epi>
__global__ __launch_bounds__(256) void k_direct(const uint32_t* __restrict__ in, uint32_t w, uint32_t h, uint32_t tilesX, Epi epi) {
  constexpr int TX = 64, TY = 16, SW = TX + 2 * R, SH = TY + 2 * R;
  __shared__ int32_t tile[SH][SW];
  __shared__ int32_t rows[SH][TX];
  const uint32_t tx0 = (blockIdx.x % tilesX) * TX, ty0 = (blockIdx.x / tilesX) * TY;
  for (int i = threadIdx.x; i < SH * SW; i += 256) {
    const int sy = i / SW, sx = i - sy * SW;
    const uint32_t gx = tx0 + (uint32_t)sx - (uint32_t)R, gy = ty0 + (uint32_t)sy - (uint32_t)R;  // left of and above the map they wrap above w and h
    tile[sy][sx] = (gx < w && gy < h) ? encode<kMax>(in[(size_t)gy * w + gx]) : kNothing;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH * TX; i += 256) {
    const int sy = i / TX, sx = i - sy * TX;
    int32_t m = tile[sy][sx];
#pragma unroll
    for (int d = 1; d <= 2 * R; ++d) m = min(m, tile[sy][sx + d]);
    rows[sy][sx] = m;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ly = ly0 + j;
    const uint32_t gx = tx0 + lx, gy = ty0 + ly;
    if (gx >= w || gy >= h) continue;
    int32_t m = rows[ly][lx];
#pragma unroll
    for (int d = 1; d <= 2 * R; ++d) m = min(m, rows[ly + d][lx]);
    epi((size_t)gy * w + gx, decode<kMax>(m));
  }
}

__global__ __launch_bounds__(256) void k_subtract(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {  // n < 2^31 and at most 2^24 threads: p cannot wrap
    const uint32_t ua = a[p], ub = b[p];
    const float d = __uint_as_float(ua) - __uint_as_float(ub);
    out[p] = (ua == kNaN || ub == kNaN || d != d) ? kNaN : __float_as_uint(d);  // a difference that is a number never has the invalid bits
  }
}

// ---- host side
inline bool size_invalid(uint32_t w, uint32_t h) { return (unsigned long long)w * h >= (1ull << 31); }
inline size_t map_bytes(uint32_t w, uint32_t h) { return align256((size_t)4 * w * h); }
inline uint32_t effective_radius(uint32_t radius, uint32_t w, uint32_t h) { return umin(radius, umax(w, h) - 1u); }

// one erosion (kMax false) or dilation of the non-empty map `src`: rows into `rowOut`, columns through the epilogue; `scratch`
// holds g of the rows and then h of the columns
template <bool kMax, typename Epi>
inline hipError_t erode_launch(const uint32_t* src, int32_t* rowOut, int32_t* scratch, uint32_t w, uint32_t h, uint32_t radius, Epi epi, hipStream_t st) {
  const uint32_t rx = umin(radius, w - 1u), ry = umin(radius, h - 1u);  // a window clipped at the map is the window of the smaller radius
  hipLaunchKernelGGL(k_rows<kMax>, dim3((h + 3u) / 4u), dim3(256), 0, st, src, scratch, rowOut, w, h, rx);
  const uint32_t segments = (h - 1u) / (2u * ry + 1u) + 1u;
  hipLaunchKernelGGL((k_cols<kMax, Epi>), dim3((w + 255u) / 256u, umin(segments, 65535u)), dim3(256), 0, st, rowOut, scratch, w, h, ry, segments, epi);
  return hipGetLastError();
}

// the same for 1 <= radius <= kDirectMaxRadius in one launch; `src` is none of the maps the epilogue writes
template <bool kMax, typename Epi>
inline hipError_t direct_launch(const uint32_t* src, uint32_t w, uint32_t h, uint32_t radius, Epi epi, hipStream_t st) {
  const uint32_t tilesX = (w + 63u) / 64u;
  const dim3 grid(tilesX * ((h + 15u) / 16u));  // w h < 2^31: below 2^21 + 2^25 tiles
  switch (radius) {
#define SSRLCV_DIRECT_CASE(R) \
  case R: hipLaunchKernelGGL((k_direct<kMax, R, Epi>), grid, dim3(256), 0, st, src, w, h, tilesX, epi); break;
    SSRLCV_DIRECT_CASE(1) SSRLCV_DIRECT_CASE(2) SSRLCV_DIRECT_CASE(3) SSRLCV_DIRECT_CASE(4)
    SSRLCV_DIRECT_CASE(5) SSRLCV_DIRECT_CASE(6) SSRLCV_DIRECT_CASE(7) SSRLCV_DIRECT_CASE(8)
#undef SSRLCV_DIRECT_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
inline bool is_direct(uint32_t radius) { return radius >= 1u && radius <= kDirectMaxRadius; }

inline bool bad_terrain_params(const ssrlcv_terrain_params* p) {
  if (!p || p->levels == 0 || p->levels > 8) return true;
  for (uint32_t k = 0; k < p->levels; ++k) {
    if (p->radius[k] == 0 || (k > 0 && p->radius[k] <= p->radius[k - 1])) return true;
    if (!(p->threshold[k] >= 0.0f && p->threshold[k] <= 3.4028234663852886e38f)) return true;
  }
  return false;
}

}  // namespace svterrain

#ifndef SSRLCV_TERRAIN_LAB
extern "C" {

size_t ssrlcv_hip_dsm_morphology_workspace_bytes(uint32_t w, uint32_t h) {
  using namespace svterrain;
  if (size_invalid(w, h) || w == 0 || h == 0) return 0;
  return 2 * map_bytes(w, h);
}

int ssrlcv_hip_dsm_morphology(const float* in, float* out, uint32_t w, uint32_t h, uint32_t radius, uint32_t op, void* workspace, size_t workspaceBytes,
                              ssrlcv_stream_t stream) {
  using namespace svterrain;
  if (op > 3 || radius == 0) return SSRLCV_ERR_INVALID_ARG;
  if (size_invalid(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!in || !out || !workspace || in == out) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_dsm_morphology_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t r = effective_radius(radius, w, h);
  const uint32_t* src = (const uint32_t*)in;
  uint32_t* dst = (uint32_t*)out;
  int32_t* rows = (int32_t*)workspace;
  int32_t* scratch = (int32_t*)((char*)workspace + map_bytes(w, h));
  if (is_direct(r)) {  // one launch a pass; the first result of an OPEN or CLOSE waits in the workspace
    uint32_t* first = (uint32_t*)workspace;
    switch (op) {
      case SSRLCV_MORPH_ERODE: SSRLCV_HIP_TRY((direct_launch<false>(src, w, h, r, Plain{dst}, st))); break;
      case SSRLCV_MORPH_DILATE: SSRLCV_HIP_TRY((direct_launch<true>(src, w, h, r, Plain{dst}, st))); break;
      case SSRLCV_MORPH_OPEN:
        SSRLCV_HIP_TRY((direct_launch<false>(src, w, h, r, Plain{first}, st)));
        SSRLCV_HIP_TRY((direct_launch<true>(first, w, h, r, Masked{dst, src}, st)));
        break;
      default:
        SSRLCV_HIP_TRY((direct_launch<true>(src, w, h, r, Plain{first}, st)));
        SSRLCV_HIP_TRY((direct_launch<false>(first, w, h, r, Masked{dst, src}, st)));
        break;
    }
    return SSRLCV_OK;
  }
  switch (op) {
    case SSRLCV_MORPH_ERODE: SSRLCV_HIP_TRY((erode_launch<false>(src, rows, scratch, w, h, r, Plain{dst}, st))); break;
    case SSRLCV_MORPH_DILATE: SSRLCV_HIP_TRY((erode_launch<true>(src, rows, scratch, w, h, r, Plain{dst}, st))); break;
    case SSRLCV_MORPH_OPEN:  // the first result waits in `out`, which nothing else touches before the last pass writes every cell
      SSRLCV_HIP_TRY((erode_launch<false>(src, rows, scratch, w, h, r, Plain{dst}, st)));
      SSRLCV_HIP_TRY((erode_launch<true>(dst, rows, scratch, w, h, r, Masked{dst, src}, st)));
      break;
    default:
      SSRLCV_HIP_TRY((erode_launch<true>(src, rows, scratch, w, h, r, Plain{dst}, st)));
      SSRLCV_HIP_TRY((erode_launch<false>(dst, rows, scratch, w, h, r, Masked{dst, src}, st)));
      break;
  }
  return SSRLCV_OK;
}

size_t ssrlcv_hip_dsm_terrain_workspace_bytes(uint32_t w, uint32_t h) {
  using namespace svterrain;
  if (size_invalid(w, h) || w == 0 || h == 0) return 0;
  return 4 * map_bytes(w, h);
}

int ssrlcv_hip_dsm_terrain(const float* height, uint32_t w, uint32_t h, const ssrlcv_terrain_params* params, float* terrain, uint8_t* level, float* opened,
                           void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  using namespace svterrain;
  if (bad_terrain_params(params)) return SSRLCV_ERR_INVALID_ARG;
  if (size_invalid(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!height || !terrain || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_dsm_terrain_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const size_t map = map_bytes(w, h);
  uint32_t* z = (uint32_t*)workspace;  // Z_{k-1}, then Z_k
  uint32_t* eroded = (uint32_t*)((char*)workspace + map);
  int32_t* rows = (int32_t*)((char*)workspace + 2 * map);
  int32_t* scratch = (int32_t*)((char*)workspace + 3 * map);
  for (uint32_t k = 1; k <= params->levels; ++k) {
    const uint32_t r = effective_radius(params->radius[k - 1], w, h);
    const uint32_t* zPrev = k == 1 ? (const uint32_t*)height : z;
    const Classify classify{zPrev, z, (uint32_t*)terrain, level, k == params->levels ? (uint32_t*)opened : nullptr, params->threshold[k - 1], k};
    if (is_direct(r)) {  // the dilation reads the erosion alone; the classification reads and writes cell p of its other maps
      SSRLCV_HIP_TRY((direct_launch<false>(zPrev, w, h, r, Plain{eroded}, st)));
      SSRLCV_HIP_TRY((direct_launch<true>(eroded, w, h, r, classify, st)));
    } else {
      SSRLCV_HIP_TRY((erode_launch<false>(zPrev, rows, scratch, w, h, r, Plain{eroded}, st)));
      SSRLCV_HIP_TRY((erode_launch<true>(eroded, rows, scratch, w, h, r, classify, st)));
    }
  }
  return SSRLCV_OK;
}

int ssrlcv_hip_dsm_subtract(const float* a, const float* b, uint32_t w, uint32_t h, float* out, ssrlcv_stream_t stream) {
  using namespace svterrain;
  if (size_invalid(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!a || !b || !out) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t n = w * h;
  hipLaunchKernelGGL(k_subtract, dim3(umin((n + 255u) / 256u, 65536u)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)a, (const uint32_t*)b,
                     (uint32_t*)out, n);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
#endif
