// ssrlcv_amd/csrc/shift.hip -- the coarse shift search between two height maps of one grid, for gfx950.  The contract is
// include/ssrlcv_hip.h "shift search"; tests/shift_ref.py restates it.  Per shift of a (2S + 1)^2 window the table holds the
// count, the sum and the sum of squares of the quantised height differences: integers, so the order of summation does not
// matter and the kernels are held to the restatement byte for byte.
//
//   k_quantise     a thread a sampled cell of both maps: float -> int32 key, INT32_MIN for an invalid cell, which no key can be
//                  (|q| <= 65536).  The stride disappears here.  The four head counts are ballots summed per wave over its
//                  trips and added once a wave: integer atomics.
//   k_search<K>    lanes own shifts, not cells.  A block stages a 64 x 16 tile of moving keys and the reference tile with a halo
//                  of S cells on every side; cells outside the grid are the sentinel.  Slot e = thread + 256 k, k < K, is the
//                  shift of entry e; its reference word for the moving cell (mx, my) is rt[base(e) + my RW + mx], base(e) =
//                  (e / L) RW + e % L, so lanes of consecutive kx read consecutive words, and RW = 65 + 2S keeps the lanes of a
//                  half-wave that sit in different rows of the window on different banks (two such lanes are 64 r + j words
//                  apart, 0 < j < 32).  The moving key is one LDS word for the whole wave; an invalid one skips the cell for the
//                  whole wave.  Per pair: one subtraction, ONE unsigned compare that is the sentinel test and the gate test at
//                  once (see `pair`), a select, two adds and a 64-bit multiply-add.  n, sum and sumSq stay in registers over all
//                  the tiles of the block; sum has an int32 partial a tile.  Up to 128 shifts the waves that own no shift split the
//                  tile's rows instead.  At the end each (thread, shift) adds once into the table: 64-bit integer atomics.
// No float atomics, no cross-lane reduction, no block waits for another: bit-equal run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"

namespace svshift {

constexpr int32_t kInvalid = INT32_MIN;
constexpr uint32_t kMaxRadius = 32;
constexpr int32_t kMaxCenter = 1 << 24, kMaxCenterQ = 1 << 18;
constexpr uint32_t kMaxSide = 1u << 24, kMaxSampled = 1u << 28;
constexpr uint32_t kGateClamp = 1u << 29;  // see `pair`
constexpr int TX = 64, TY = 16;            // the tile of moving cells
constexpr uint32_t kQuantiseGridCap = 2048;
constexpr uint32_t kSearchGridCap = 512;   // two blocks a CU; each flushes (2S + 1)^2 entries at its end

// ---- quantise: grid min(ceil(n / 256), cap); every wave makes the same number of trips, so a ballot sees all of its lanes
__device__ __forceinline__ int32_t quantise(float x, float scale, bool& clipped) {
  const float t = x * scale;
  const bool ok = fabsf(t) <= 65536.0f;  // false for a NaN
  clipped = !ok && fabsf(x) <= 3.4028234663852886e38f;
  return ok ? (int32_t)rintf(t) : kInvalid;
}

__global__ __launch_bounds__(256) void k_quantise(const float* __restrict__ moving, const float* __restrict__ reference, int32_t* __restrict__ qm,
                                                  int32_t* __restrict__ qr, uint32_t w, uint32_t sw, uint32_t n, uint32_t g, float scale, uint32_t* head) {
  uint32_t count[4] = {0, 0, 0, 0};  // the same in every lane of a wave
  const uint32_t perTrip = gridDim.x * 256u;
  const uint32_t trips = (n - 1u) / perTrip + 1u;  // n >= 1
  for (uint32_t trip = 0; trip < trips; ++trip) {
    const uint32_t p = trip * perTrip + blockIdx.x * 256u + threadIdx.x;  // below n + 2^19 <= 2^28 + 2^19
    bool clippedM = false, clippedR = false;
    int32_t m = kInvalid, r = kInvalid;
    if (p < n) {
      const uint32_t j = p / sw, i = p - j * sw;
      const size_t src = (size_t)j * g * w + (size_t)i * g;  // j g < h and i g < w
      m = quantise(moving[src], scale, clippedM);
      r = quantise(reference[src], scale, clippedR);
      qm[p] = m;
      qr[p] = r;
    }
    count[0] += (uint32_t)__popcll(__ballot(m != kInvalid));
    count[1] += (uint32_t)__popcll(__ballot(r != kInvalid));
    count[2] += (uint32_t)__popcll(__ballot(clippedM));
    count[3] += (uint32_t)__popcll(__ballot(clippedR));
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (count[k]) atomicAdd(head + k, count[k]);
  }
}

// ---- search: grid min(tiles, cap), dynamic LDS (TX TY + (TY + 2S)(TX + 2S + 1)) words
// One pair.  m is a valid key, |m| <= 2^16; r is a key or the sentinel -2^31; |c| <= 2^18; G = min(gateQ, 2^29).  In arithmetic
// modulo 2^32, u = m - r - c + G.  r a key: |m - r - c| <= 2^17 + 2^18 < 2^29, so u <= 2G iff |d - c| <= G, and a G of 2^29
// passes every pair, as "no test" must.  r the sentinel: m - r = m + 2^31, so u lies in [2^31 - 2^16 - 2^18, 2^31 + 2^16 + 2^18 +
// 2^29], which does not wrap and is above 2G <= 2^30: the pair fails.  `mg` is m - c + G.
__device__ __forceinline__ void pair(uint32_t m, uint32_t mg, int32_t r, uint32_t twoG, uint32_t& n, int32_t& part, uint64_t& sq) {
  const bool ok = mg - (uint32_t)r <= twoG;
  const int32_t d = ok ? (int32_t)(m - (uint32_t)r) : 0;  // |d| <= 2^17
  n += ok ? 1u : 0u;
  part += d;                                              // over a tile of 1024 cells |part| <= 2^27
  sq += (uint64_t)((int64_t)d * (int64_t)d);              // d d <= 2^34; at most 2^28 cells: below 2^62
}

// the cells of rows [rowLo, rowHi) of the staged tile against the first KA slots of the thread
template <int K, int KA>
__device__ __forceinline__ void walk(const int32_t* mt, const int32_t* rt, int rowLo, int rowHi, int RW, uint32_t offset, uint32_t twoG,
                                     const uint32_t (&base)[K], uint32_t (&n)[K], int32_t (&part)[K], uint64_t (&sq)[K]) {
  for (int my = rowLo; my < rowHi; ++my) {
    for (int mx = 0; mx < TX; mx += 4) {
      const int4 m4 = *reinterpret_cast<const int4*>(mt + my * TX + mx);  // one address for the whole wave
      const int32_t mk[4] = {__builtin_amdgcn_readfirstlane(m4.x), __builtin_amdgcn_readfirstlane(m4.y), __builtin_amdgcn_readfirstlane(m4.z),
                             __builtin_amdgcn_readfirstlane(m4.w)};
      const int32_t* row = rt + my * RW + mx;
      if (mk[0] != kInvalid && mk[1] != kInvalid && mk[2] != kInvalid && mk[3] != kInvalid) {  // no branch between the 4 KA reads
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int k = 0; k < KA; ++k) pair((uint32_t)mk[u], (uint32_t)mk[u] + offset, row[base[k] + u], twoG, n[k], part[k], sq[k]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (mk[u] == kInvalid) continue;  // the whole wave
#pragma unroll
          for (int k = 0; k < KA; ++k) pair((uint32_t)mk[u], (uint32_t)mk[u] + offset, row[base[k] + u], twoG, n[k], part[k], sq[k]);
        }
      }
    }
  }
}

// K = ceil((2S + 1)^2 / 256): slot k of a thread is entry thread + 256 k, and only its last slot can lie behind the table
template <int K>
__global__ __launch_bounds__(256) void k_search(const int32_t* __restrict__ qm, const int32_t* __restrict__ qr, uint32_t sw, uint32_t sh, uint32_t tilesX,
                                                uint32_t tiles, int32_t cx, int32_t cy, int32_t S, uint32_t offset /* G - centerQ */, uint32_t twoG,
                                                ssrlcv_shift_entry* table) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  int32_t* mt = lds;            // [TY][TX]
  int32_t* rt = lds + TX * TY;  // [TY + 2S][RW]
  const int L = 2 * S + 1, count = L * L, HW = TX + 2 * S, RW = HW + 1, RH = TY + 2 * S;
  // the slots of this thread, and the rows of the tile its wave walks: all 16, or -- with at most 128 shifts -- the share of its
  // group of `slots` threads
  int slots = 256, rowLo = 0, rowHi = TY;
  if (K == 1 && count <= 128) {
    slots = count <= 64 ? 64 : 128;
    const int groups = 256 / slots, group = __builtin_amdgcn_readfirstlane((int)threadIdx.x / slots);
    rowLo = group * (TY / groups);
    rowHi = rowLo + TY / groups;
  }
  const int first = (int)threadIdx.x % slots;  // its slot at k = 0
  // whether any lane of this wave has a shift in its last slot: the whole wave takes one of the two walks
  const bool lastLive = __builtin_amdgcn_readfirstlane(((int)threadIdx.x & ~63) % slots) + 256 * (K - 1) < count;
  uint32_t base[K], n[K];
  int64_t sum[K];
  uint64_t sq[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = first + 256 * k, ee = e < count ? e : 0;  // a slot without a shift reads entry 0's words and is never flushed
    base[k] = (uint32_t)((ee / L) * RW + ee % L);
    n[k] = 0;
    sum[k] = 0;
    sq[k] = 0;
  }
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int tx0 = (int)(tile % tilesX) * TX, ty0 = (int)(tile / tilesX) * TY;  // below 2^24 + 64
    const int rx0 = tx0 + cx - S, ry0 = ty0 + cy - S;                            // |.| < 2^25 + 2^7: the reference tile's corner
    if (rx0 >= (int)sw || rx0 + HW <= 0 || ry0 >= (int)sh || ry0 + RH <= 0) continue;  // the whole block: no shift of this tile is inside
    __syncthreads();  // the tile before has been read
    for (int i = threadIdx.x; i < TX * TY; i += 256) {
      const uint32_t gx = (uint32_t)(tx0 + (i & (TX - 1))), gy = (uint32_t)(ty0 + i / TX);
      mt[i] = (gx < sw && gy < sh) ? qm[(size_t)gy * sw + gx] : kInvalid;
    }
    for (int i = threadIdx.x; i < RH * HW; i += 256) {
      const int y = i / HW, x = i - y * HW;
      const int gx = rx0 + x, gy = ry0 + y;
      rt[y * RW + x] = (gx >= 0 && gx < (int)sw && gy >= 0 && gy < (int)sh) ? qr[(size_t)gy * sw + (size_t)gx] : kInvalid;
    }
    __syncthreads();
    int32_t part[K];
#pragma unroll
    for (int k = 0; k < K; ++k) part[k] = 0;
    if (lastLive) walk<K, K>(mt, rt, rowLo, rowHi, RW, offset, twoG, base, n, part, sq);
    else if (K > 1) walk<K, (K > 1 ? K - 1 : 1)>(mt, rt, rowLo, rowHi, RW, offset, twoG, base, n, part, sq);
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] += (int64_t)part[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = first + 256 * k;
    if (e < count && n[k] != 0u) {  // n == 0: the sums are 0 too
      atomicAdd(&table[e].n, n[k]);
      atomicAdd(reinterpret_cast<unsigned long long*>(&table[e].sum), (unsigned long long)sum[k]);  // two's complement: the signed sum
      atomicAdd(reinterpret_cast<unsigned long long*>(&table[e].sumSq), (unsigned long long)sq[k]);
    }
  }
}

// ---- host side
inline bool bad_params(const ssrlcv_shift_params* p) {
  if (!p) return true;
  if (!(p->scale > 0.0f && p->scale <= 3.4028234663852886e38f)) return true;
  if (p->stride == 0 || p->radius > kMaxRadius) return true;
  if (p->centerX > kMaxCenter || p->centerX < -kMaxCenter || p->centerY > kMaxCenter || p->centerY < -kMaxCenter) return true;
  return p->centerQ > kMaxCenterQ || p->centerQ < -kMaxCenterQ;
}
inline uint32_t sampled(uint32_t side, uint32_t g) { return (uint32_t)(((uint64_t)side + g - 1u) / g); }
inline bool bad_size(uint32_t w, uint32_t h, uint32_t g) {
  return w > kMaxSide || h > kMaxSide || (uint64_t)sampled(w, g) * sampled(h, g) > kMaxSampled;
}
inline size_t entries(uint32_t radius) { return (size_t)(2u * radius + 1u) * (2u * radius + 1u); }
inline size_t table_bytes(uint32_t radius) { return sizeof(ssrlcv_shift_table) + entries(radius) * sizeof(ssrlcv_shift_entry); }
inline size_t keys_bytes(uint32_t sw, uint32_t sh) { return align256((size_t)4 * sw * sh); }

static_assert(sizeof(ssrlcv_shift_params) == 28 && sizeof(ssrlcv_shift_entry) == 24 && sizeof(ssrlcv_shift_table) == 16 && sizeof(ssrlcv_shift_result) == 64,
              "the layouts of include/ssrlcv_hip.h");

}  // namespace svshift

#ifndef SSRLCV_SHIFT_LAB
extern "C" {

size_t ssrlcv_shift_table_bytes(uint32_t radius) { return radius > svshift::kMaxRadius ? 0 : svshift::table_bytes(radius); }

size_t ssrlcv_hip_shift_search_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_shift_params* params) {
  using namespace svshift;
  if (bad_params(params) || bad_size(w, h, params->stride) || w == 0 || h == 0) return 0;
  return 2 * keys_bytes(sampled(w, params->stride), sampled(h, params->stride));
}

int ssrlcv_hip_shift_search(const float* moving, const float* reference, uint32_t w, uint32_t h, const ssrlcv_shift_params* params,
                            ssrlcv_shift_table* table, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  using namespace svshift;
  if (bad_params(params)) return SSRLCV_ERR_INVALID_ARG;
  if (bad_size(w, h, params->stride)) return SSRLCV_ERR_UNSUPPORTED;
  if (!table || ((uintptr_t)table & 7u)) return SSRLCV_ERR_INVALID_ARG;  // the 64-bit sums are added in place
  const hipStream_t st = (hipStream_t)stream;
  if (w != 0 && h != 0) {
    if (!moving || !reference || !workspace) return SSRLCV_ERR_INVALID_ARG;
    if (workspaceBytes < ssrlcv_hip_shift_search_workspace_bytes(w, h, params)) return SSRLCV_ERR_WORKSPACE;
  }
  SSRLCV_HIP_TRY(hipMemsetAsync(table, 0, table_bytes(params->radius), st));  // the atomics below add into zeros
  if (w == 0 || h == 0) return SSRLCV_OK;
  const uint32_t g = params->stride, sw = sampled(w, g), sh = sampled(h, g), n = sw * sh;  // n <= 2^28
  int32_t* qm = (int32_t*)workspace;
  int32_t* qr = (int32_t*)((char*)workspace + keys_bytes(sw, sh));
  const uint32_t blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_quantise, dim3(blocks < kQuantiseGridCap ? blocks : kQuantiseGridCap), dim3(256), 0, st, moving, reference, qm, qr, w, sw, n, g,
                     params->scale, (uint32_t*)table);
  SSRLCV_LAUNCH_CHECK();
  const int S = (int)params->radius;
  const uint32_t tilesX = (sw + TX - 1u) / TX, tiles = tilesX * ((sh + TY - 1u) / TY);  // below n / 1024 + sw / 64 + sh / 16 + 2 < 2^21
  const uint32_t G = params->gateQ < kGateClamp ? params->gateQ : kGateClamp;
  const uint32_t offset = G - (uint32_t)params->centerQ, twoG = 2u * G;
  const size_t ldsBytes = (size_t)4 * (TX * TY + (TY + 2 * S) * (TX + 2 * S + 1));  // 45 376 at S = 32
  const dim3 grid(tiles < kSearchGridCap ? tiles : kSearchGridCap);
  ssrlcv_shift_entry* out = (ssrlcv_shift_entry*)(table + 1);
  const int need = (int)((entries(params->radius) + 255u) / 256u);  // slots a thread
#define SSRLCV_SHIFT_LAUNCH(K) \
  hipLaunchKernelGGL(k_search<K>, grid, dim3(256), ldsBytes, st, qm, qr, sw, sh, tilesX, tiles, params->centerX, params->centerY, S, offset, twoG, out)
  switch (need) {
#define SSRLCV_SHIFT_CASE(K) \
  case K: SSRLCV_SHIFT_LAUNCH(K); break;
    SSRLCV_SHIFT_CASE(1) SSRLCV_SHIFT_CASE(2) SSRLCV_SHIFT_CASE(3) SSRLCV_SHIFT_CASE(4) SSRLCV_SHIFT_CASE(5) SSRLCV_SHIFT_CASE(6)
    SSRLCV_SHIFT_CASE(7) SSRLCV_SHIFT_CASE(8) SSRLCV_SHIFT_CASE(9) SSRLCV_SHIFT_CASE(10) SSRLCV_SHIFT_CASE(11) SSRLCV_SHIFT_CASE(12)
    SSRLCV_SHIFT_CASE(13) SSRLCV_SHIFT_CASE(14) SSRLCV_SHIFT_CASE(15) SSRLCV_SHIFT_CASE(16) SSRLCV_SHIFT_CASE(17)  // 4225 entries at S = 32
#undef SSRLCV_SHIFT_CASE
    default: return SSRLCV_ERR_INVALID_ARG;
  }
#undef SSRLCV_SHIFT_LAUNCH
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_shift_pick_host(const ssrlcv_shift_table* table_host, size_t tableBytes, const ssrlcv_shift_params* params, uint32_t minOverlap,
                           ssrlcv_shift_result* out) {
  using namespace svshift;
  if (!table_host || !out || bad_params(params) || tableBytes != table_bytes(params->radius)) return SSRLCV_ERR_INVALID_ARG;
  const int S = (int)params->radius, L = 2 * S + 1;
  const char* first = (const char*)(table_host + 1);
  const uint32_t least = minOverlap > 1u ? minOverlap : 1u;
  double v[(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1)];
  bool candidate[(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1)];
  uint32_t candidates = 0;
  int best = -1, bestR2 = 0;
  for (int e = 0; e < L * L; ++e) {
    ssrlcv_shift_entry entry;
    memcpy(&entry, first + (size_t)e * sizeof entry, sizeof entry);
    candidate[e] = entry.n >= least;
    v[e] = 0.0;
    if (!candidate[e]) continue;
    ++candidates;
    const double mean = (double)entry.sum / (double)entry.n;
    const double meanSq = (double)entry.sumSq / (double)entry.n, square = mean * mean;
    v[e] = meanSq - square;
    const int kx = e % L - S, ky = e / L - S, r2 = kx * kx + ky * ky;
    if (best < 0 || v[e] < v[best] || (v[e] == v[best] && r2 < bestR2)) {  // entries come by ky, then kx: an equal r2 keeps the earlier one
      best = e;
      bestR2 = r2;
    }
  }
  if (best < 0) return SSRLCV_ERR_UNSUPPORTED;
  const int bx = best % L, by = best / L;
  auto step = [&](int minus, int plus, bool inside) {
    if (!inside || !candidate[minus] || !candidate[plus]) return 0.0;
    const double den = (v[minus] - v[best]) + (v[plus] - v[best]);
    if (!(den > 0.0)) return 0.0;
    const double s = 0.5 * (v[minus] - v[plus]) / den;
    return s > 0.5 ? 0.5 : s < -0.5 ? -0.5 : s;
  };
  const double stepX = step(best - 1, best + 1, bx > 0 && bx < L - 1), stepY = step(best - L, best + L, by > 0 && by < L - 1);
  double second = INFINITY;
  for (int e = 0; e < L * L; ++e) {
    const int dx = e % L - bx, dy = e / L - by;
    if (candidate[e] && (dx < -1 || dx > 1 || dy < -1 || dy > 1) && v[e] < second) second = v[e];
  }
  ssrlcv_shift_entry entry;
  memcpy(&entry, first + (size_t)best * sizeof entry, sizeof entry);
  const double g = (double)params->stride, scale = (double)params->scale, s2 = scale * scale;
  ssrlcv_shift_result r;
  r.shiftX = (int64_t)params->stride * ((int64_t)params->centerX + (bx - S));
  r.shiftY = (int64_t)params->stride * ((int64_t)params->centerY + (by - S));
  r.subX = stepX * g;
  r.subY = stepY * g;
  r.bias = ((double)entry.sum / (double)entry.n) / scale;
  r.variance = v[best] / s2;
  r.second = second / s2;  // +inf stays +inf
  r.n = entry.n;
  r.candidates = candidates;
  *out = r;
  return SSRLCV_OK;
}

}  // extern "C"
#endif
