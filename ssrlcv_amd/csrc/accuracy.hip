// ssrlcv_amd/csrc/accuracy.hip -- surface accuracy for gfx950: the signed height difference of every point of a cloud to a reference
// height map, and exact robust statistics of such differences.  The contract is include/ssrlcv_hip.h "surface accuracy";
// tests/accuracy_ref.py restates it.
//
//   k_dsm_difference  a thread per point: the point in the frame by the expression of the surface model (dsm_frame.h), then the
//                     reference's height under it -- the cell's own height (CELL), or the plane of the triangle of the reference's
//                     mesh it lies in, from the `cells` bytes of ssrlcv_hip_disparity_mesh (MESH: mesh_lookup.h, the definition
//                     register.hip shares) -- in fixed-order float32
//   k_stats_tiles     a block walks tiles of 4096 values: the float64 sums of y and y y in the contract's shape (lane l adds entries
//                     l + 256 r in order, the lanes fold by halves), one partial a tile; the counts, the least and the greatest key
//                     in registers and one integer atomic each a block; the histogram of the keys' first digit in LDS, flushed by
//                     integer atomics
//   k_stats_reduce    the partials by the same shape again, a block a tile of 4096 partials
//   k_stats_hist      the histogram of the next digit of the values that share a quantile's prefix, one histogram for every
//                     distinct prefix
//   k_stats_narrow    one block: every quantile's rank inside its histogram picks the digit, the prefix grows, the rank shrinks;
//                     equal prefixes share a histogram in the next pass; behind the last digit the prefix IS the value, and the
//                     record is written
// Radix select over the order keys, digits of 11, 11 and 10 bits from the top.  Integer adds and maxima commute and the sums have a fixed
// shape, so the record is bit-equal run to run; there is no float atomic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "mesh_lookup.h"
#include "order_key.h"

namespace {

using dsm::finite_bits;
using dsm::frame_ok;
using dsm::too_long_a_side;
using dsm::too_many_cells;

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kTile = 4096;     // values a tile: 256 lanes x 16 entries
constexpr uint32_t kSlots = 8;       // quantiles a call
constexpr uint32_t kMaxBlocks = 2048;  // 256 CUs x 8 blocks of 4 waves

// The digits of the radix select, from the top: 11, 11 and 10 bits.  Measured against 4 x 8 bits on 16 M values
// (profiles/accuracy_bench.txt): a pass over the values less, and faster in five of six rows.
constexpr uint32_t kPasses = 3, kMaxBins = 2048;
constexpr uint32_t kShift[kPasses] = {21, 10, 0}, kBits[kPasses] = {11, 11, 10};
constexpr uint32_t kCUs = 256, kLdsPerCU = 160u * 1024u;  // MI355X: how many blocks of a histogram pass a CU holds at once

// ---- the difference

__device__ __forceinline__ bool finite_f(float v) { return finite_bits(__float_as_uint(v)); }

__global__ __launch_bounds__(256) void k_dsm_difference(const ssrlcv_float3* __restrict__ points, uint32_t n, const float* __restrict__ height,
                                                        ssrlcv_dsm_frame f, const uint8_t* __restrict__ cells, uint32_t* __restrict__ diff) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // below 2^32: at most 2^24 blocks
  if (t >= n) return;
  uint32_t out = kNaN;
  float u, v, z;
  if (dsm::point_uvz(points[t], f, u, v, z) && finite_f(z)) {
    if (!cells) {  // CELL: the height of the cell the point falls into
      const float fi = floorf(u), fj = floorf(v);
      if (fi >= 0.0f && fi < (float)f.w && fj >= 0.0f && fj < (float)f.h) {
        const float r = height[(uint32_t)fj * f.w + (uint32_t)fi];  // below w h < 2^31
        if (__float_as_uint(r) != kNaN && finite_f(r)) out = __float_as_uint(z - r);
      }
    } else {  // MESH: the triangle of the reference's mesh under the point (mesh_lookup.h)
      float d, rs, rt;
      if (dsm::mesh_difference(u, v, z, height, cells, f.w, f.h, d, rs, rt)) out = __float_as_uint(d);
    }
  }
  diff[t] = out;
}

// ---- the statistics

struct StatsCtrl {               // the head of the workspace, cleared at the start of a call
  uint32_t valid, finite;        // counts
  uint32_t leastInv, greatest;   // the maxima of ~ukey and of ukey over the finite values
  uint32_t prefix[kSlots];       // a quantile's resolved digits, in place
  uint32_t rank[kSlots];         // its rank among the values that share them
  uint32_t group[kSlots];        // the histogram it reads in the next pass
  uint32_t groupPrefix[kSlots];  // the prefix of every histogram
  uint32_t groups;
  uint32_t pad[3];
  double2 total;                 // the sums, where a third level is needed
};
static_assert(sizeof(StatsCtrl) <= 256, "the control block is the first 256 bytes of the workspace");

// the unsigned form of the order key: the float order as an unsigned integer order
__device__ __forceinline__ uint32_t ukey_of(uint32_t bits) { return (uint32_t)order_key(bits) ^ 0x80000000u; }
__device__ __forceinline__ uint32_t bits_of(uint32_t ukey) { return (uint32_t)order_key(ukey ^ 0x80000000u); }

// y of an entry and whether it takes part
__device__ __forceinline__ bool transformed(uint32_t bits, float center, uint32_t absolute, float& y, bool& valid) {
  valid = bits != kNaN;
  y = __uint_as_float(bits) - center;
  if (absolute) y = fabsf(y);
  return valid && finite_f(y);
}

// One add to an LDS histogram for every active lane.  The first active lane's digit is taken out first, twice: its lanes are counted
// by a ballot and one of them adds the number, so an input whose values share the digit (a constant map: every digit of every
// pass) costs one LDS atomic a wave instead of 64 on one address, as k_dsm_scatter merges the lanes of one cell.  Every lane of the
// wave calls this together.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t digit, bool active) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long left = __ballot(active);
    if (left == 0ull) return;  // the same in every lane
    const int first = __ffsll(left) - 1;
    const uint32_t d = __shfl(digit, first, 64);
    const unsigned long long same = __ballot(active && digit == d);
    if (lane == first) atomicAdd(hist + d, (uint32_t)__popcll(same));
    active = active && digit != d;
  }
  if (active) atomicAdd(hist + digit, 1u);
}

// the 256 lane sums of a tile folded by halves (128, 64 through LDS; 32 .. 1 inside wave 0): thread 0 holds the tile's sums
__device__ __forceinline__ void fold_tile(double& s, double& ss, double (*fold)[256]) {
  const uint32_t l = threadIdx.x;
  fold[0][l] = s;
  fold[1][l] = ss;
  __syncthreads();
  if (l < 64u) {
    s = (fold[0][l] + fold[0][l + 128u]) + (fold[0][l + 64u] + fold[0][l + 192u]);
    ss = (fold[1][l] + fold[1][l + 128u]) + (fold[1][l + 64u] + fold[1][l + 192u]);
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) {
      s += __shfl_down(s, half, 64);
      ss += __shfl_down(ss, half, 64);
    }
  }
  __syncthreads();  // the fold arrays are free again
}

__global__ __launch_bounds__(256) void k_stats_tiles(const uint32_t* __restrict__ values, uint32_t n, uint32_t tiles, float center, uint32_t absolute,
                                                     uint32_t bins, uint32_t shift, StatsCtrl* __restrict__ ctrl, uint32_t* __restrict__ hist,
                                                     double2* __restrict__ partial) {
  extern __shared__ uint32_t lhist[];  // `bins` words: the first digit's histogram; none without a quantile
  __shared__ double fold[2][256];
  __shared__ uint32_t red[4][4];
  const uint32_t l = threadIdx.x;
  for (uint32_t b = l; b < bins; b += 256u) lhist[b] = 0u;
  __syncthreads();
  uint32_t nValid = 0, nFinite = 0, leastInv = 0, greatest = 0;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned long long base = (unsigned long long)tile * kTile + l;
    uint32_t bits[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned long long at = base + 256u * (unsigned)r;
      bits[r] = at < n ? values[at] : kNaN;  // padding is an invalid entry
    }
    double s = 0.0, ss = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float y;
      bool valid;
      const bool fin = transformed(bits[r], center, absolute, y, valid);
      const double d = fin ? (double)y : 0.0;
      s += d;
      ss += d * d;
      nValid += valid ? 1u : 0u;
      nFinite += fin ? 1u : 0u;
      const uint32_t k = ukey_of(__float_as_uint(y));
      leastInv = fin ? max(leastInv, ~k) : leastInv;
      greatest = fin ? max(greatest, k) : greatest;
      if (bins) hist_add(lhist, k >> shift, fin);
    }
    fold_tile(s, ss, fold);
    if (l == 0u) partial[tile] = make_double2(s, ss);
  }
  // the block's counts and extremes: shuffles inside a wave, four words a wave through LDS, one atomic each
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    nValid += __shfl_down(nValid, o, 64);
    nFinite += __shfl_down(nFinite, o, 64);
    leastInv = max(leastInv, __shfl_down(leastInv, o, 64));
    greatest = max(greatest, __shfl_down(greatest, o, 64));
  }
  if ((l & 63u) == 0u) {
    red[l >> 6][0] = nValid, red[l >> 6][1] = nFinite, red[l >> 6][2] = leastInv, red[l >> 6][3] = greatest;
  }
  __syncthreads();
  if (l == 0u) {
    atomicAdd(&ctrl->valid, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    atomicAdd(&ctrl->finite, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
    atomicMax(&ctrl->leastInv, max(max(red[0][2], red[1][2]), max(red[2][2], red[3][2])));
    atomicMax(&ctrl->greatest, max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3])));
  }
  for (uint32_t b = l; b < bins; b += 256u) {
    const uint32_t c = lhist[b];
    if (c) atomicAdd(hist + b, c);
  }
}

__global__ __launch_bounds__(256) void k_stats_reduce(const double2* __restrict__ in, uint32_t count, double2* __restrict__ out) {
  __shared__ double fold[2][256];
  const unsigned long long base = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
  double s = 0.0, ss = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const unsigned long long at = base + 256u * (unsigned)r;
    const double2 p = at < count ? in[at] : make_double2(0.0, 0.0);
    s += p.x;
    ss += p.y;
  }
  fold_tile(s, ss, fold);
  if (threadIdx.x == 0u) out[blockIdx.x] = make_double2(s, ss);
}

__global__ __launch_bounds__(256) void k_stats_hist(const uint32_t* __restrict__ values, uint32_t n, uint32_t tiles, float center, uint32_t absolute,
                                                    uint32_t bins, uint32_t shift, const StatsCtrl* __restrict__ ctrl, uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t lhist[];  // `bins` words for every histogram of this pass
  const uint32_t l = threadIdx.x;
  const uint32_t groups = ctrl->groups;  // at most kSlots; 0 when no value takes part
  if (groups == 0u) return;
  const uint32_t resolved = shift + __popc(bins - 1u);  // the digits above this one: below 32 behind the first pass
  uint32_t want[kSlots];
#pragma unroll
  for (uint32_t g = 0; g < kSlots; ++g) want[g] = g < groups ? ctrl->groupPrefix[g] >> resolved : 0u;
  for (uint32_t b = l; b < groups * bins; b += 256u) lhist[b] = 0u;
  __syncthreads();
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned long long base = (unsigned long long)tile * kTile + l;
    uint32_t bits[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned long long at = base + 256u * (unsigned)r;
      bits[r] = at < n ? values[at] : kNaN;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float y;
      bool valid;
      const bool fin = transformed(bits[r], center, absolute, y, valid);
      const uint32_t k = ukey_of(__float_as_uint(y));
      const uint32_t digit = (k >> shift) & (bins - 1u);
#pragma unroll
      for (uint32_t g = 0; g < kSlots; ++g) {
        if (g < groups) hist_add(lhist + g * bins, digit, fin && (k >> resolved) == want[g]);  // `groups` is the same in every lane
      }
    }
  }
  __syncthreads();
  for (uint32_t b = l; b < groups * bins; b += 256u) {
    const uint32_t c = lhist[b];
    if (c) atomicAdd(hist + (b / bins) * kMaxBins + (b % bins), c);
  }
}

__global__ __launch_bounds__(256) void k_stats_narrow(StatsCtrl* __restrict__ ctrl, const uint32_t* __restrict__ hist, ssrlcv_diff_stats_params prm,
                                                      uint32_t pass, uint32_t bins, uint32_t shift, uint32_t n, const double2* __restrict__ total,
                                                      ssrlcv_diff_stats* __restrict__ out) {
  __shared__ uint32_t scan[256];
  __shared__ uint32_t newPrefix[kSlots], newRank[kSlots];
  const uint32_t l = threadIdx.x, per = bins >> 8;  // bins is 256, 1024 or 2048
  const uint32_t m = ctrl->finite;
  const uint32_t slots = m ? prm.numQuantiles : 0u;
  for (uint32_t k = 0; k < slots; ++k) {
    const uint32_t rank = pass ? ctrl->rank[k] : (uint32_t)((unsigned long long)prm.quantile[k] * (m - 1u) / 10000ull);
    const uint32_t prefix = pass ? ctrl->prefix[k] : 0u;
    const uint32_t* h = hist + (pass ? ctrl->group[k] : 0u) * kMaxBins + l * per;
    uint32_t mine = 0;
    for (uint32_t i = 0; i < per; ++i) mine += h[i];
    scan[l] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {  // the inclusive sums of the 256 chunks
      const uint32_t below = l >= o ? scan[l - o] : 0u;
      __syncthreads();
      scan[l] += below;
      __syncthreads();
    }
    uint32_t before = scan[l] - mine;
    if (rank >= before && rank < scan[l]) {  // one thread: the histogram holds more than `rank` values
      for (uint32_t i = 0; i < per; ++i) {
        const uint32_t c = h[i];
        if (rank < before + c) {
          newPrefix[k] = prefix | ((l * per + i) << shift);
          newRank[k] = rank - before;
          break;
        }
        before += c;
      }
    }
    __syncthreads();
  }
  if (l != 0u) return;
  uint32_t groups = 0;
  for (uint32_t k = 0; k < slots; ++k) {  // equal prefixes share the next pass's histogram
    uint32_t g = groups;
    for (uint32_t j = 0; j < k; ++j)
      if (newPrefix[j] == newPrefix[k]) {
        g = ctrl->group[j];
        break;
      }
    if (g == groups) ctrl->groupPrefix[groups++] = newPrefix[k];
    ctrl->prefix[k] = newPrefix[k];
    ctrl->rank[k] = newRank[k];
    ctrl->group[k] = g;
  }
  ctrl->groups = groups;
  if (!out) return;
  out->n = n;
  out->valid = ctrl->valid;
  out->finite = m;
  out->reserved = 0u;
  out->sum = total->x;
  out->sumSq = total->y;
  out->min = __uint_as_float(m ? bits_of(~ctrl->leastInv) : kNaN);
  out->max = __uint_as_float(m ? bits_of(ctrl->greatest) : kNaN);
  for (uint32_t k = 0; k < kSlots; ++k) out->quantile[k] = __uint_as_float(k < slots ? bits_of(newPrefix[k]) : kNaN);
}

__global__ void k_stats_empty(ssrlcv_diff_stats* out) {
  out->n = out->valid = out->finite = out->reserved = 0u;
  out->sum = out->sumSq = 0.0;
  out->min = out->max = __uint_as_float(kNaN);
  for (uint32_t k = 0; k < kSlots; ++k) out->quantile[k] = __uint_as_float(kNaN);
}

// ---- host side
bool params_ok(const ssrlcv_diff_stats_params* p) {
  if (!p || p->numQuantiles > kSlots) return false;
  for (uint32_t k = 0; k < p->numQuantiles; ++k)
    if (p->quantile[k] > 10000u) return false;
  return dsm::finite_host(p->center) && p->absolute <= 1u;
}

uint32_t tiles_of(uint32_t n) { return (uint32_t)(((unsigned long long)n + kTile - 1u) / kTile); }
constexpr size_t kCtrlBytes = 256;
constexpr size_t kHistBytes = (size_t)kPasses * kSlots * kMaxBins * 4;  // a multiple of 256
size_t partial_bytes(uint32_t count) { return align256((size_t)count * sizeof(double2)); }
size_t stats_bytes(uint32_t n) { return kCtrlBytes + kHistBytes + partial_bytes(tiles_of(n)) + partial_bytes(tiles_of(tiles_of(n))); }

}  // namespace

extern "C" {

int ssrlcv_hip_dsm_difference(const ssrlcv_float3* points, uint32_t n, const float* height, const ssrlcv_dsm_frame* frame, const uint8_t* cells,
                              float* diff, ssrlcv_stream_t stream) {
  if (!frame_ok(frame) || too_many_cells(frame->w, frame->h)) return SSRLCV_ERR_INVALID_ARG;
  if (too_long_a_side(frame->w, frame->h)) return SSRLCV_ERR_UNSUPPORTED;
  if (n == 0) return SSRLCV_OK;
  if (!points || !height || !diff) return SSRLCV_ERR_INVALID_ARG;
  const dim3 blocks((uint32_t)(((unsigned long long)n + 255u) / 256u));
  hipLaunchKernelGGL(k_dsm_difference, blocks, dim3(256), 0, (hipStream_t)stream, points, n, height, *frame, cells, (uint32_t*)diff);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_difference_stats_workspace_bytes(uint32_t n, const ssrlcv_diff_stats_params* params) {
  return params_ok(params) ? stats_bytes(n) : 0;
}

int ssrlcv_hip_difference_stats(const float* values, uint32_t n, const ssrlcv_diff_stats_params* params, ssrlcv_diff_stats* out_dev, void* workspace,
                                size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!params_ok(params) || !out_dev) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // the empty record, and nothing else is looked at
    hipLaunchKernelGGL(k_stats_empty, dim3(1), dim3(1), 0, st, out_dev);
    SSRLCV_LAUNCH_CHECK();
    return SSRLCV_OK;
  }
  if (!values || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < stats_bytes(n)) return SSRLCV_ERR_WORKSPACE;
  const uint32_t t1 = tiles_of(n), t2 = tiles_of(t1);
  unsigned char* base = (unsigned char*)workspace;
  StatsCtrl* ctrl = (StatsCtrl*)base;
  uint32_t* hist = (uint32_t*)(base + kCtrlBytes);
  double2* partial1 = (double2*)(base + kCtrlBytes + kHistBytes);
  double2* partial2 = (double2*)(base + kCtrlBytes + kHistBytes + partial_bytes(t1));
  const uint32_t* bits = (const uint32_t*)values;
  const uint32_t q = params->numQuantiles;
  const dim3 walkers(t1 < kMaxBlocks ? t1 : kMaxBlocks);
  SSRLCV_HIP_TRY(hipMemsetAsync(base, 0, kCtrlBytes + kHistBytes, st));
  const uint32_t bins0 = q ? 1u << kBits[0] : 0u;
  hipLaunchKernelGGL(k_stats_tiles, walkers, dim3(256), (size_t)bins0 * 4, st, bits, n, t1, params->center, params->absolute, bins0, kShift[0], ctrl, hist,
                     partial1);
  SSRLCV_LAUNCH_CHECK();
  const double2* total = partial1;  // one tile: its partial is the total
  if (t1 > 1u) {
    hipLaunchKernelGGL(k_stats_reduce, dim3(t2), dim3(256), 0, st, partial1, t1, partial2);
    SSRLCV_LAUNCH_CHECK();
    total = partial2;
    if (t2 > 1u) {  // at most 256 second-level partials: the third level is one tile, into the control block
      hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(256), 0, st, partial2, t2, &ctrl->total);
      SSRLCV_LAUNCH_CHECK();
      total = &ctrl->total;
    }
  }
  const uint32_t passes = q ? kPasses : 1u;  // without a quantile the first narrowing step only writes the record
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t bins = 1u << kBits[p];
    uint32_t* h = hist + (size_t)p * kSlots * kMaxBins;
    if (p) {
      // every block clears and flushes its q histograms: no more blocks than the chip holds at once (two at 8 x 2048 bins)
      const uint32_t lds = q * bins * 4u, resident = kCUs * (kLdsPerCU / lds < 8u ? kLdsPerCU / lds : 8u);
      const dim3 counters(t1 < resident ? t1 : resident);
      hipLaunchKernelGGL(k_stats_hist, counters, dim3(256), (size_t)lds, st, bits, n, t1, params->center, params->absolute, bins, kShift[p], ctrl, h);
      SSRLCV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_stats_narrow, dim3(1), dim3(256), 0, st, ctrl, h, *params, p, bins, kShift[p], n, total, p + 1u == passes ? out_dev : nullptr);
    SSRLCV_LAUNCH_CHECK();
  }
  return SSRLCV_OK;
}

}  // extern "C"
