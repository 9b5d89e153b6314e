// ssrlcv_amd/csrc/objects.hip -- what stands on the terrain, for gfx950: the connected footprints of the cells of an object-height
// map that are at least minHeight high, one record each, and the map of their numbers.  The contract is include/ssrlcv_hip.h
// "surface objects"; tests/objects_ref.py restates it.  A record holds integer sums, integer minima and maxima and selected bit
// patterns only, so the order of the cells does not matter and the kernels are held to the restatement byte for byte.
//
//   k_obj_mask      a thread a cell: the member map, v where the cell is valid and v >= minHeight, the invalid pattern elsewhere.
//   svcc::label_components   the labelling of disparity_filter.hip on that map (cc_label.h): labels[p] names p's tile-local root,
//                   labels[labels[p]] the object's label, counts[label] its cells.
//   ObjKeep / ObjEmit + compact.h   the roots with counts >= minCells in raster order: a root's place in that order is its
//                   object's number, written where the member map stood (the labelling has read it), and the thread that emits a
//                   root below `capacity` initialises its record: label, cells, zeros, and the neutral elements of the minima.
//   k_obj_reduce    a block a 64 x 16 tile of k_cc_tile's tiling, a wave a row; a tile without a member leaves after one block-wide
//                   vote and writes its ids alone.  Per cell: the final label (two hops), the
//                   quantised height, the sides it shares with no cell of its object -- final labels of the tile and a halo of one
//                   cell stand in LDS.  Adjacent lanes of one tile-local root form a run (one ballot, as k_cc_tile); clipped,
//                   perimeter, q, q q, the peak and the low key are added over the run by shuffles (as k_dsm_scatter), the sums
//                   of the coordinates of a run are closed forms.  A run's last lane adds it into the LDS slot of its tile-local
//                   root -- tile-local coordinates, so three packed 64-bit words hold nine sums -- and each slot that met a cell is
//                   flushed once into its record: 64-bit atomic adds for the sums, a 64-bit atomic max on (key, complemented
//                   index) for the peak, 32-bit atomics for the box, the low key, perimeter and clipped.  A slot that holds the
//                   whole object stores instead.  The same pass writes ids from the slots' numbers.
//   k_obj_finish    a thread a record: the peak's and the low's keys back to bits; thread 0 writes *count_dev.
// No float atomics, no block waits for another: bit-equal run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "cc_label.h"
#include "compact.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "order_key.h"

namespace svobj {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int TX = svcc::kTileW, TY = svcc::kTileH, kSlots = TX * TY;  // a wave is a row: the ballots rely on TX == 64
constexpr int kRowsPerLane = kSlots / 256;
constexpr int HW = TX + 2, HH = TY + 2;        // the tile of final labels with its halo
constexpr uint32_t kMaxSide = 65536u, kMaxCells = 1u << 30;
constexpr uint32_t kPerThread = 16;            // compact.h: a wave owns a run of 1024 elements, a block 4096
constexpr uint32_t kMaskGridCap = 4096;        // blocks of 256 cells
constexpr uint32_t kReduceGridCap = 1024;      // blocks of one tile: four a CU, two of them resident beside their 61 KB of LDS
constexpr uint32_t kFinishGridCap = 1024;      // blocks of 256 records

static_assert(sizeof(ssrlcv_object_params) == 16 && sizeof(ssrlcv_object_record) == 104 && sizeof(ssrlcv_object_measures) == 152,
              "the layouts of include/ssrlcv_hip.h");
static_assert(offsetof(ssrlcv_object_record, peakIndex) == 32 && offsetof(ssrlcv_object_record, peak) == 36 &&
              offsetof(ssrlcv_object_record, low) == 40 && offsetof(ssrlcv_object_record, sumX) == 48,
              "peakIndex and peak are one 64-bit word while the record is accumulated");

__device__ __forceinline__ bool is_member(uint32_t bits, float minHeight) { return bits != kNaN && __uint_as_float(bits) >= minHeight; }

// the order key as an unsigned number: the float order, -0 below +0
__device__ __forceinline__ uint32_t ukey(uint32_t bits) { return (uint32_t)order_key(bits) ^ 0x80000000u; }
__device__ __forceinline__ uint32_t ukey_bits(uint32_t key) { return (uint32_t)order_key(key ^ 0x80000000u); }

__global__ __launch_bounds__(256) void k_obj_mask(const uint32_t* __restrict__ in, uint32_t* __restrict__ mask, uint32_t n, float minHeight) {
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < n; c += gridDim.x * 256u) {
    const uint32_t bits = in[c];
    mask[c] = is_member(bits, minHeight) ? bits : kNaN;
  }
}

// while a record is accumulated: the word at peakIndex holds (key << 32) | (0xFFFFFFFF - index), `low` holds a key
struct ObjKeep {
  const uint32_t* labels;
  const uint32_t* counts;
  uint32_t minCells;  // >= 1
  __device__ uint32_t operator()(uint32_t p) const { return labels[p] == p && counts[p] >= minCells ? 1u : 0u; }
};
struct ObjEmit {
  const uint32_t* counts;
  uint32_t* number;
  ssrlcv_object_record* records;
  uint32_t capacity;
  __device__ void operator()(uint32_t p, int, uint32_t dst) const {
    number[p] = dst;
    if (dst >= capacity) return;
    ssrlcv_object_record r = {};
    r.label = p;
    r.cells = counts[p];
    const uint32_t none = kNone;
    r.minX = r.minY = none;
    __builtin_memcpy(&r.low, &none, 4);
    records[dst] = r;
  }
};

// the sums of one tile-local root over a tile, in tile-local coordinates lx < 64, ly < 16, at most 1024 cells:
//   a   n (11 bits) | clipped << 11 (11) | perimeter << 22 (12: at most 2 n + 2) | sum lx << 34 (15) | sum ly << 49 (13)
//   b   sum lx lx (21 bits) | sum lx ly << 21 (18) | sum ly ly << 39 (17)
struct Slots {
  unsigned long long a[kSlots], b[kSlots], qq[kSlots], peak[kSlots], columns[kSlots];
  int32_t q[kSlots];
  uint32_t rows[kSlots], low[kSlots], number[kSlots];
};

template <typename T>
__device__ __forceinline__ T run_add(T v, unsigned lane, unsigned start) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(v, o, 64);
    if (lane >= start + (unsigned)o) v += y;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_obj_reduce(const uint32_t* __restrict__ in, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ counts,
                                                    const uint32_t* __restrict__ number, uint32_t w, uint32_t h, uint32_t tilesX, uint32_t tiles,
                                                    float minHeight, float scale, uint32_t minCells, uint32_t* __restrict__ ids,
                                                    ssrlcv_object_record* __restrict__ records, uint32_t capacity) {
  __shared__ Slots s;
  __shared__ uint32_t finalLabel[HH * HW];
  const uint32_t lx = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
    const uint32_t x0 = tx * TX, y0 = ty * TY;  // below 65536
    uint32_t cell[kRowsPerLane];
    int anyMember = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      const uint32_t gx = x0 + lx, gy = y0 + wave + 4u * j;
      cell[j] = (gx < w && gy < h) ? in[gy * w + gx] : kNaN;  // below 2^30
      anyMember |= is_member(cell[j], minHeight) ? 1 : 0;
    }
    // also the barrier behind the tile before: its slots have been read.  A tile without a member has nothing to add: most tiles of
    // a map of buildings and trees
    if (!__syncthreads_or(anyMember)) {
      if (ids) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
          const uint32_t gx = x0 + lx, gy = y0 + wave + 4u * j;
          if (gx < w && gy < h) ids[gy * w + gx] = kNone;
        }
      }
      continue;
    }
    for (int i = threadIdx.x; i < kSlots; i += 256) {
      s.a[i] = s.b[i] = s.qq[i] = s.peak[i] = s.columns[i] = 0ull;
      s.q[i] = 0;
      s.rows[i] = 0u;
      s.low[i] = kNone;
    }
    // final labels of the tile and its halo: labels[labels[p]], UINT32_MAX outside the map and at a non-member
    for (int i = threadIdx.x; i < HH * HW; i += 256) {
      const int hy = i / HW, hx = i - hy * HW;
      const uint32_t gx = x0 + (uint32_t)hx - 1u, gy = y0 + (uint32_t)hy - 1u;  // wraps to above w, h at the map's first column, row
      uint32_t l = kNone;
      if (gx < w && gy < h) {
        l = labels[gy * w + gx];  // below 2^30
        if (l != kNone) l = labels[l];
      }
      finalLabel[i] = l;
    }
    __syncthreads();
    uint32_t slot[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      const uint32_t ly = wave + 4u * j, gx = x0 + lx, gy = y0 + ly;
      const bool inside = gx < w && gy < h;
      const uint32_t p = inside ? gy * w + gx : 0u;
      const uint32_t bits = cell[j];
      const bool member = is_member(bits, minHeight);
      // the tile-local root as a slot of this tile.  A tile-local root names the final root, which may lie in another tile: it is
      // its own slot then; if that root lies in this tile the cell joins its slot, which belongs to the same object
      uint32_t sl = kNone;
      if (member) {
        const uint32_t t = labels[p];
        const uint32_t tyy = t / w, txx = t - tyy * w;
        sl = (txx - x0 < (uint32_t)TX && tyy - y0 < (uint32_t)TY) ? (tyy - y0) * TX + (txx - x0) : ly * TX + lx;
      }
      slot[j] = sl;
      const uint32_t hi = (ly + 1u) * HW + lx + 1u, mine = finalLabel[hi];
      const uint32_t sides = (finalLabel[hi - 1] != mine) + (finalLabel[hi + 1] != mine) + (finalLabel[hi - HW] != mine) + (finalLabel[hi + HW] != mine);
      const float v = __uint_as_float(bits), t = v * scale;
      const bool takesPart = member && fabsf(t) <= 65536.0f;
      const int32_t q = takesPart ? (int32_t)rintf(t) : 0;
      // runs of adjacent lanes of one slot
      const uint32_t before = __shfl_up(sl, 1, 64);
      const unsigned long long heads = __ballot(member && (lx == 0u || before != sl));
      const unsigned long long below = heads & ((2ull << lx) - 1ull);
      const uint32_t start = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;  // of a member: never without a head
      const uint32_t after = __shfl_down(sl, 1, 64);
      const bool last = member && (lx == 63u || after != sl);
      const uint32_t cp = run_add<uint32_t>(member ? ((takesPart ? 0u : 1u) | sides << 16) : 0u, lx, start);  // clipped | perimeter << 16
      const int32_t sq = run_add<int32_t>(q, lx, start);
      const unsigned long long sqq = run_add<unsigned long long>((unsigned long long)((long long)q * (long long)q), lx, start);
      unsigned long long best = member ? ((unsigned long long)ukey(bits) << 32) | (unsigned long long)(kNone - p) : 0ull;
      uint32_t least = member ? ukey(bits) : kNone;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long yb = __shfl_up(best, o, 64);
        const uint32_t yl = __shfl_up(least, o, 64);
        if (lx >= start + (unsigned)o) {
          best = max(best, yb);
          least = min(least, yl);
        }
      }
      if (last) {
        const unsigned long long len = lx - start + 1u, sumX = (unsigned long long)(start + lx) * len / 2u;  // start + .. + lx
        // squares 0 .. k: k (k + 1) (2 k + 1) / 6
        const unsigned long long upTo = (unsigned long long)lx * (lx + 1u) * (2u * lx + 1u) / 6u;
        const unsigned long long under = start ? (unsigned long long)(start - 1u) * start * (2u * start - 1u) / 6u : 0ull;
        const unsigned long long a = len | (unsigned long long)(cp & 0xFFFFu) << 11 | (unsigned long long)(cp >> 16) << 22 | sumX << 34 | (len * ly) << 49;
        const unsigned long long b = (upTo - under) | (sumX * ly) << 21 | (len * ly * ly) << 39;
        atomicAdd(&s.a[sl], a);
        atomicAdd(&s.b[sl], b);
        if (sq) atomicAdd(&s.q[sl], sq);
        if (sqq) atomicAdd(&s.qq[sl], sqq);
        atomicMax(&s.peak[sl], best);
        atomicMin(&s.low[sl], least);
        atomicOr(&s.columns[sl], (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << start);
        atomicOr(&s.rows[sl], 1u << ly);
      }
    }
    __syncthreads();
    // each slot that met a cell: its object's number, and its sums into the record
    for (int i = threadIdx.x; i < kSlots; i += 256) {
      const unsigned long long a = s.a[i];
      const uint32_t n = (uint32_t)(a & 0x7FFu);
      if (n == 0u) continue;
      const uint32_t sy = (uint32_t)i / TX, sx = (uint32_t)i - sy * TX;
      const uint32_t root = labels[labels[(y0 + sy) * w + x0 + sx]], cells = counts[root];
      const uint32_t num = cells >= minCells ? number[root] : kNone;
      s.number[i] = num;
      if (num >= capacity) continue;  // dropped, or behind the records
      ssrlcv_object_record* r = records + num;
      const unsigned long long b = s.b[i];
      const unsigned long long clipped = a >> 11 & 0x7FFu, perimeter = a >> 22 & 0xFFFu, slx = a >> 34 & 0x7FFFu, sly = a >> 49;
      const unsigned long long sxx = b & 0x1FFFFFu, sxy = b >> 21 & 0x3FFFFu, syy = b >> 39;
      const unsigned long long X = x0, Y = y0, N = n;
      const unsigned long long sumX = N * X + slx, sumY = N * Y + sly;
      const unsigned long long sumXX = N * X * X + 2u * X * slx + sxx, sumXY = N * X * Y + X * sly + Y * slx + sxy, sumYY = N * Y * Y + 2u * Y * sly + syy;
      const unsigned long long columns = s.columns[i];
      const uint32_t rows = s.rows[i];
      const uint32_t minX = x0 + (uint32_t)__ffsll((long long)columns) - 1u, maxX = x0 + 63u - (uint32_t)__clzll((long long)columns);
      const uint32_t minY = y0 + (uint32_t)__ffs((int)rows) - 1u, maxY = y0 + 31u - (uint32_t)__clz((int)rows);
      const unsigned long long sumQ = (unsigned long long)(long long)s.q[i];  // two's complement: the signed sum
      unsigned long long* peakWord = reinterpret_cast<unsigned long long*>(&r->peakIndex);
      uint32_t* lowWord = reinterpret_cast<uint32_t*>(&r->low);
      if (n == cells) {  // the whole object: nobody else writes this record
        r->minX = minX, r->minY = minY, r->maxX = maxX, r->maxY = maxY;
        r->perimeter = (uint32_t)perimeter, r->clipped = (uint32_t)clipped;
        *peakWord = s.peak[i];
        *lowWord = s.low[i];
        r->sumX = sumX, r->sumY = sumY, r->sumXX = sumXX, r->sumXY = sumXY, r->sumYY = sumYY;
        r->sumQ = (long long)sumQ, r->sumQQ = s.qq[i];
        continue;
      }
      atomicMin(&r->minX, minX);
      atomicMin(&r->minY, minY);
      atomicMax(&r->maxX, maxX);
      atomicMax(&r->maxY, maxY);
      if (perimeter) atomicAdd(&r->perimeter, (uint32_t)perimeter);
      if (clipped) atomicAdd(&r->clipped, (uint32_t)clipped);
      atomicMax(peakWord, s.peak[i]);
      atomicMin(lowWord, s.low[i]);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumX), sumX);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumY), sumY);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumXX), sumXX);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumXY), sumXY);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumYY), sumYY);
      if (sumQ) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumQ), sumQ);
      if (s.qq[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumQQ), s.qq[i]);
    }
    if (!ids) continue;  // the whole block
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      const uint32_t gx = x0 + lx, gy = y0 + wave + 4u * j;
      if (gx < w && gy < h) ids[gy * w + gx] = slot[j] == kNone ? kNone : s.number[slot[j]];
    }
  }
}

// the keys of the records that were written back to bits, and the count
__global__ __launch_bounds__(256) void k_obj_finish(ssrlcv_object_record* __restrict__ records, uint32_t capacity, const uint32_t* __restrict__ total,
                                                    uint32_t* __restrict__ count_dev) {
  const uint32_t count = *total, written = count < capacity ? count : capacity;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count_dev = count;
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < written; k += gridDim.x * 256u) {
    ssrlcv_object_record* r = records + k;
    unsigned long long word;
    __builtin_memcpy(&word, &r->peakIndex, 8);
    uint32_t lowKey;
    __builtin_memcpy(&lowKey, &r->low, 4);
    const uint32_t peakBits = ukey_bits((uint32_t)(word >> 32)), lowBits = ukey_bits(lowKey);
    r->peakIndex = kNone - (uint32_t)word;
    __builtin_memcpy(&r->peak, &peakBits, 4);
    __builtin_memcpy(&r->low, &lowBits, 4);
  }
}

// ---- host side
inline bool bad_params(const ssrlcv_object_params* p) {
  if (!p) return true;
  if (p->minHeight != p->minHeight) return true;  // a NaN
  if (!(p->maxDiff >= 0.0f)) return true;         // a NaN or negative
  return !(p->scale > 0.0f && p->scale <= 3.4028234663852886e38f);
}
inline bool bad_size(uint32_t w, uint32_t h) { return w > kMaxSide || h > kMaxSide || (unsigned long long)w * h > kMaxCells; }
inline size_t map_bytes(uint32_t n) { return align256((size_t)4 * n); }
inline size_t compaction_bytes(uint32_t n) { return align256(svc::workspace_words<1, kPerThread>(n) * 4); }
inline uint32_t capped(uint32_t blocks, uint32_t cap) { return blocks < cap ? blocks : cap; }

struct Plan {
  uint32_t *number, *labels, *counts, *tables;  // `number` is the member map until the labelling has read it
  Plan(void* workspace, uint32_t n) {
    char* at = (char*)workspace;
    number = (uint32_t*)at;
    labels = (uint32_t*)(at + map_bytes(n));
    counts = (uint32_t*)(at + 2 * map_bytes(n));
    tables = (uint32_t*)(at + 3 * map_bytes(n));
  }
};

inline hipError_t launch_mask(const float* objects, uint32_t n, float minHeight, const Plan& plan, hipStream_t st) {
  hipLaunchKernelGGL(k_obj_mask, dim3(capped((n + 255u) / 256u, kMaskGridCap)), dim3(256), 0, st, (const uint32_t*)objects, plan.number, n, minHeight);
  return hipGetLastError();
}

inline hipError_t launch_reduce(const float* objects, uint32_t w, uint32_t h, const ssrlcv_object_params& p, const Plan& plan, uint32_t* ids,
                                ssrlcv_object_record* records, uint32_t capacity, hipStream_t st) {
  const uint32_t tilesX = (w + TX - 1u) / TX, tiles = tilesX * ((h + TY - 1u) / TY);  // below 2^20 + 2^11
  hipLaunchKernelGGL(k_obj_reduce, dim3(capped(tiles, kReduceGridCap)), dim3(256), 0, st, (const uint32_t*)objects, plan.labels, plan.counts, plan.number, w,
                     h, tilesX, tiles, p.minHeight, p.scale, p.minCells ? p.minCells : 1u, ids, records, capacity);
  return hipGetLastError();
}

}  // namespace svobj

#ifndef SSRLCV_OBJECTS_LAB
extern "C" {

size_t ssrlcv_hip_dsm_objects_workspace_bytes(uint32_t w, uint32_t h) {
  using namespace svobj;
  if (bad_size(w, h) || w == 0 || h == 0) return 0;
  return 3 * map_bytes(w * h) + compaction_bytes(w * h);
}

int ssrlcv_hip_dsm_objects(const float* objects, uint32_t w, uint32_t h, const ssrlcv_object_params* params, uint32_t* ids,
                           ssrlcv_object_record* records, uint32_t capacity, uint32_t* count_dev, void* workspace, size_t workspaceBytes,
                           ssrlcv_stream_t stream) {
  using namespace svobj;
  if (bad_params(params)) return SSRLCV_ERR_INVALID_ARG;
  if (bad_size(w, h)) return SSRLCV_ERR_UNSUPPORTED;
  if (!count_dev) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (w == 0 || h == 0) {  // no cell, no object; nothing else is looked at
    SSRLCV_HIP_TRY(hipMemsetAsync(count_dev, 0, 4, st));
    return SSRLCV_OK;
  }
  if (!objects || !workspace || (!records && capacity != 0) || ((uintptr_t)records & 7u)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_dsm_objects_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  const uint32_t n = w * h;
  const Plan plan(workspace, n);
  SSRLCV_HIP_TRY(launch_mask(objects, n, params->minHeight, plan, st));
  svcc::label_components((const float*)plan.number, w, h, params->maxDiff, plan.labels, plan.counts, st);
  SSRLCV_LAUNCH_CHECK();
  const ObjKeep keep{plan.labels, plan.counts, params->minCells ? params->minCells : 1u};
  const ObjEmit emit{plan.counts, plan.number, records, capacity};
  uint32_t* totals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(n, keep, emit, plan.tables, &totals, st)));
  SSRLCV_HIP_TRY(launch_reduce(objects, w, h, *params, plan, ids, records, capacity, st));
  const uint32_t most = capacity < n ? capacity : n;  // no more objects than cells
  hipLaunchKernelGGL(k_obj_finish, dim3(capped((most + 255u) / 256u + (most == 0u), kFinishGridCap)), dim3(256), 0, st, records, capacity, totals + 1, count_dev);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_object_measures_host(const ssrlcv_object_record* record, const ssrlcv_dsm_frame* frame, float scale, ssrlcv_object_measures* out) {
  if (!record || !out || !dsm::frame_ok(frame)) return SSRLCV_ERR_INVALID_ARG;
  if (!(scale > 0.0f && scale <= 3.4028234663852886e38f)) return SSRLCV_ERR_INVALID_ARG;
  if (record->cells == 0 || record->clipped > record->cells) return SSRLCV_ERR_INVALID_ARG;
  // the header's expressions in the header's order; -ffp-contract=off keeps every operation on its own
  ssrlcv_object_measures m;
  const double c = (double)frame->cell, s = (double)scale;
  const double n = (double)record->cells, cc = c * c;
  m.area = n * cc;
  m.perimeterLength = (double)record->perimeter * c;
  m.compactness = (12.566370614359172 * m.area) / (m.perimeterLength * m.perimeterLength);
  m.centroidX = (double)record->sumX / n;
  m.centroidY = (double)record->sumY / n;
  const double a = (m.centroidX + 0.5) * c, b = (m.centroidY + 0.5) * c;
  for (int k = 0; k < 3; ++k) m.world[k] = ((double)frame->origin[k] + a * (double)frame->ex[k]) + b * (double)frame->ey[k];
  const double part = (double)(record->cells - record->clipped), meanQ = (double)record->sumQ / part;
  m.meanHeight = meanQ / s;
  m.volume = ((double)record->sumQ / s) * cc;
  const double var = (double)record->sumQQ / part - meanQ * meanQ;
  m.rmsHeight = sqrt(var < 0.0 ? 0.0 : var) / s;
  m.mxx = (double)record->sumXX / n - m.centroidX * m.centroidX;
  m.mxy = (double)record->sumXY / n - m.centroidX * m.centroidY;
  m.myy = (double)record->sumYY / n - m.centroidY * m.centroidY;
  const double t = 0.5 * (m.mxx + m.myy), d = 0.5 * (m.mxx - m.myy), r = sqrt(d * d + m.mxy * m.mxy);
  m.lambdaMajor = t + r;
  const double l = t - r;
  m.lambdaMinor = l < 0.0 ? 0.0 : l;
  double vx = d >= 0.0 ? d + r : m.mxy, vy = d >= 0.0 ? m.mxy : r - d;
  if (vx < 0.0) {
    vx = -vx;
    vy = -vy;
  }
  const double g = sqrt(vx * vx + vy * vy);
  m.axisX = g > 0.0 ? vx / g : 1.0;
  m.axisY = g > 0.0 ? vy / g : 0.0;
  m.elongation = m.lambdaMinor > 0.0 ? sqrt(m.lambdaMajor / m.lambdaMinor) : m.lambdaMajor > 0.0 ? (double)INFINITY : 1.0;
  *out = m;
  return SSRLCV_OK;
}

}  // extern "C"
#endif
