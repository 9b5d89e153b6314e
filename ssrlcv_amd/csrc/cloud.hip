// ssrlcv_amd/csrc/cloud.hip -- point-cloud stage after triangulation (MeshFactory's neighbour filter and normals): exact
// k-nearest neighbours over a uniform grid, the statistical neighbour-distance filter, and oriented normals.  The
// contract (neighbour key, float32 rounding sequence, statistics, normals) is stated in include/ssrlcv_hip.h and
// DESIGN.md section 4; it is this library's own (PARITY UNPINNED: upstream's Octree code has no fixture).
//
// Stream-ordered pipeline of ssrlcv_hip_knn (no host round trip):
//   k_bbox_cloud        bounding box of the finite points (order-preserving keys, atomicMax), finite count
//   k_cell_size         one thread: the cell size h (explicit, or from the box and n)
//   k_insert            hash every finite point's cell (63-bit packed key, 64-bit atomicCAS), per-slot counts.  With an
//                       automatic h it first runs once to count the occupied cells; k_resize_cells re-sizes h from that
//                       occupancy, and the table is cleared and built again
//   exclusive scan      slot starts (scan_lookback.h); k_scatter puts the points in cell-contiguous order
//   k_knn_grid<K>       THE HOT PATH: one lane per point in cell order, top-K (d2, j) keys in registers, rings of cells
//                       until the k-th key is below the guaranteed distance of every unsearched cell; queries still open
//                       after kRingCap rings, or at a scale where float32 products underflow, go to the far list
//   k_knn_far<K>        the far list, exactly: every finite point through LDS tiles, 8 waves per 64 queries
// Everything is keyed by (d2, j), so the result does not depend on h, on the order inside a cell or on scheduling.
#include <hip/hip_runtime.h>
#include <cmath>
#include "align256.h"
#include "device_math.h"
#include "scan_lookback.h"
#include "ssrlcv_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRingCap = 3;            // rings 0..kRingCap on the grid, then the far path
constexpr double kGridBoundMin = 0x1p-100;  // the grid's ring stop holds for squared distances from here up (k_knn_grid)
constexpr int kFarWaves = 8;          // waves sharing the 64 queries of a far block
constexpr int kFarTile = 256;          // points staged in LDS per wave and step of the far scan
constexpr uint32_t kAxisBits = 21;     // cell coordinate bits per axis of the packed key
constexpr double kMaxCellsPerAxis = 1048576.0;  // h >= largest extent / 2^20, so coordinates fit kAxisBits
constexpr unsigned long long kEmpty = ~0ull;    // a packed key has bit 63 clear
constexpr unsigned long long kNoNeighbour = (0x7f800000ull << 32) | 0xffffffffull;  // (+inf, UINT32_MAX)

// Workspace header (zeroed before use).  The box holds order-preserving keys: maxima as max(key), minima as max(~key).
struct CloudHdr {
  uint32_t boxMaxNot[3];
  uint32_t boxMax[3];
  uint32_t nFinite;
  uint32_t occupied;  // cells of the first automatic h
  uint32_t farCount;
  uint32_t cells[3];  // cells per axis at the final h
  double lo[3];
  double h;
};
constexpr size_t kHdrBytes = 256;
static_assert(sizeof(CloudHdr) <= kHdrBytes, "CloudHdr");

inline uint32_t table_log2(uint32_t n) {
  uint32_t l = 1;
  while ((1ull << l) < 2ull * n) ++l;
  return l;
}

struct KnnLayout {
  size_t keys, start, slot, rank, sorted, far, scan, total;
  uint32_t log2T, T;
};
inline KnnLayout knn_layout(uint32_t n) {
  KnnLayout L;
  L.log2T = table_log2(n ? n : 1);
  L.T = 1u << L.log2T;
  L.keys = kHdrBytes;
  L.start = L.keys + align256((size_t)L.T * 8);
  L.slot = L.start + align256(((size_t)L.T + 1) * 4);
  L.rank = L.slot + align256((size_t)n * 4);
  L.sorted = L.rank + align256((size_t)n * 4);
  L.far = L.sorted + align256((size_t)n * 16);
  L.scan = L.far + align256((size_t)n * 4);
  L.total = L.scan + svs::workspace_bytes<1>(svs::scan_tiles<8>(L.T + 1));
  return L;
}

__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fdekey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool finite3(const ssrlcv_float3& p) {
  return isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
}
__device__ __forceinline__ uint32_t hash_slot(unsigned long long key, uint32_t log2T) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2T));
}
__device__ __forceinline__ unsigned long long pack_cell(int64_t cx, int64_t cy, int64_t cz) {
  return (unsigned long long)cx | ((unsigned long long)cy << kAxisBits) | ((unsigned long long)cz << (2 * kAxisBits));
}
// the cell coordinate of a point along one axis, in float64 (the query's bound uses the same value)
__device__ __forceinline__ double cell_f(float x, double lo, double h) { return ((double)x - lo) / h; }
__device__ __forceinline__ int64_t cell_i(double f, uint32_t cells) {
  int64_t c = (int64_t)floor(f);
  return c < 0 ? 0 : c >= (int64_t)cells ? (int64_t)cells - 1 : c;
}
__device__ __forceinline__ unsigned long long point_cell(const ssrlcv_float3& p, const CloudHdr* h) {
  return pack_cell(cell_i(cell_f(p.x, h->lo[0], h->h), h->cells[0]), cell_i(cell_f(p.y, h->lo[1], h->h), h->cells[1]),
                   cell_i(cell_f(p.z, h->lo[2], h->h), h->cells[2]));
}
// the float32 squared distance of the contract: dx = p[j] - p[i], ((dx dx + dy dy) + dz dz), every step rounded
__device__ __forceinline__ float d2f(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
// (d2, j) as one 64-bit key: d2 >= 0, so its bits order as an unsigned integer
__device__ __forceinline__ unsigned long long nkey(float d2, uint32_t j) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | j;
}

// ---- top-K list in registers: keys ascending, fully unrolled compare-and-shift (no run-time index: no scratch)
template <int K>
struct TopK {
  unsigned long long key[K];
  unsigned long long kth;  // the k-th key (k <= K; run-time k)
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int t = 0; t < K; ++t) key[t] = kNoNeighbour;
    kth = kNoNeighbour;
  }
  __device__ __forceinline__ void insert(unsigned long long c, uint32_t k) {
#pragma unroll
    for (int t = K - 1; t >= 0; --t) {
      const bool shift = t > 0 && c < key[t > 0 ? t - 1 : 0];
      const bool here = c < key[t];
      key[t] = shift ? key[t > 0 ? t - 1 : 0] : here ? c : key[t];
    }
    if (k == (uint32_t)K) {
      kth = key[K - 1];
    } else {
#pragma unroll
      for (int t = 0; t < K; ++t)
        if ((uint32_t)t + 1 == k) kth = key[t];
    }
  }
  __device__ __forceinline__ void write(uint32_t i, uint32_t k, uint32_t* __restrict__ nbr, float* __restrict__ d2) const {
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if ((uint32_t)t < k) {
        nbr[(size_t)i * k + t] = (uint32_t)key[t];
        if (d2) d2[(size_t)i * k + t] = __uint_as_float((uint32_t)(key[t] >> 32));
      }
    }
  }
};

__global__ __launch_bounds__(kThreads) void k_bbox_cloud(const ssrlcv_float3* __restrict__ p, uint32_t n, CloudHdr* __restrict__ h) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t fin = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const ssrlcv_float3 q = p[i];
    if (!finite3(q)) continue;
    ++fin;
    lo[0] = fminf(lo[0], q.x), lo[1] = fminf(lo[1], q.y), lo[2] = fminf(lo[2], q.z);
    hi[0] = fmaxf(hi[0], q.x), hi[1] = fmaxf(hi[1], q.y), hi[2] = fmaxf(hi[2], q.z);
  }
  uint32_t kmn[3], kmx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    kmn[a] = ~fkey(lo[a]);
    kmx[a] = fkey(hi[a]);
    for (int o = 32; o > 0; o >>= 1) {
      kmn[a] = max(kmn[a], (uint32_t)__shfl_xor(kmn[a], o, 64));
      kmx[a] = max(kmx[a], (uint32_t)__shfl_xor(kmx[a], o, 64));
    }
  }
  fin = svs::wave_total(fin);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMax(&h->boxMaxNot[a], kmn[a]);
      atomicMax(&h->boxMax[a], kmx[a]);
    }
    atomicAdd(&h->nFinite, fin);
  }
}

__device__ void set_cells(CloudHdr* h, double cell, double maxE) {
  if (!(cell >= maxE / kMaxCellsPerAxis)) cell = maxE / kMaxCellsPerAxis;
  if (!(cell > 0) || !isfinite(cell)) cell = 1.0;
  h->h = cell;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double span = ((double)fdekey(h->boxMax[a]) - h->lo[a]) / cell;
    h->cells[a] = span >= 0 ? (uint32_t)floor(span) + 1 : 1u;  // no finite point: one (empty) cell
  }
}

// cellSize > 0: that (raised to largest extent / 2^20); 0: from the box and the finite count (first guess for a volume)
__global__ void k_cell_size(CloudHdr* h, float cellSize, uint32_t k) {
  double e[3], maxE = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    h->lo[a] = (double)fdekey(~h->boxMaxNot[a]);
    e[a] = (double)fdekey(h->boxMax[a]) - h->lo[a];
    if (!(e[a] >= 0)) e[a] = 0;  // no finite point: the box stays empty
    maxE = fmax(maxE, e[a]);
  }
  double cell = cellSize;
  if (!(cellSize > 0)) {
    const double nf = h->nFinite ? (double)h->nFinite : 1.0;
    const double s0 = fmax(e[0], fmax(e[1], e[2])), s2 = fmin(e[0], fmin(e[1], e[2])), s1 = e[0] + e[1] + e[2] - s0 - s2;
    if (s2 > 0) cell = cbrt(s0 * s1 * s2 * k / nf);
    else if (s1 > 0) cell = sqrt(s0 * s1 * k / nf);
    else cell = s0 * k / nf;
  }
  set_cells(h, cell, maxE);
}

// automatic h, second step: aim at k points per OCCUPIED cell (a terrain cloud is a sheet: occupancy grows as h^2)
__global__ void k_resize_cells(CloudHdr* h, uint32_t k) {
  double maxE = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) maxE = fmax(maxE, (double)fdekey(h->boxMax[a]) - h->lo[a]);
  if (!(maxE >= 0)) maxE = 0;
  const double occ = h->occupied ? (double)h->nFinite / h->occupied : (double)k;
  set_cells(h, h->h * sqrt((double)k / occ), maxE);
}

// insert the cell of every finite point; count_only: count the newly occupied cells (first automatic h)
__global__ __launch_bounds__(kThreads) void k_insert(const ssrlcv_float3* __restrict__ p, uint32_t n, CloudHdr* __restrict__ h,
                                                     unsigned long long* __restrict__ keys, uint32_t log2T,
                                                     uint32_t* __restrict__ slotCount, uint32_t* __restrict__ slotOf,
                                                     uint32_t* __restrict__ rankOf, int count_only) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t fresh = 0;
  if (i < n) {
    const ssrlcv_float3 q = p[i];
    if (finite3(q)) {
      const unsigned long long key = point_cell(q, h);
      const uint32_t mask = (1u << log2T) - 1;
      uint32_t s = hash_slot(key, log2T);
      while (true) {
        const unsigned long long prev = atomicCAS(&keys[s], kEmpty, key);
        if (prev == kEmpty) fresh = 1;
        if (prev == kEmpty || prev == key) break;
        s = (s + 1) & mask;
      }
      if (!count_only) {
        slotOf[i] = s;
        rankOf[i] = atomicAdd(&slotCount[s], 1u);
      }
    }
  }
  if (count_only) {
    fresh = svs::wave_total(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&h->occupied, fresh);
  }
}

// cell-contiguous order: (x, y, z, original index); non-finite points get their empty result here
__global__ __launch_bounds__(kThreads) void k_scatter(const ssrlcv_float3* __restrict__ p, uint32_t n, uint32_t k,
                                                      const uint32_t* __restrict__ start, const uint32_t* __restrict__ slotOf,
                                                      const uint32_t* __restrict__ rankOf, float4* __restrict__ sorted,
                                                      uint32_t* __restrict__ nbr, float* __restrict__ d2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ssrlcv_float3 q = p[i];
  if (finite3(q)) {
    sorted[start[slotOf[i]] + rankOf[i]] = make_float4(q.x, q.y, q.z, __uint_as_float(i));
  } else {
    for (uint32_t t = 0; t < k; ++t) {
      nbr[(size_t)i * k + t] = 0xffffffffu;
      if (d2) d2[(size_t)i * k + t] = INFINITY;
    }
  }
}

__device__ __forceinline__ bool find_cell(const unsigned long long* __restrict__ keys, uint32_t log2T, unsigned long long key,
                                          uint32_t& slot) {
  const uint32_t mask = (1u << log2T) - 1;
  uint32_t s = hash_slot(key, log2T);
  while (true) {
    const unsigned long long v = keys[s];
    if (v == key) {
      slot = s;
      return true;
    }
    if (v == kEmpty) return false;
    s = (s + 1) & mask;
  }
}

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn_grid(const float4* __restrict__ sorted, const unsigned long long* __restrict__ keys,
                                                       const uint32_t* __restrict__ start, uint32_t log2T,
                                                       CloudHdr* __restrict__ h, uint32_t k, uint32_t* __restrict__ far,
                                                       uint32_t* __restrict__ nbr, float* __restrict__ d2out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= h->nFinite) return;
  const float4 q = sorted[t];
  const uint32_t qi = __float_as_uint(q.w);
  const double cell = h->h;
  const double f[3] = {cell_f(q.x, h->lo[0], cell), cell_f(q.y, h->lo[1], cell), cell_f(q.z, h->lo[2], cell)};
  const uint32_t nc[3] = {h->cells[0], h->cells[1], h->cells[2]};
  const int64_t c[3] = {cell_i(f[0], nc[0]), cell_i(f[1], nc[1]), cell_i(f[2], nc[2])};
  TopK<K> top;
  top.init();
  bool done = false;
  for (int r = 0; r <= kRingCap && !done; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int64_t cz = c[2] + dz;
      if (cz < 0 || cz >= (int64_t)nc[2]) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int64_t cy = c[1] + dy;
        if (cy < 0 || cy >= (int64_t)nc[1]) continue;
        const bool face = dz == -r || dz == r || dy == -r || dy == r;
        const int step = face || r == 0 ? 1 : 2 * r;  // inside the shell's yz-rim only dx = -r and dx = r are on it
        for (int dx = -r; dx <= r; dx += step) {
          const int64_t cx = c[0] + dx;
          if (cx < 0 || cx >= (int64_t)nc[0]) continue;
          uint32_t s;
          if (!find_cell(keys, log2T, pack_cell(cx, cy, cz), s)) continue;
          const uint32_t e = start[s + 1];
          for (uint32_t j = start[s]; j < e; ++j) {
            const float4 c4 = sorted[j];
            const uint32_t ci = __float_as_uint(c4.w);
            const unsigned long long key = nkey(d2f(q.x, q.y, q.z, c4.x, c4.y, c4.z), ci);
            if (key < top.kth && ci != qi) top.insert(key, k);
          }
        }
      }
    }
    // every unsearched cell lies beyond the faces of the searched (2r+1)^3 block: the query's distance to the nearest
    // face, less a margin for the float64 cell coordinates, is a lower bound D of the true squared distance of every
    // point in them.  The float32 d2 of the contract is at least (1 - 5 2^-24) of the true one (the difference, the
    // product and two sums, each within 2^-24 relative) ONLY WHILE NOTHING UNDERFLOWS: a product below 2^-126 is rounded
    // to a multiple of 2^-149, and below 2^-150 to 0, so at tiny scales the float32 key stops following the distance
    // (at 2^-80 every d2 is 0 and the contract's answer is the k lowest indices).  With D >= 2^-100 the largest of the
    // three products is at least 2^-102, normal like every sum it enters, and the two others lose at most 2^-150 each:
    // d2 >= D (1 - 5 2^-24) - 2^-149 >= D (1 - 5 2^-24 - 2^-49) > D (1 - 1e-6).  So the ring stop is taken only with
    // bound >= kGridBoundMin; below it the query goes to the far scan, which evaluates the key itself and is exact at
    // every scale.  (Overflow needs no guard: d2 = +inf is above every bound.)
    double gap = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double lo = f[a] - (double)(c[a] - r), hi = (double)(c[a] + r + 1) - f[a];
      // a face at the edge of the grid has no cell behind it
      if (c[a] - r > 0) gap = fmin(gap, lo);
      if (c[a] + r + 1 < (int64_t)nc[a]) gap = fmin(gap, hi);
    }
    gap = fmax(gap - 1e-6, 0.0) * cell;
    const double bound = gap * gap * (1.0 - 1e-6);
    done = bound >= kGridBoundMin && (double)__uint_as_float((uint32_t)(top.kth >> 32)) < bound;
  }
  if (!done) {
    far[atomicAdd(&h->farCount, 1u)] = qi;
    return;
  }
  top.write(qi, k, nbr, d2out);
}

// the far list: every finite point, exactly: the key of the contract is evaluated for every pair, so underflow (d2
// subnormal or 0) and overflow (d2 = +inf) order as the contract says, with no distance argument.  A block takes 64 queries (one per lane) and kFarWaves waves: wave w scans
// tiles w, w + kFarWaves, ... of the cell-ordered points through its own LDS tile (every lane reads the same point: an
// LDS broadcast), then the waves' lists are merged into wave 0's through LDS.  The split keeps the GPU busy when only
// a few thousand queries are far.
template <int K>
__global__ __launch_bounds__(kFarWaves * 64) void k_knn_far(const float4* __restrict__ sorted, const ssrlcv_float3* __restrict__ p,
                                                            const CloudHdr* __restrict__ h, uint32_t k, const uint32_t* __restrict__ far,
                                                            uint32_t* __restrict__ nbr, float* __restrict__ d2out) {
  static_assert(kFarWaves * kFarTile * sizeof(float4) >= 64 * K * sizeof(unsigned long long), "merge buffer");
  __shared__ float4 tiles[kFarWaves * kFarTile];
  const uint32_t nFar = h->farCount, nf = h->nFinite;
  const uint32_t b0 = blockIdx.x * 64;
  if (b0 >= nFar) return;  // block-uniform
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t = b0 + lane;
  const bool active = t < nFar;
  const uint32_t qi = active ? far[t] : 0;
  const ssrlcv_float3 q = p[qi];
  float4* tile = tiles + wave * kFarTile;
  TopK<K> top;
  top.init();
  for (uint32_t round = 0; round < nf; round += kFarWaves * kFarTile) {  // the same trip count for every wave
    const uint32_t base = round + wave * kFarTile;
    __syncthreads();
    for (uint32_t l = lane; l < kFarTile; l += 64)
      if (base + l < nf) tile[l] = sorted[base + l];
    __syncthreads();
    const uint32_t m = base >= nf ? 0u : nf - base < (uint32_t)kFarTile ? nf - base : (uint32_t)kFarTile;
    for (uint32_t l = 0; l < m; ++l) {
      const float4 c4 = tile[l];
      const uint32_t ci = __float_as_uint(c4.w);
      const unsigned long long key = nkey(d2f(q.x, q.y, q.z, c4.x, c4.y, c4.z), ci);
      if (key < top.kth && ci != qi) top.insert(key, k);
    }
  }
  unsigned long long* buf = (unsigned long long*)tiles;  // [K][64]
  for (uint32_t w = 1; w < (uint32_t)kFarWaves; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int e = 0; e < K; ++e) buf[e * 64 + lane] = top.key[e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int e = 0; e < K; ++e) {
        const unsigned long long key = buf[e * 64 + lane];
        if (key < top.kth) top.insert(key, k);
      }
    }
  }
  if (wave == 0 && active) top.write(qi, k, nbr, d2out);
}

// ---- statistical filter ------------------------------------------------------------------------------------------
constexpr uint32_t kStatBlocks = 512;  // fixed partition: block b sums points [b n / 512, (b + 1) n / 512)

struct FilterLayout {
  size_t partial, mean, scan, total;
};
inline FilterLayout filter_layout(uint32_t n) {
  FilterLayout L;
  L.partial = kHdrBytes;
  L.mean = L.partial + align256((size_t)kStatBlocks * 3 * sizeof(double));
  L.scan = L.mean + align256((size_t)n * sizeof(float));
  L.total = L.scan + svs::workspace_bytes<1>(svs::scan_tiles<8>(n));
  return L;
}

// fixed tree over the 256 threads of a block (every thread's v in, the block's sum in thread 0)
__device__ __forceinline__ double block_sum_fixed(double v) {
  __shared__ double s[kThreads];
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < (unsigned)w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// m_i = (sqrtf(d2_1) + ... + sqrtf(d2_k)) / k; pass 0: per-block sum of the finite m_i and their count; pass 1: per-block
// sum of (m_i - mu)^2.  Thread j of block b takes the points b0 + j, b0 + j + 256, ... of the block's fixed range.
__global__ __launch_bounds__(kThreads) void k_mean_stats(const float* __restrict__ d2, uint32_t n, uint32_t k, float* __restrict__ mean,
                                                         double* __restrict__ partial, const double* __restrict__ stats, int pass) {
  const uint32_t b0 = (uint32_t)((uint64_t)blockIdx.x * n / kStatBlocks), b1 = (uint32_t)((uint64_t)(blockIdx.x + 1) * n / kStatBlocks);
  double acc = 0, cnt = 0;
  const double mu = pass ? stats[0] : 0.0;
  for (uint32_t i = b0 + threadIdx.x; i < b1; i += kThreads) {
    float m;
    if (pass == 0) {
      float s = 0.f;
      for (uint32_t t = 0; t < k; ++t) s = s + sqrtf(d2[(size_t)i * k + t]);  // correctly rounded (HIP's default)
      m = s / (float)k;
      mean[i] = m;
    } else {
      m = mean[i];
    }
    if (isfinite(m)) {
      const double dm = (double)m - mu;
      acc += pass ? dm * dm : (double)m;
      cnt += 1.0;
    }
  }
  acc = block_sum_fixed(acc);
  cnt = block_sum_fixed(cnt);
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 3 + pass] = acc;
    if (pass == 0) partial[blockIdx.x * 3 + 2] = cnt;
  }
}

// one block: the partials in a fixed tree -> stats {mu, std, t}
__global__ __launch_bounds__(kThreads) void k_stats_reduce(const double* __restrict__ partial, double* __restrict__ stats, float sigma,
                                                           int pass) {
  double a = 0, c = 0;
  for (uint32_t b = threadIdx.x; b < kStatBlocks; b += kThreads) {
    a += partial[b * 3 + pass];
    c += partial[b * 3 + 2];
  }
  a = block_sum_fixed(a);
  c = block_sum_fixed(c);
  if (threadIdx.x == 0) {
    if (c == 0) {
      stats[0] = stats[1] = stats[2] = 0.0;
    } else if (pass == 0) {
      stats[0] = a / c;
    } else {
      stats[1] = sqrt(a / c);
      stats[2] = stats[0] + (double)sigma * stats[1];
    }
  }
}

// the kept points in input order: one look-back pass (scan_lookback.h), 8 points per thread
constexpr uint32_t kItems = 8;
__global__ __launch_bounds__(kThreads) void k_filter_compact(const ssrlcv_float3* __restrict__ p, uint32_t n, const float* __restrict__ mean,
                                                             const double* __restrict__ stats, const float* __restrict__ nIn,
                                                             ssrlcv_float3* __restrict__ pOut, uint32_t* __restrict__ idxOut,
                                                             float* __restrict__ nOut, uint32_t* __restrict__ count,
                                                             svs::TileScan<1> ts) {
  const double t = stats[2];
  uint32_t keep;
  auto read = [&](uint32_t base, uint32_t (&mine)[1]) {
    keep = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      if (base + j < n) {
        const float m = mean[base + j];
        if (isfinite(m) && (double)m <= t) keep |= 1u << j;
      }
    }
    mine[0] = __popc(keep);
  };
  auto write = [&](uint32_t base, const uint32_t (&at)[1]) {
    uint32_t o = at[0];
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      if (keep & (1u << j)) {
        const uint32_t i = base + j;
        pOut[o] = p[i];
        idxOut[o] = i;
        if (nOut) {
          nOut[3 * (size_t)o] = nIn[3 * (size_t)i];
          nOut[3 * (size_t)o + 1] = nIn[3 * (size_t)i + 1];
          nOut[3 * (size_t)o + 2] = nIn[3 * (size_t)i + 2];
        }
        ++o;
      }
    }
  };
  auto finish = [&](const uint32_t (&totals)[1]) { *count = totals[0]; };
  svs::for_each_tile<1, kItems>(ts, read, write, finish);
}

// ---- normals: covariance of the k + 1 points about their mean (float64), cyclic Jacobi, smallest eigenvector -------
constexpr int kJacobiSweeps = 10;

__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3], int p, int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
  for (int r = 0; r < 3; ++r) {  // A <- A J
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = c * arp - s * arq;
    A[r][q] = s * arp + c * arq;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {  // A <- J^T A
    const double apr = A[p][r], aqr = A[q][r];
    A[p][r] = c * apr - s * aqr;
    A[q][r] = s * apr + c * aqr;
  }
  A[p][q] = A[q][p] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {  // V <- V J
    const double vrp = V[r][p], vrq = V[r][q];
    V[r][p] = c * vrp - s * vrq;
    V[r][q] = s * vrp + c * vrq;
  }
}

__global__ __launch_bounds__(kThreads) void k_normals(const ssrlcv_float3* __restrict__ p, uint32_t n, const uint32_t* __restrict__ nbr,
                                                      uint32_t k, double vx, double vy, double vz, float* __restrict__ normals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ssrlcv_float3 q = p[i];
  double nrm[3] = {0, 0, 0};
  bool ok = finite3(q);
  // shifted by p_i: the differences of two floats are exact in float64, and k + 1 coincident points give exactly zero
  double m[3] = {0, 0, 0};
  for (uint32_t t = 0; t < k && ok; ++t) {
    const uint32_t j = nbr[(size_t)i * k + t];
    if (j >= n) {
      ok = false;
      break;
    }
    const ssrlcv_float3 c = p[j];
    m[0] += (double)c.x - q.x, m[1] += (double)c.y - q.y, m[2] += (double)c.z - q.z;
  }
  if (ok) {
    const double inv = 1.0 / (double)(k + 1);
    m[0] *= inv, m[1] *= inv, m[2] *= inv;
    double A[3][3];  // point i itself (shifted: the origin) first, then its neighbours
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) A[a][b] = m[a] * m[b];
    for (uint32_t t = 0; t < k; ++t) {
      const ssrlcv_float3 c = p[nbr[(size_t)i * k + t]];
      const double d[3] = {(double)c.x - q.x - m[0], (double)c.y - q.y - m[1], (double)c.z - q.z - m[2]};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) A[a][b] += d[a] * d[b];
    }
    A[1][0] = A[0][1], A[2][0] = A[0][2], A[2][1] = A[1][2];
    if (A[0][0] + A[1][1] + A[2][2] > 0) {
      double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
      for (int s = 0; s < kJacobiSweeps; ++s) {
        jacobi_rotate(A, V, 0, 1);
        jacobi_rotate(A, V, 0, 2);
        jacobi_rotate(A, V, 1, 2);
      }
      // the smallest diagonal entry (lowest index on ties), selected without a run-time register index
      const bool s1 = A[1][1] < A[0][0], s2 = A[2][2] < (s1 ? A[1][1] : A[0][0]);
      double e[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) e[r] = s2 ? V[r][2] : s1 ? V[r][1] : V[r][0];
      const double l = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      const double dot = e[0] * (vx - q.x) + e[1] * (vy - q.y) + e[2] * (vz - q.z);
      const double sg = dot < 0 ? -1.0 / l : 1.0 / l;
      nrm[0] = e[0] * sg, nrm[1] = e[1] * sg, nrm[2] = e[2] * sg;
    }
  }
  normals[3 * (size_t)i] = (float)nrm[0];
  normals[3 * (size_t)i + 1] = (float)nrm[1];
  normals[3 * (size_t)i + 2] = (float)nrm[2];
}

template <int K>
void launch_search(const KnnLayout& L, char* ws, const ssrlcv_float3* points, uint32_t n, uint32_t k, uint32_t* nbr, float* d2,
                   hipStream_t st) {
  CloudHdr* h = (CloudHdr*)ws;
  const float4* sorted = (const float4*)(ws + L.sorted);
  const uint32_t* far = (const uint32_t*)(ws + L.far);
  hipLaunchKernelGGL(k_knn_grid<K>, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, sorted,
                     (const unsigned long long*)(ws + L.keys), (const uint32_t*)(ws + L.start), L.log2T, h, k,
                     (uint32_t*)(ws + L.far), nbr, d2);
  hipLaunchKernelGGL(k_knn_far<K>, dim3((n + 63) / 64), dim3(kFarWaves * 64), 0, st, sorted, points, h, k, far, nbr, d2);
}

}  // namespace

extern "C" {

size_t ssrlcv_hip_knn_workspace_bytes(uint32_t numPoints, uint32_t k) {
  (void)k;
  return knn_layout(numPoints).total;
}

int ssrlcv_hip_knn(const ssrlcv_float3* points, uint32_t numPoints, uint32_t k, float cellSize, uint32_t* neighbors,
                   float* dist2, uint32_t* farQueries, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!points || !neighbors || !workspace || k < 1 || k > SSRLCV_KNN_MAX_K || numPoints < k + 1 || !(cellSize >= 0) ||
      !std::isfinite(cellSize) || numPoints > (1u << 30))
    return SSRLCV_ERR_INVALID_ARG;
  const KnnLayout L = knn_layout(numPoints);
  if (workspaceBytes < L.total) return SSRLCV_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CloudHdr* h = (CloudHdr*)ws;
  unsigned long long* keys = (unsigned long long*)(ws + L.keys);
  uint32_t* start = (uint32_t*)(ws + L.start);
  uint32_t* slotOf = (uint32_t*)(ws + L.slot);
  uint32_t* rankOf = (uint32_t*)(ws + L.rank);
  const uint32_t n = numPoints, blocks = (n + kThreads - 1) / kThreads;
  const uint32_t boxBlocks = blocks < 1024 ? blocks : 1024;
  SSRLCV_HIP_TRY(hipMemsetAsync(h, 0, kHdrBytes, st));
  SSRLCV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)L.T * 8, st));
  hipLaunchKernelGGL(k_bbox_cloud, dim3(boxBlocks), dim3(kThreads), 0, st, points, n, h);
  hipLaunchKernelGGL(k_cell_size, dim3(1), dim3(1), 0, st, h, cellSize, k);
  SSRLCV_LAUNCH_CHECK();
  if (cellSize == 0.0f) {
    hipLaunchKernelGGL(k_insert, dim3(blocks), dim3(kThreads), 0, st, points, n, h, keys, L.log2T, nullptr, nullptr, nullptr, 1);
    hipLaunchKernelGGL(k_resize_cells, dim3(1), dim3(1), 0, st, h, k);
    SSRLCV_LAUNCH_CHECK();
    SSRLCV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)L.T * 8, st));
  }
  SSRLCV_HIP_TRY(hipMemsetAsync(start, 0, ((size_t)L.T + 1) * 4, st));
  hipLaunchKernelGGL(k_insert, dim3(blocks), dim3(kThreads), 0, st, points, n, h, keys, L.log2T, start, slotOf, rankOf, 0);
  SSRLCV_LAUNCH_CHECK();
  SSRLCV_HIP_TRY(svs::exclusive_scan<8>(start, start, L.T + 1, ws + L.scan, st));
  hipLaunchKernelGGL(k_scatter, dim3(blocks), dim3(kThreads), 0, st, points, n, k, start, slotOf, rankOf,
                     (float4*)(ws + L.sorted), neighbors, dist2);
  SSRLCV_LAUNCH_CHECK();
  if (k <= 8) launch_search<8>(L, ws, points, n, k, neighbors, dist2, st);
  else if (k <= 16) launch_search<16>(L, ws, points, n, k, neighbors, dist2, st);
  else launch_search<32>(L, ws, points, n, k, neighbors, dist2, st);
  SSRLCV_LAUNCH_CHECK();
  if (farQueries) SSRLCV_HIP_TRY(hipMemcpyAsync(farQueries, &h->farCount, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

size_t ssrlcv_hip_neighbor_filter_workspace_bytes(uint32_t numPoints, uint32_t k) {
  (void)k;
  return filter_layout(numPoints).total;
}

int ssrlcv_hip_neighbor_distance_filter(const ssrlcv_float3* points, uint32_t numPoints, const float* dist2, uint32_t k,
                                        float sigma, float* meanDist, double* stats, ssrlcv_float3* pointsOut,
                                        uint32_t* indexOut, const float* normalsIn, float* normalsOut, uint32_t* count,
                                        void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!points || !dist2 || !stats || !pointsOut || !indexOut || !count || !workspace || k < 1 || k > SSRLCV_KNN_MAX_K ||
      numPoints < k + 1 || !std::isfinite(sigma) || (!normalsIn != !normalsOut) || numPoints > (1u << 30))
    return SSRLCV_ERR_INVALID_ARG;
  const FilterLayout L = filter_layout(numPoints);
  if (workspaceBytes < L.total) return SSRLCV_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* partial = (double*)(ws + L.partial);
  float* mean = meanDist ? meanDist : (float*)(ws + L.mean);
  hipLaunchKernelGGL(k_mean_stats, dim3(kStatBlocks), dim3(kThreads), 0, st, dist2, numPoints, k, mean, partial, stats, 0);
  hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(kThreads), 0, st, partial, stats, sigma, 0);
  hipLaunchKernelGGL(k_mean_stats, dim3(kStatBlocks), dim3(kThreads), 0, st, dist2, numPoints, k, mean, partial, stats, 1);
  hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(kThreads), 0, st, partial, stats, sigma, 1);
  SSRLCV_LAUNCH_CHECK();
  SSRLCV_HIP_TRY(svs::launch_tiles<1>(k_filter_compact, svs::scan_tiles<kItems>(numPoints), ws + L.scan, st, points, numPoints, mean,
                                       (const double*)stats, normalsIn, pointsOut, indexOut, normalsOut, count));
  return SSRLCV_OK;
}

int ssrlcv_hip_point_normals(const ssrlcv_float3* points, uint32_t numPoints, const uint32_t* neighbors, uint32_t k,
                             ssrlcv_float3 viewpoint, float* normals, ssrlcv_stream_t stream) {
  if (!points || !neighbors || !normals || k < 1 || k > SSRLCV_KNN_MAX_K || numPoints < k + 1 ||
      !std::isfinite(viewpoint.x) || !std::isfinite(viewpoint.y) || !std::isfinite(viewpoint.z))
    return SSRLCV_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_normals, dim3((numPoints + kThreads - 1) / kThreads), dim3(kThreads), 0, st, points, numPoints,
                     neighbors, k, (double)viewpoint.x, (double)viewpoint.y, (double)viewpoint.z, normals);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
