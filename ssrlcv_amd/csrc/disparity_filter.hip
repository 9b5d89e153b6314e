// ssrlcv_amd/csrc/disparity_filter.hip -- the map-domain post-filters of the dense stereo chain: connected components of a
// disparity map (4-adjacent valid pixels whose disparities differ by at most maxDiff), the speckle filter that invalidates the
// components of at most maxSpeckleSize pixels, the lower median over the valid pixels of a 3 x 3 or 5 x 5 window, and hole
// filling from the nearest measured pixels along up to eight directions.
// The contract is include/ssrlcv_hip.h "disparity post-filters"; tests/speckle_ref.py restates it operation by operation.
// Hole filling is "hole filling" there and tests/fill_ref.py; its kernels (k_fill_rows, k_fill_march, k_fill_select) are
// described where they stand, below the median.
//
// Labelling is union-find, never label propagation: no pass is repeated until nothing changes, so a serpentine that crosses
// every tile costs what a blob costs.  `labels` is the parent array of one forest over the pixels; a parent is always a
// SMALLER raster index of the same component, so the root of a finished tree is the component's smallest index.
//
//   k_cc_tile     one block per 64 x 16 tile, a wave per row.  Row runs come from one ballot (a run's first lane is its head;
//                 every lane finds its head with a count of leading zeros), the rows of the tile are united through LDS with
//                 atomicMin, and every pixel leaves with its tile-local root as a global raster index.  The pixels of each
//                 tile-local component are counted in LDS -- one LDS add per row run -- and the count is STORED at the local
//                 root's entry of `counts`, 0 everywhere else: every entry is written, so the workspace may hold anything.
//   k_cc_seam     one lane per pixel of a tile's first column or first row: where it links to the pixel across the seam, the
//                 lock-free union(find(a), find(b)) that hangs the larger root under the smaller with atomicMin.
//                 A lane whose neighbour one step back along the seam already carries the same union leaves it to that lane,
//                 so a smooth surface costs one union per tile edge, not one per seam pixel; the finds start at the
//                 tile-local roots and shorten their paths.
//   k_cc_roots    the tile-local roots (the pixels with a count) to their final roots; one that is not the final root adds its
//                 count to the final root's: one global atomic per (tile, local component), not one per pixel.  Every other
//                 pixel still names its tile-local root, so its label is one more hop away: labels[labels[p]].
//   k_cc_sizes, k_speckle_apply   the streaming passes that take that hop: label(p) = labels[labels[p]], size(p) =
//                 counts[label(p)].
//   k_median<M>   a 64 x 16 tile and its halo in LDS, 4 pixels per lane; Batcher's odd-even merge sort as a fixed network on
//                 the integer keys, the missing entries at INT32_MAX, the rank chosen by the valid count.
//
// A stale read of a parent is harmless everywhere: any value an entry ever held is an ancestor of its pixel in the final
// forest (entries only ever decrease, along links).  The atomics decide at the L2, so a hook on a pixel that is no longer a
// root is seen by its return value and taken up from there.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "cc_label.h"
#include "device_math.h"
#include "order_key.h"

namespace {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kTileW = 64, kTileH = 16, kTilePixels = kTileW * kTileH;  // a wave is a row: k_cc_tile's ballots rely on kTileW == 64
constexpr int kRowsPerLane = kTilePixels / 256;

// item 1 of the contract: one float subtraction; false for a NaN, so an invalid pixel (a NaN) links to nothing
__device__ __forceinline__ bool linked(float a, float b, float maxDiff) { return fabsf(a - b) <= maxDiff; }

__device__ __forceinline__ uint32_t lds_find(const volatile uint32_t* L, uint32_t x) {
  uint32_t p;
  while ((p = L[x]) != x) x = p;
  return x;
}

__device__ __forceinline__ void lds_union(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&L[a], b);
    if (old == a) return;  // a was a root and hangs under b now
    a = old;               // somebody hooked a first: L[a] = min(old, b), and old and b are still to be united
  }
}

__device__ __forceinline__ uint32_t g_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t g_find(const uint32_t* L, uint32_t x) {
  uint32_t p;
  while ((p = g_load(L + x)) != x) x = p;
  return x;
}

// p and q are pixels on either side of a seam: their entries name their tile-local roots (or, once shortened, a root above)
__device__ __forceinline__ void g_union(uint32_t* L, uint32_t p, uint32_t q) {
  uint32_t a = g_load(L + p), b = g_load(L + q);
  const uint32_t a0 = a, b0 = b;
  for (;;) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a == b) break;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&L[a], b);
    if (old == a) {
      a = b;
      break;
    }
    a = old;
  }
  // a is above both tile-local roots in one tree now: shorten their paths for the finds behind this one, the other seam pixels
  // of the same two tiles first of all (a minimum with an ancestor is safe); a pixel's own entry is never touched
  if (a < a0) atomicMin(&L[a0], a);
  if (a < b0) atomicMin(&L[b0], a);
}

__global__ __launch_bounds__(256) void k_cc_tile(const float* __restrict__ disparity, uint32_t w, uint32_t h, uint32_t tilesX, float maxDiff,
                                                 uint32_t* __restrict__ labels, uint32_t* __restrict__ counts) {
  __shared__ float sd[kTilePixels];
  __shared__ uint32_t sl[kTilePixels];
  __shared__ uint32_t sc[kTilePixels];
  const uint32_t ty = blockIdx.x / tilesX, tx = blockIdx.x - ty * tilesX;
  const uint32_t x0 = tx * kTileW, y0 = ty * kTileH;
  const uint32_t lx = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t gx = x0 + lx;
  float d[kRowsPerLane];
  uint32_t runLength[kRowsPerLane];  // of the run this lane heads, else 0
  bool left[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const uint32_t ly = wave + 4u * j, gy = y0 + ly;
    d[j] = (gx < w && gy < h) ? disparity[(size_t)gy * w + gx] : __uint_as_float(kNaN);  // outside the image: invalid
    sd[ly * kTileW + lx] = d[j];
  }
  __syncthreads();
  // rows: a run is a maximal stretch of pixels each linked to its left neighbour; every lane points at its run's head
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const uint32_t ly = wave + 4u * j, i = ly * kTileW + lx;
    const bool valid = __float_as_uint(d[j]) != kNaN;
    left[j] = lx > 0 && linked(d[j], sd[i - 1], maxDiff);  // a linked neighbour is valid (its value is no NaN)
    const unsigned long long heads = __ballot(valid && !left[j]);
    const unsigned long long ends = heads | __ballot(!valid);
    uint32_t parent = kNone;
    runLength[j] = 0;
    if (valid) {
      const unsigned long long below = heads & ((2ull << lx) - 1ull);  // never 0: the run of a valid lane has a head at or below it
      parent = ly * kTileW + (63u - (uint32_t)__clzll((long long)below));
      if (!left[j]) {
        const unsigned long long above = lx < 63u ? ends >> (lx + 1u) : 0ull;
        runLength[j] = above ? (uint32_t)__ffsll((long long)above) : 64u - lx;
      }
    }
    sl[i] = parent;
    sc[i] = 0u;
  }
  __syncthreads();
  // columns: unite with the pixel above, unless the two pixels to the left already carry the same union
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const uint32_t ly = wave + 4u * j, i = ly * kTileW + lx;
    if (ly == 0 || !linked(d[j], sd[i - kTileW], maxDiff)) continue;
    if (left[j] && linked(sd[i - 1], sd[i - kTileW - 1], maxDiff) && linked(sd[i - kTileW], sd[i - kTileW - 1], maxDiff)) continue;
    lds_union(sl, i, i - kTileW);
  }
  __syncthreads();
  uint32_t root[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const uint32_t ly = wave + 4u * j, i = ly * kTileW + lx;
    root[j] = __float_as_uint(d[j]) != kNaN ? lds_find(sl, i) : kNone;
    if (runLength[j]) atomicAdd(&sc[root[j]], runLength[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const uint32_t ly = wave + 4u * j, i = ly * kTileW + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const uint32_t p = gy * w + gx;  // below 2^31
    labels[p] = root[j] == kNone ? kNone : (y0 + root[j] / kTileW) * w + x0 + (root[j] & 63u);
    counts[p] = root[j] == i ? sc[i] : 0u;
  }
}

// items 0 .. nV - 1: the first column of every tile column but the first, against the pixel to its left;
// items nV .. : the first row of every tile row but the first, against the pixel above
__global__ __launch_bounds__(256) void k_cc_seam(const float* __restrict__ disparity, uint32_t w, uint32_t nV, uint32_t items, uint32_t seamsX,
                                                 float maxDiff, uint32_t* labels) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  // p against q across the seam; s = the step back along the seam, 0 for the first pixel of a tile's edge
  uint32_t p, q, s;
  if (i < nV) {
    const uint32_t y = i / seamsX, k = i - y * seamsX;
    p = y * w + (k + 1u) * kTileW;
    q = p - 1u;
    s = y % kTileH ? w : 0u;
  } else {
    const uint32_t j = i - nV, k = j / w, x = j - k * w;
    p = (k + 1u) * kTileH * w + x;
    q = p - w;
    s = x % kTileW ? 1u : 0u;
  }
  const float dp = disparity[p], dq = disparity[q];
  if (!linked(dp, dq, maxDiff)) return;
  if (s) {
    // the pair one step back along the same edge of the same two tiles: if it is linked across the seam and each of its pixels
    // to the one here, inside its tile, then its lane carries this union (or hands it on the same way; the first pair never does)
    const float bp = disparity[p - s], bq = disparity[q - s];
    if (linked(bp, bq, maxDiff) && linked(dp, bp, maxDiff) && linked(dq, bq, maxDiff)) return;
  }
  g_union(labels, p, q);
}

// the tile-local roots (the pixels with a count) to their final roots, their counts with them; every other pixel still names
// its tile-local root, one hop below the final one
__global__ __launch_bounds__(256) void k_cc_roots(uint32_t* labels, uint32_t* counts, uint32_t n) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const uint32_t c = counts[p];
    if (c == 0u) continue;
    const uint32_t r = g_find(labels, p);
    if (r == p) continue;
    labels[p] = r;
    atomicAdd(&counts[r], c);  // only final roots are added to, and p is none
  }
}

// the last hop of every pixel, written back, and the sizes if they are asked for
__global__ __launch_bounds__(256) void k_cc_sizes(uint32_t* labels, const uint32_t* __restrict__ counts, uint32_t* __restrict__ sizes, uint32_t n) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const uint32_t l = labels[p];
    const uint32_t r = l == kNone ? kNone : labels[l];  // l is a tile-local root: its entry is final (and a final root names itself)
    if (r != l) labels[p] = r;
    if (sizes) sizes[p] = r == kNone ? 0u : counts[r];
  }
}

__global__ __launch_bounds__(256) void k_speckle_apply(float* __restrict__ disparity, uint32_t* __restrict__ cost, const uint32_t* __restrict__ labels,
                                                       const uint32_t* __restrict__ counts, uint32_t n, uint32_t maxSpeckleSize) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const uint32_t l = labels[p];
    if (l == kNone || counts[labels[l]] > maxSpeckleSize) continue;  // labels[l]: the last hop, from the tile-local root
    disparity[p] = __uint_as_float(kNaN);
    if (cost) cost[p] = kNone;
  }
}

// ---- median (order_key and sort_network: csrc/order_key.h)
template <int M>
__global__ __launch_bounds__(256) void k_median(const float* __restrict__ in, float* __restrict__ out, uint32_t w, uint32_t h, uint32_t tilesX) {
  constexpr int kHaloW = kTileW + 2 * M, kHaloH = kTileH + 2 * M, kWindow = (2 * M + 1) * (2 * M + 1);
  constexpr int kNet = kWindow <= 16 ? 16 : 32;
  __shared__ uint32_t sb[kHaloH * kHaloW];
  const uint32_t ty = blockIdx.x / tilesX, tx = blockIdx.x - ty * tilesX;
  const int x0 = (int)(tx * kTileW) - M, y0 = (int)(ty * kTileH) - M;
  for (int i = threadIdx.x; i < kHaloH * kHaloW; i += 256) {
    const int hy = i / kHaloW, hx = i - hy * kHaloW;
    const int gx = x0 + hx, gy = y0 + hy;
    sb[i] = (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) ? __float_as_uint(in[(size_t)gy * w + gx]) : kNaN;  // outside: not there
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int j = 0; j < kRowsPerLane; ++j) {
    const int ly = wave + 4 * j;
    const uint32_t gx = tx * kTileW + lx, gy = ty * kTileH + ly;
    if (gx >= w || gy >= h) continue;
    const uint32_t self = sb[(ly + M) * kHaloW + lx + M];
    int32_t a[kNet];
    int n = 0;
#pragma unroll
    for (int k = 0; k < kNet; ++k) {
      if (k < kWindow) {
        const uint32_t bits = sb[(ly + k / (2 * M + 1)) * kHaloW + lx + k % (2 * M + 1)];
        const bool valid = bits != kNaN;
        n += valid ? 1 : 0;
        a[k] = valid ? order_key(bits) : INT32_MAX;
      } else {
        a[k] = INT32_MAX;
      }
    }
    uint32_t result = kNaN;  // holes are never filled
    if (self != kNaN) {
      sort_network<kNet>(a);
      const int rank = (n - 1) / 2;  // the lower median of the n >= 1 valid values; at most (kWindow - 1) / 2
      int32_t key = a[0];
#pragma unroll
      for (int k = 1; k <= (kWindow - 1) / 2; ++k) key = rank == k ? a[k] : key;
      result = (uint32_t)order_key((uint32_t)key);
    }
    out[(size_t)gy * w + gx] = __uint_as_float(result);
  }
}

// ---- hole filling (include/ssrlcv_hip.h "hole filling"; tests/fill_ref.py restates it)
// Every selected direction gets a hit map in the workspace: at a hole, the first measured value upstream within maxGap steps,
// else the invalid pattern.  A carry along the line -- the last measured value and the steps since it -- makes that O(1) per
// pixel whatever the gap.  Only holes are stored to, and k_fill_select reads the maps only at holes, so the entries at measured
// pixels may hold anything.
struct FillDirs {
  uint32_t count;  // selected directions, in the order of the bits
  uint8_t dir[8];
};

// One lane per line of direction (DX, DY), DY != 0, a wave per block.  Step s of the march is row y = s (DY > 0) or h - 1 - s;
// line c is at x = c + DX s there, so the lanes of a wave read 64 neighbouring x of one row.  c runs over -(h - 1) .. w - 1 for
// DX = +1 (the lines with c < 0 start on the first column), 0 .. w + h - 2 for DX = -1, 0 .. w - 1 for a column.  A wave only
// walks the rows in which one of its lines is inside the image; a line enters once and leaves once, so a lane outside has
// nothing to carry.  The loads do not depend on the carry: kFillRows rows are in flight, loaded before the first is looked at.
//
// One wave per 64 lines is (w + h) / 64 waves per direction, each waiting for h / kFillRows round trips to memory one after the
// other: too few to fill the chip.  So the steps are cut into strips of `stripRows`, and a wave marches one strip of its lines.
// What a strip hands on is the carry itself -- the last measured value in it (the invalid pattern: none) and the steps since --
// so a first launch (kSummary) marches every strip but the last from an empty carry and stores no hit, only that pair; the
// second folds the pairs of the strips upstream of its own into its carry-in, at most strips - 1 coalesced loads that depend on
// the image's height and on nothing in it, and marches with the stores.
constexpr int kFillRows = 16;
constexpr uint32_t kFillStripRows = 128;  // the strips of a large map; a multiple of kFillRows
constexpr uint32_t kFillMaxStrips = 1024;

struct FillStrips {
  uint32_t rows, count;  // steps per strip, strips
  uint32_t* carries;     // [direction slot][strip < count - 1][line][value, steps]; lineStride lines, a multiple of 64
  uint32_t lineStride;
};

template <int DX, int DY, bool kSummary>
__device__ __forceinline__ void fill_march(const uint32_t* __restrict__ in, uint32_t* __restrict__ hit, long long w, long long h, uint32_t maxGap,
                                           long long block, uint32_t strip, const FillStrips& strips, uint32_t* __restrict__ carries) {
  const long long c0 = block * 64 - (DX > 0 ? h - 1 : 0);
  if (c0 >= (DX < 0 ? w + h - 1 : w)) return;
  const long long c = c0 + threadIdx.x;
  // the steps of this strip in which one of the wave's lines is inside the image
  long long sLo = (long long)strip * strips.rows, sHi = min(h, sLo + strips.rows) - 1;
  if (DX > 0) {
    sLo = max(sLo, -(c0 + 63));
    sHi = min(sHi, w - 1 - c0);
  } else if (DX < 0) {
    sLo = max(sLo, c0 - (w - 1));
    sHi = min(sHi, c0 + 63);
  }
  const size_t line = (size_t)block * 64 + threadIdx.x;  // below lineStride
  uint32_t value = kNaN, steps = 0;  // steps stays below w + h < 2^32: it cannot wrap, so it need not saturate
  if (!kSummary) {
#pragma unroll 8
    for (uint32_t k = 0; k < strip; ++k) {
      const uint32_t* e = carries + ((size_t)k * strips.lineStride + line) * 2;
      const uint32_t stripValue = e[0], stripSteps = e[1];
      steps = stripValue != kNaN ? stripSteps : steps + stripSteps;
      value = stripValue != kNaN ? stripValue : value;
    }
  }
  for (long long s = sLo; s <= sHi; s += kFillRows) {
    uint32_t v[kFillRows];
    size_t at[kFillRows];
    bool inside[kFillRows];
#pragma unroll
    for (int j = 0; j < kFillRows; ++j) {
      const long long sj = s + j, x = c + DX * sj;
      inside[j] = sj <= sHi && x >= 0 && x < w;
      // a lane outside loads the nearest pixel of the row inside instead (and drops it): no branch around the load
      const long long y = DY > 0 ? min(sj, sHi) : h - 1 - min(sj, sHi);
      at[j] = (size_t)(y * w + min(max(x, 0ll), w - 1));
      v[j] = in[at[j]];
    }
#pragma unroll
    for (int j = 0; j < kFillRows; ++j) {
      if (!inside[j]) continue;
      if (v[j] != kNaN) {
        value = v[j];
        steps = 0;
      } else {
        ++steps;
        if (!kSummary) hit[at[j]] = steps <= maxGap ? value : kNaN;  // value is the invalid pattern until the line has met a measured pixel
      }
    }
  }
  if (kSummary) {  // a wave with no step in this strip hands on (none, 0) like a lane that was outside throughout
    uint32_t* e = carries + ((size_t)strip * strips.lineStride + line) * 2;
    e[0] = value;
    e[1] = steps;
  }
}

// grid (blocks of 64 lines, strips -- all but the last for kSummary --, the selected non-horizontal directions)
template <bool kSummary>
__global__ __launch_bounds__(64) void k_fill_march(const uint32_t* __restrict__ in, uint32_t* __restrict__ hits, size_t mapStride, uint32_t w, uint32_t h,
                                                   uint32_t maxGap, FillDirs slots, FillDirs dirs, FillStrips strips) {
  const uint32_t dir = dirs.dir[blockIdx.z], strip = blockIdx.y;
  uint32_t* hit = hits + slots.dir[blockIdx.z] * mapStride;
  uint32_t* carries = strips.carries + (size_t)blockIdx.z * (strips.count - 1u) * strips.lineStride * 2;
  switch (dir) {
    case 2: fill_march<0, 1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
    case 3: fill_march<0, -1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
    case 4: fill_march<1, 1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
    case 5: fill_march<-1, 1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
    case 6: fill_march<1, -1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
    default: fill_march<-1, -1, kSummary>(in, hit, w, h, maxGap, blockIdx.x, strip, strips, carries); break;
  }
}

// The two horizontal directions: a wave per row, 64 pixels at a time in the direction of the carry (lane l is pixel 64 i + l
// from the row's upstream end).  Inside a chunk the last measured pixel below a lane comes from one ballot and one shuffle; the
// chunk's last measured value and its distance from the chunk's end are the carry into the next.
// grid (rows / 4, the selected horizontal directions)
__global__ __launch_bounds__(256) void k_fill_rows(const uint32_t* __restrict__ in, uint32_t* __restrict__ hits, size_t mapStride, uint32_t w, uint32_t h,
                                                   uint32_t maxGap, FillDirs slots, FillDirs dirs) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t y = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (y >= h) return;
  const bool mirrored = dirs.dir[blockIdx.y] == 1u;  // direction 1 carries from the right end to the left
  const uint32_t* row = in + y * w;
  uint32_t* hit = hits + slots.dir[blockIdx.y] * mapStride + y * w;
  uint32_t value = kNaN, steps = 0;  // of the chunks behind: the last measured value, its distance from the last chunk's end (below w + 64)
  for (uint32_t base = 0; base < w; base += 64u) {  // w < 2^31: base + 64 cannot wrap
    const uint32_t i = base + lane;
    const uint32_t x = mirrored ? w - 1u - i : i;
    const uint32_t v = i < w ? row[x] : kNaN;
    const unsigned long long measured = __ballot(v != kNaN);
    const unsigned long long below = measured & ((1ull << lane) - 1ull);
    const int source = below ? 63 - __clzll((long long)below) : 0;
    const uint32_t near = (uint32_t)__shfl((int)v, source);
    if (i < w && v == kNaN) {
      const uint32_t found = below ? near : value;
      const uint32_t t = below ? lane - (uint32_t)source : steps + lane + 1u;
      hit[x] = t <= maxGap ? found : kNaN;
    }
    if (measured) {
      const int top = 63 - __clzll((long long)measured);
      value = (uint32_t)__shfl((int)v, top);
      steps = 63u - (uint32_t)top;
    } else {
      steps += 64u;
    }
  }
}

// measured pixels pass through; a hole takes rank 0 or (n - 1) / 2 of the n hits its selected maps hold, if n >= minHits
__global__ __launch_bounds__(256) void k_fill_select(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint8_t* __restrict__ filled,
                                                     const uint32_t* __restrict__ hits, size_t mapStride, uint32_t n, uint32_t maps, uint32_t minHits,
                                                     uint32_t rule) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    uint32_t result = in[p];
    uint8_t mark = 0;
    if (result == kNaN) {
      int32_t a[8];
      int found = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t bits = (uint32_t)k < maps ? hits[k * mapStride + p] : kNaN;
        const bool valid = bits != kNaN;
        found += valid ? 1 : 0;
        a[k] = valid ? order_key(bits) : INT32_MAX;
      }
      if (found > 0 && (uint32_t)found >= minHits) {
        sort_network<8>(a);
        const int rank = rule ? (found - 1) / 2 : 0;
        int32_t key = a[0];
#pragma unroll
        for (int k = 1; k <= 3; ++k) key = rank == k ? a[k] : key;
        result = (uint32_t)order_key((uint32_t)key);
        mark = 1;
      }
    }
    out[p] = result;
    if (filled) filled[p] = mark;
  }
}

// ---- host side
bool too_many_pixels(uint32_t w, uint32_t h) { return (unsigned long long)w * h >= (1ull << 31); }

unsigned capped_blocks(uint32_t items) {
  const unsigned b = (unsigned)((items + 255u) / 256u);
  return b > 4096u ? 4096u : b;
}

uint32_t tiles_x(uint32_t w) { return (w + kTileW - 1u) / kTileW; }
uint32_t tiles_y(uint32_t h) { return (h + kTileH - 1u) / kTileH; }

// labels <- for a tile-local root the component's label, for every other pixel its tile-local root: the label is
// labels[labels[p]]; counts <- at every component's root its size
void label_components(const float* disparity, uint32_t w, uint32_t h, float maxDiff, uint32_t* labels, uint32_t* counts, hipStream_t stream) {
  const uint32_t tx = tiles_x(w), ty = tiles_y(h), n = w * h;
  hipLaunchKernelGGL(k_cc_tile, dim3(tx * ty), dim3(256), 0, stream, disparity, w, h, tx, maxDiff, labels, counts);
  const uint32_t nV = (tx - 1u) * h, nH = (ty - 1u) * w;  // together below w h / 16 + w h / 64
  if (nV + nH)
    hipLaunchKernelGGL(k_cc_seam, dim3((nV + nH + 255u) / 256u), dim3(256), 0, stream, disparity, w, nV, nV + nH, tx - 1u, maxDiff, labels);
  hipLaunchKernelGGL(k_cc_roots, dim3(capped_blocks(n)), dim3(256), 0, stream, labels, counts, n);
}

bool bad_max_diff(float maxDiff) { return !(maxDiff >= 0.0f); }  // a NaN or a negative number

}  // namespace

// the same labelling for objects.hip (cc_label.h)
namespace svcc {
static_assert(kTileW == ::kTileW && kTileH == ::kTileH, "cc_label.h names k_cc_tile's tile");
void label_components(const float* disparity, uint32_t w, uint32_t h, float maxDiff, uint32_t* labels, uint32_t* counts, hipStream_t stream) {
  ::label_components(disparity, w, h, maxDiff, labels, counts, stream);
}
}  // namespace svcc

extern "C" {

size_t ssrlcv_hip_disparity_components_workspace_bytes(uint32_t w, uint32_t h) {
  if (too_many_pixels(w, h)) return 0;
  return align256((size_t)4 * w * h);
}

int ssrlcv_hip_disparity_components(const float* disparity, uint32_t w, uint32_t h, float maxDiff, uint32_t* labels, uint32_t* sizes,
                                    void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (bad_max_diff(maxDiff) || too_many_pixels(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!disparity || !labels || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_disparity_components_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  uint32_t* counts = (uint32_t*)workspace;
  label_components(disparity, w, h, maxDiff, labels, counts, (hipStream_t)stream);
  const uint32_t n = w * h;
  hipLaunchKernelGGL(k_cc_sizes, dim3(capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, labels, counts, sizes, n);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_stereo_filter_speckles_workspace_bytes(uint32_t w, uint32_t h) {
  if (too_many_pixels(w, h)) return 0;
  return 2 * align256((size_t)4 * w * h);
}

int ssrlcv_hip_stereo_filter_speckles(float* disparity, uint32_t* cost, uint32_t w, uint32_t h, float maxDiff, uint32_t maxSpeckleSize,
                                      void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (bad_max_diff(maxDiff) || too_many_pixels(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!disparity || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_stereo_filter_speckles_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  if (maxSpeckleSize == 0) return SSRLCV_OK;  // every component has at least one pixel: nothing to remove
  const uint32_t n = w * h;
  uint32_t* labels = (uint32_t*)workspace;
  uint32_t* counts = (uint32_t*)((char*)workspace + align256((size_t)4 * n));
  label_components(disparity, w, h, maxDiff, labels, counts, (hipStream_t)stream);
  hipLaunchKernelGGL(k_speckle_apply, dim3(capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, disparity, cost, labels, counts, n, maxSpeckleSize);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_hip_stereo_filter_median(const float* in, float* out, uint32_t w, uint32_t h, uint32_t radius, ssrlcv_stream_t stream) {
  if (radius == 0 || too_many_pixels(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (radius > 2) return SSRLCV_ERR_UNSUPPORTED;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!in || !out || in == out) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t tx = tiles_x(w), ty = tiles_y(h);
  if (radius == 1)
    hipLaunchKernelGGL(k_median<1>, dim3(tx * ty), dim3(256), 0, (hipStream_t)stream, in, out, w, h, tx);
  else
    hipLaunchKernelGGL(k_median<2>, dim3(tx * ty), dim3(256), 0, (hipStream_t)stream, in, out, w, h, tx);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

static bool bad_fill_params(const ssrlcv_fill_params* p) {
  if (!p || p->paths == 0 || p->paths > 0xFFu) return true;
  return p->minHits == 0 || p->minHits > (uint32_t)__builtin_popcount(p->paths) || p->rule > 1;
}

size_t ssrlcv_hip_stereo_fill_holes_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_fill_params* params) {
  if (bad_fill_params(params) || too_many_pixels(w, h)) return 0;
  return (size_t)__builtin_popcount(params->paths) * align256((size_t)4 * w * h);
}

int ssrlcv_hip_stereo_fill_holes(const float* in, float* out, uint8_t* filled, uint32_t w, uint32_t h, const ssrlcv_fill_params* params,
                                 void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (bad_fill_params(params) || too_many_pixels(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!in || !out || !workspace || in == out) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_stereo_fill_holes_workspace_bytes(w, h, params)) return SSRLCV_ERR_WORKSPACE;
  const uint32_t n = w * h;
  const size_t mapStride = align256((size_t)4 * n) / 4;
  // slot = the direction's place among the selected ones; the horizontal directions share a launch, and so do the six others
  FillDirs rowDirs = {}, rowSlots = {}, marchDirs = {}, marchSlots = {};
  uint32_t maps = 0;
  for (uint32_t d = 0; d < 8; ++d) {
    if (!(params->paths >> d & 1u)) continue;
    FillDirs& dirs = d < 2 ? rowDirs : marchDirs;
    FillDirs& slots = d < 2 ? rowSlots : marchSlots;
    dirs.dir[dirs.count] = (uint8_t)d;
    slots.dir[dirs.count++] = (uint8_t)maps++;
  }
  const uint32_t* src = (const uint32_t*)in;
  uint32_t* hits = (uint32_t*)workspace;
  if (params->maxGap == 0) maps = 0;  // nothing is within 0 steps: no map is written and none is read
  if (maps && rowDirs.count)
    hipLaunchKernelGGL(k_fill_rows, dim3((h + 3u) / 4u, rowDirs.count), dim3(256), 0, (hipStream_t)stream, src, hits, mapStride, w, h, params->maxGap,
                       rowSlots, rowDirs);
  if (maps && marchDirs.count) {
    // strips of kFillStripRows steps, fewer and longer ones if their carries -- 8 bytes per direction, strip but the last and
    // line -- would not fit where they are kept: in `out`, which nothing else touches before k_fill_select writes every pixel
    const uint32_t lineBlocks = (uint32_t)(((size_t)w + h - 1u + 63u) / 64u);
    FillStrips strips = {kFillStripRows, (h + kFillStripRows - 1u) / kFillStripRows, (uint32_t*)out, lineBlocks * 64u};
    const size_t carryBytes = (size_t)marchDirs.count * strips.lineStride * 8u;  // of one strip
    const size_t most = std::min<size_t>(kFillMaxStrips, 1u + (size_t)4 * n / carryBytes);
    if (strips.count > most) {
      const size_t rows = ((size_t)h + most - 1u) / most;
      strips.rows = (uint32_t)((rows + kFillRows - 1u) / kFillRows * kFillRows);
      strips.count = (h + strips.rows - 1u) / strips.rows;
    }
    if (strips.count > 1u)
      hipLaunchKernelGGL(k_fill_march<true>, dim3(lineBlocks, strips.count - 1u, marchDirs.count), dim3(64), 0, (hipStream_t)stream, src, hits, mapStride,
                         w, h, params->maxGap, marchSlots, marchDirs, strips);
    hipLaunchKernelGGL(k_fill_march<false>, dim3(lineBlocks, strips.count, marchDirs.count), dim3(64), 0, (hipStream_t)stream, src, hits, mapStride, w, h,
                       params->maxGap, marchSlots, marchDirs, strips);
  }
  hipLaunchKernelGGL(k_fill_select, dim3(capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, src, (uint32_t*)out, filled, hits, mapStride, n, maps,
                     params->minHits, params->rule);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
