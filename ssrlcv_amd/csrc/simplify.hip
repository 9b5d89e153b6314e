// ssrlcv_amd/csrc/simplify.hip -- error-bounded right-triangle simplification of a height map's grid mesh for gfx950.  The contract
// is include/ssrlcv_hip.h "surface simplification"; tests/simplify_ref.py restates it.  Everything is a selection over the existing
// nodes, one fixed-order float32 expression a node and `max`, which commutes: bit-equal run to run.
//
//   k_level          one half-level (A or D) of the lattice of side 2^k, a thread a node of it, heights and errors from memory:
//                    the A-nodes of a level read the D-nodes of the level below, its D-nodes its A-nodes, so a level is two
//                    launches while its lattice has more than 4096 nodes
//   k_upper_tail     the remaining levels in ONE block, a barrier between half-levels, and +inf at the domain's corners
//                    E(m) is the maximum of e over m's descendants, and they reach 3 2^k nodes from a D-node of level k: a tile
//                    cannot finish its own levels from its own nodes.  The form that runs the two finest levels of 64 x 64 nodes
//                    and a halo of 8 in LDS is bit-equal and lost the A/B on every map (0.45 against 0.23 ms at 4096^2,
//                    profiles/simplify_bench.txt); it lives in tools/simplify_lab.hip, which includes this file.
//   SimpKeep / SimpEmit + compact.h   the triangle list: candidate id = Y 2w + 2 xi + s walks the doubled raster, a node row (Y
//                    even, node xi, apex s) then a cell row (Y odd, cell xi, apex s).  The emit writes the corners' RASTER
//                    indices and marks them kept in vertexIndex (idempotent stores of one value), whether or not the record fits
//   KeptKeep / KeptRank + compact.h   the rank of every kept node in raster order, and `kept`
//   k_remap          the written records' raster indices -> vertex ranks
// Every output word has one writer but the kept marks, which are stores of one value: no atomics, and no block waits for another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "compact.h"
#include "device_math.h"

namespace svsimp {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kInf = 0x7F800000u;
constexpr uint32_t kMark = 0u;        // vertexIndex of a kept node between the triangle pass and the ranking
constexpr uint32_t kPerThread = 16;   // compact.h: a wave owns a run of 1024 elements, a block 4096
constexpr uint32_t kTailNodes = 4096;  // a half-level of at most this many lattice nodes runs in the one-block tail

struct Dom {
  uint32_t w, h;
  int L;       // 2^L >= max(w - 1, h - 1, 1)
  uint32_t S;  // 2^L
  __host__ __device__ bool in_grid(int x, int y) const { return (uint32_t)x < w && (uint32_t)y < h; }
  __host__ __device__ bool in_domain(int x, int y) const { return (uint32_t)x <= S && (uint32_t)y <= S; }
  __host__ __device__ size_t at(int x, int y) const { return (size_t)y * w + (size_t)x; }
};

inline Dom make_dom(uint32_t w, uint32_t h) {
  uint32_t m = (w > h ? w : h);
  m = m > 2 ? m - 1 : 1;
  int L = 0;
  while ((1u << L) < m) ++L;
  return Dom{w, h, L, 1u << L};
}

// min(tz(x), tz(y)) with tz(0) = infinity (32 here: above every L)
__host__ __device__ inline int node_k(uint32_t x, uint32_t y) {
  const uint32_t v = x | y;
  return v ? __builtin_ctz(v) : 32;
}

// hypotenuse a-b and the two apexes of split node (x, y) of level k = node_k(x, y), the apexes ascending in (y, x)
struct Split {
  int ax, ay, bx, by, cx[2], cy[2];
  bool dnode;
};
__host__ __device__ inline Split split_of(int x, int y, int k) {
  const int u = 1 << k;
  const bool ox = (x >> k) & 1, oy = (y >> k) & 1;  // odd multiples of u: tz == k
  Split s;
  s.dnode = ox && oy;
  if (s.dnode) {
    const bool main = ((((x - u) >> (k + 1)) + ((y - u) >> (k + 1))) & 1) == 0;
    if (main) {
      s.ax = x - u; s.ay = y - u; s.bx = x + u; s.by = y + u;
      s.cx[0] = x + u; s.cy[0] = y - u; s.cx[1] = x - u; s.cy[1] = y + u;
    } else {
      s.ax = x + u; s.ay = y - u; s.bx = x - u; s.by = y + u;
      s.cx[0] = x - u; s.cy[0] = y - u; s.cx[1] = x + u; s.cy[1] = y + u;
    }
  } else if (ox) {  // tz(x) < tz(y): the edge runs along x
    s.ax = x - u; s.ay = y; s.bx = x + u; s.by = y;
    s.cx[0] = x; s.cy[0] = y - u; s.cx[1] = x; s.cy[1] = y + u;
  } else {
    s.ax = x; s.ay = y - u; s.bx = x; s.by = y + u;
    s.cx[0] = x - u; s.cy[0] = y; s.cx[1] = x + u; s.cy[1] = y;
  }
  return s;
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// e(m): hbits(x, y) gives a node's height bits, 0x7FC00000 for a node that is not present
template <typename HF>
__device__ __forceinline__ uint32_t node_e(const Dom& d, int x, int y, int k, const Split& s, HF hbits) {
  const uint32_t hm = hbits(x, y), ha = hbits(s.ax, s.ay), hb = hbits(s.bx, s.by);
  bool ok = hm != kNaN && ha != kNaN && hb != kNaN;
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (d.in_domain(s.cx[q], s.cy[q])) ok = ok && hbits(s.cx[q], s.cy[q]) != kNaN;
  if (!ok) return kInf;
  const float mid = (__uint_as_float(ha) + __uint_as_float(hb)) * 0.5f;
  const float e = fabsf(__uint_as_float(hm) - mid);
  return e < __uint_as_float(kInf) ? __float_as_uint(e) : kInf;  // a NaN becomes +inf; fabsf leaves no -0
}

// the maximum of E over the children: ebits(x, y) gives a child's E bits (+inf outside the grid; 0 for one that is another's to add)
template <typename EF>
__device__ __forceinline__ uint32_t children_max(const Dom& d, int x, int y, int k, bool dnode, EF ebits) {
  uint32_t m = 0;
  if (dnode) {
    const int u = 1 << k;
    m = umax(umax(ebits(x - u, y), ebits(x + u, y)), umax(ebits(x, y - u), ebits(x, y + u)));
  } else if (k > 0) {
    const int v = 1 << (k - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cx = x + ((q & 1) ? v : -v), cy = y + ((q & 2) ? v : -v);
      if (d.in_domain(cx, cy)) m = umax(m, ebits(cx, cy));
    }
  }
  return m;
}

struct GlobalHeight {
  const float* height;
  Dom d;
  __device__ uint32_t operator()(int x, int y) const { return d.in_grid(x, y) ? __float_as_uint(height[d.at(x, y)]) : kNaN; }
};
struct GlobalError {
  const uint32_t* error;
  Dom d;
  __device__ uint32_t operator()(int x, int y) const { return d.in_grid(x, y) ? error[d.at(x, y)] : kInf; }
};

// ---- one half-level from memory: lattice node i of the grid's part of the lattice of side 2^k
// Only the nodes of the half-level are enumerated -- every lane of a wave has a node: the kernels are bound by the instructions
// they issue, not by their bytes.  A-nodes: every lattice row has `slots` = ceil(nx / 2) of them at most, the odd ix of an even
// row and the even ix of an odd row.  D-nodes: the odd ix of the odd rows, `slots` = floor(nx / 2) a row.
__host__ __device__ inline uint32_t phase_slots(uint32_t nx, int phase) { return phase == 0 ? (nx + 1u) >> 1 : nx >> 1; }
__host__ __device__ inline uint32_t phase_nodes(uint32_t nx, uint32_t ny, int phase) {
  return phase_slots(nx, phase) * (phase == 0 ? ny : ny >> 1);
}
__device__ __forceinline__ void level_node(const float* height, uint32_t* error, const Dom& d, int k, int phase, uint32_t nx, uint32_t i) {
  const uint32_t slots = phase_slots(nx, phase);
  const uint32_t r = i / slots, j = i - r * slots;
  const uint32_t iy = phase == 0 ? r : 2u * r + 1u;
  const uint32_t ix = phase == 0 ? 2u * j + (1u - (iy & 1u)) : 2u * j + 1u;
  if (ix >= nx) return;  // the last slot of an even row of A-nodes when nx is odd
  const int gx = (int)(ix << k), gy = (int)(iy << k);  // inside the grid: nx and ny count the lattice nodes below w and h
  const Split s = split_of(gx, gy, k);
  const uint32_t e = node_e(d, gx, gy, k, s, GlobalHeight{height, d});
  error[d.at(gx, gy)] = umax(e, children_max(d, gx, gy, k, s.dnode, GlobalError{error, d}));
}
__host__ __device__ inline uint32_t lattice_nx(const Dom& d, int k) { return ((d.w - 1) >> k) + 1; }
__host__ __device__ inline uint32_t lattice_ny(const Dom& d, int k) { return ((d.h - 1) >> k) + 1; }

__global__ __launch_bounds__(256) void k_level(const float* height, uint32_t* error, Dom d, int k, int phase) {
  const uint32_t nx = lattice_nx(d, k), n = phase_nodes(nx, lattice_ny(d, k), phase);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) level_node(height, error, d, k, phase, nx, i);
}

__global__ __launch_bounds__(1024) void k_upper_tail(const float* height, uint32_t* error, Dom d, int kBegin) {
  for (int k = kBegin; k < d.L; ++k) {
    const uint32_t nx = lattice_nx(d, k), ny = lattice_ny(d, k);
    for (int phase = 0; phase < 2; ++phase) {
      const uint32_t n = phase_nodes(nx, ny, phase);
      for (uint32_t i = threadIdx.x; i < n; i += 1024u) level_node(height, error, d, k, phase, nx, i);
      __syncthreads();  // the block's stores to `error` are visible to the block
    }
  }
  if (threadIdx.x < 4) {  // the domain's corners are no split nodes
    const int cx = (threadIdx.x & 1) ? (int)d.S : 0, cy = (threadIdx.x & 2) ? (int)d.S : 0;
    if (d.in_grid(cx, cy)) error[d.at(cx, cy)] = kInf;
  }
}

// the levels kBegin .. L - 1 of the error map of a non-empty height map, the levels below being in `error` already; the library
// calls it from level 0 (tools/simplify_lab.hip also behind a kernel of its own for the finest levels)
inline hipError_t errors_launch(const float* height, Dom d, uint32_t* error, hipStream_t st, int kBegin = 0) {
  int k = kBegin;
  for (; k < d.L; ++k) {
    const uint32_t nx = lattice_nx(d, k), ny = lattice_ny(d, k);
    if (nx * ny <= kTailNodes) break;
    for (int phase = 0; phase < 2; ++phase) {
      const uint32_t n = phase_nodes(nx, ny, phase);  // 0 for the D-nodes of a lattice one node wide
      if (n) hipLaunchKernelGGL(k_level, dim3((n + 255u) / 256u), dim3(256), 0, st, height, error, d, k, phase);
    }
  }
  hipLaunchKernelGGL(k_upper_tail, dim3(1), dim3(1024), 0, st, height, error, d, k);
  return hipGetLastError();
}

// ---- the triangle list
struct Cand {
  int ax, ay, bx, by, cx, cy, mx, my;
  bool leaf, root;  // root: the split node of level 0
};
__device__ __forceinline__ bool decode(const Dom& d, uint32_t id, Cand& c) {
  const uint32_t pitch = 2u * d.w;
  const uint32_t Y = id / pitch, r = id - Y * pitch;
  const int xi = (int)(r >> 1), s = (int)(r & 1u), yj = (int)(Y >> 1);
  c.leaf = (Y & 1u) != 0u;
  c.root = false;
  c.mx = xi; c.my = yj;
  if (c.leaf) {
    if ((uint32_t)xi + 1u >= d.w) return false;
    if (((xi + yj) & 1) == 0) {
      c.ax = xi; c.ay = yj; c.bx = xi + 1; c.by = yj + 1;
      c.cx = s ? xi : xi + 1; c.cy = s ? yj + 1 : yj;
    } else {
      c.ax = xi + 1; c.ay = yj; c.bx = xi; c.by = yj + 1;
      c.cx = s ? xi + 1 : xi; c.cy = s ? yj + 1 : yj;
    }
    return true;
  }
  const int k = node_k((uint32_t)xi, (uint32_t)yj);
  if (k >= d.L) return false;
  const Split sp = split_of(xi, yj, k);
  c.ax = sp.ax; c.ay = sp.ay; c.bx = sp.bx; c.by = sp.by;
  c.cx = sp.cx[s]; c.cy = sp.cy[s];
  c.root = sp.dnode && k == d.L - 1;
  return d.in_domain(c.cx, c.cy);
}

struct SimpKeep {
  const float* height;
  const float* error;
  Dom d;
  float tol;
  __device__ bool present(int x, int y) const { return __float_as_uint(height[d.at(x, y)]) != kNaN; }
  __device__ uint32_t operator()(uint32_t id) const {
    Cand c;
    if (!decode(d, id, c)) return 0u;
    if (c.leaf) {
      if (!present(c.ax, c.ay) || !present(c.bx, c.by) || !present(c.cx, c.cy)) return 0u;
      return (d.L == 0 || !(error[d.at(c.cx, c.cy)] <= tol)) ? 1u : 0u;
    }
    if (!(error[d.at(c.mx, c.my)] <= tol)) return 0u;
    // E(m) <= tol makes a, b and c present in an error map of this height map; any other map is still read inside its bounds
    if (!d.in_grid(c.ax, c.ay) || !d.in_grid(c.bx, c.by) || !d.in_grid(c.cx, c.cy)) return 0u;
    return (c.root || !(error[d.at(c.cx, c.cy)] <= tol)) ? 1u : 0u;
  }
};
struct SimpEmit {
  Dom d;
  uint32_t* vertexIndex;
  uint32_t* out;
  uint32_t capacity;
  __device__ void operator()(uint32_t id, int, uint32_t dst) const {
    Cand c;
    decode(d, id, c);
    const uint32_t na = (uint32_t)d.at(c.ax, c.ay), nb = (uint32_t)d.at(c.bx, c.by), nc = (uint32_t)d.at(c.cx, c.cy);
    vertexIndex[na] = kMark;  // kept whether or not the record fits
    vertexIndex[nb] = kMark;
    vertexIndex[nc] = kMark;
    if (dst >= capacity) return;
    const int cross = (c.ax - c.cx) * (c.by - c.cy) - (c.ay - c.cy) * (c.bx - c.cx);
    out[(size_t)dst * 3] = nc;
    out[(size_t)dst * 3 + 1] = cross < 0 ? na : nb;
    out[(size_t)dst * 3 + 2] = cross < 0 ? nb : na;
  }
};

struct KeptKeep {
  const uint32_t* vertexIndex;
  __device__ uint32_t operator()(uint32_t node) const { return vertexIndex[node] == kMark ? 1u : 0u; }
};
struct KeptRank {  // node `node` is read (KeptKeep) and then written by one thread alone
  uint32_t* vertexIndex;
  const uint32_t* nodeIndex;
  uint32_t* kept;
  uint32_t keptCapacity;
  __device__ void operator()(uint32_t node, int, uint32_t dst) const {
    vertexIndex[node] = dst;
    if (dst < keptCapacity) kept[dst] = nodeIndex ? nodeIndex[node] : node;
  }
};

__global__ __launch_bounds__(256) void k_remap(uint32_t* __restrict__ out, uint32_t capacity, const uint32_t* __restrict__ total,
                                               const uint32_t* __restrict__ vertexIndex) {
  const uint32_t n = *total < capacity ? *total : capacity;
  const size_t words = (size_t)n * 3;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < words; i += (size_t)gridDim.x * 256u) out[i] = vertexIndex[out[i]];
}

// ---- host side
inline bool size_invalid(uint32_t w, uint32_t h) { return (unsigned long long)w * h >= (1ull << 31); }
inline bool size_unsupported(uint32_t w, uint32_t h) { return (unsigned long long)w * h > (1ull << 29); }
inline uint32_t candidates(uint32_t w, uint32_t h) { return 2u * w * (2u * h - 1u); }
inline size_t compaction_bytes(uint32_t n) { return align256(svc::workspace_words<1, kPerThread>(n) * 4); }

}  // namespace svsimp

#ifndef SSRLCV_SIMPLIFY_LAB
extern "C" {

int ssrlcv_hip_dsm_simplify_errors(const float* height, uint32_t w, uint32_t h, float* error, ssrlcv_stream_t stream) {
  using namespace svsimp;
  if (size_invalid(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (size_unsupported(w, h)) return SSRLCV_ERR_UNSUPPORTED;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!height || !error) return SSRLCV_ERR_INVALID_ARG;
  SSRLCV_HIP_TRY(errors_launch(height, make_dom(w, h), (uint32_t*)error, (hipStream_t)stream));
  return SSRLCV_OK;
}

size_t ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(uint32_t w, uint32_t h) {
  using namespace svsimp;
  if (size_invalid(w, h) || size_unsupported(w, h) || w == 0 || h == 0) return 0;
  return compaction_bytes(candidates(w, h)) + compaction_bytes(w * h);
}

int ssrlcv_hip_dsm_simplify_mesh(const float* height, const float* error, uint32_t w, uint32_t h, float tolerance, const uint32_t* nodeIndex,
                                 uint32_t* vertexIndex, uint32_t* out, uint32_t capacity, uint32_t* triCount_dev, uint32_t* kept,
                                 uint32_t keptCapacity, uint32_t* vertexCount_dev, void* workspace, size_t workspaceBytes,
                                 ssrlcv_stream_t stream) {
  using namespace svsimp;
  if (!(fabsf(tolerance) <= 3.4028234663852886e38f)) return SSRLCV_ERR_INVALID_ARG;
  if (size_invalid(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (size_unsupported(w, h)) return SSRLCV_ERR_UNSUPPORTED;
  if (!triCount_dev || !vertexCount_dev) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (w == 0 || h == 0) {  // an empty map: no triangle and no vertex, and nothing else is looked at
    SSRLCV_HIP_TRY(hipMemsetAsync(triCount_dev, 0, 4, st));
    SSRLCV_HIP_TRY(hipMemsetAsync(vertexCount_dev, 0, 4, st));
    return SSRLCV_OK;
  }
  if (!height || !error || !vertexIndex || !workspace || (!out && capacity != 0) || (!kept && keptCapacity != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(w, h)) return SSRLCV_ERR_WORKSPACE;
  const Dom d = make_dom(w, h);
  const uint32_t nodes = w * h, cand = candidates(w, h);
  uint32_t* wsTri = (uint32_t*)workspace;
  uint32_t* wsKept = (uint32_t*)((char*)workspace + compaction_bytes(cand));
  SSRLCV_HIP_TRY(hipMemsetAsync(vertexIndex, 0xFF, (size_t)nodes * 4, st));
  SimpKeep keep{height, error, d, tolerance};
  SimpEmit emit{d, vertexIndex, out, capacity};
  uint32_t* triTotals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(cand, keep, emit, wsTri, &triTotals, st)));
  KeptKeep keptKeep{vertexIndex};
  KeptRank rank{vertexIndex, nodeIndex, kept, keptCapacity};
  uint32_t* keptTotals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(nodes, keptKeep, rank, wsKept, &keptTotals, st)));
  const unsigned long long most = 2ull * (w - 1) * (h - 1);  // the full-resolution mesh
  const unsigned long long words = 3ull * (capacity < most ? capacity : most);
  if (words) {
    const unsigned long long blocks = (words + 255ull) / 256ull;
    hipLaunchKernelGGL(k_remap, dim3((uint32_t)(blocks < 65536ull ? blocks : 65536ull)), dim3(256), 0, st, out, capacity, triTotals + 1, vertexIndex);
    SSRLCV_LAUNCH_CHECK();
  }
  SSRLCV_HIP_TRY(hipMemcpyAsync(triCount_dev, triTotals + 1, 4, hipMemcpyDeviceToDevice, st));
  SSRLCV_HIP_TRY(hipMemcpyAsync(vertexCount_dev, keptTotals + 1, 4, hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

}  // extern "C"
#endif
