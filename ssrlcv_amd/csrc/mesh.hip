// ssrlcv_amd/csrc/mesh.hip -- triangle mesh and normals from a disparity map for gfx950.  The contract is include/ssrlcv_hip.h
// "disparity mesh"; tests/mesh_ref.py restates it.  The sampling grid of ssrlcv_hip_stereo_matches gives the connectivity, a
// disparity jump a depth edge, the face winding the orientation: everything is a selection or a fixed-order float32 expression.
//
//   k_mesh_cells     a thread per node (i, j): UINT32_MAX into vertexIndex at an invalid node, and the byte of cell (i, j) where
//                    the node is the cell's corner a: four disparities, six differences, one comparison for the diagonal
//   MeshKeep / MeshRank + compact.h   the rank of every valid node among the valid nodes in raster order: the ordered compaction
//                    of ssrlcv_hip_stereo_matches with the same mask, which emits the rank itself instead of a record
//   TriKeep / TriEmit + compact.h     the triangle list: slot 2 cell + t carries triangle t of the cell iff bit t of its byte is
//                    set; the emit looks its three corners up in vertexIndex
//   k_mesh_normals   a thread per node: the up to eight triangles around it (four cells, T0 then T1), their cross products
//                    summed in that order, one sqrt and three divisions
//   k_select_map     old vertex -> new vertex: the inverse of keptIndex in the workspace (UINT32_MAX first)
//   k_select_cells   clears the bits of the triangles that lose a corner (reads the OLD vertexIndex), then
//   k_select_nodes   renumbers vertexIndex in place
// Every output word has exactly one writer, so nothing is added up in memory, and no block waits for another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "compact.h"
#include "device_math.h"
#include "mesh_corners.h"

namespace {

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kPerThread = 16;  // compact.h: a wave owns a run of 1024 elements, a block 4096

// samples 0, step, 2 step, ... below n (stereo_grid of csrc/stereo.hip)
uint32_t mesh_grid(uint32_t n, uint32_t step) { return n ? (n - 1) / step + 1 : 0; }

struct Grid {
  uint32_t gw, gh;
  __host__ __device__ uint32_t nodes() const { return gw * gh; }
  __host__ __device__ uint32_t cells() const { return gw >= 2 && gh >= 2 ? (gw - 1) * (gh - 1) : 0u; }
};

__device__ __forceinline__ bool joined(float p, float q, float maxJump) { return fabsf(p - q) <= maxJump; }  // false for a NaN

__global__ __launch_bounds__(256) void k_mesh_cells(const float* __restrict__ disparity, uint32_t w, uint32_t step, Grid g, float maxJump,
                                                    uint32_t* __restrict__ vertexIndex, uint8_t* __restrict__ cells) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  if (node >= g.nodes()) return;
  const uint32_t j = node / g.gw, i = node - j * g.gw;
  const size_t at = (size_t)j * step * w + (size_t)i * step;  // pixel (i step, j step): below w h < 2^31
  const float da = disparity[at];
  const bool va = __float_as_uint(da) != kNaN;
  if (!va) vertexIndex[node] = kNone;  // the valid nodes are MeshRank's
  if (i + 1 >= g.gw || j + 1 >= g.gh) return;
  const size_t down = (size_t)step * w;
  const float db = disparity[at + step], dc = disparity[at + down], dd = disparity[at + down + step];
  const bool vb = __float_as_uint(db) != kNaN, vc = __float_as_uint(dc) != kNaN, vd = __float_as_uint(dd) != kNaN;
  uint32_t byte = 0;
  if ((int)va + (int)vb + (int)vc + (int)vd >= 3) {
    // four valid corners: b-c iff it is the smaller jump (ties and NaN comparisons: a-d); three: the diagonal between valid corners
    const bool bc = va && vd ? (vb && vc && fabsf(db - dc) < fabsf(da - dd)) : true;
    const bool ab = va && vb && joined(da, db, maxJump), ac = va && vc && joined(da, dc, maxJump);
    const bool bd = vb && vd && joined(db, dd, maxJump), cd = vc && vd && joined(dc, dd, maxJump);
    bool t0, t1;
    if (bc) {
      const bool diag = vb && vc && joined(db, dc, maxJump);
      t0 = diag && ac && ab;  // (a, c, b)
      t1 = diag && cd && bd;  // (b, c, d)
    } else {
      const bool diag = va && vd && joined(da, dd, maxJump);
      t0 = diag && ac && cd;  // (a, c, d)
      t1 = diag && bd && ab;  // (a, d, b)
    }
    byte = (t0 ? 1u : 0u) | (t1 ? 2u : 0u);
    if (byte && bc) byte |= 4u;
  }
  cells[(size_t)j * (g.gw - 1) + i] = (uint8_t)byte;
}

struct MeshKeep {
  const float* disparity;
  uint32_t w, step, gw;
  __device__ uint32_t operator()(uint32_t node) const {
    const uint32_t j = node / gw, i = node - j * gw;
    return __float_as_uint(disparity[(size_t)j * step * w + (size_t)i * step]) != kNaN ? 1u : 0u;
  }
};
struct MeshRank {
  uint32_t* vertexIndex;
  __device__ void operator()(uint32_t node, int, uint32_t dst) const { vertexIndex[node] = dst; }
};

// ---- the triangle list
struct TriKeep {
  const uint8_t* cells;
  __device__ uint32_t operator()(uint32_t slot) const { return ((uint32_t)cells[slot >> 1] >> (slot & 1u)) & 1u; }
};
struct TriEmit {
  const uint32_t* vertexIndex;
  const uint8_t* cells;
  Grid g;
  uint32_t* out;
  uint32_t capacity;
  __device__ void operator()(uint32_t slot, int, uint32_t dst) const {
    if (dst >= capacity) return;
    const uint32_t cell = slot >> 1, cj = cell / (g.gw - 1), ci = cell - cj * (g.gw - 1);
    uint32_t node[3];
    triangle_nodes(g.gw, ci, cj, (cells[cell] & 4u) != 0u, (int)(slot & 1u), node);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)dst * 3 + k] = vertexIndex[node[k]];
  }
};

// ---- normals
__global__ __launch_bounds__(256) void k_mesh_normals(const ssrlcv_float3* __restrict__ points, uint32_t n, const uint32_t* __restrict__ vertexIndex,
                                                      const uint8_t* __restrict__ cells, Grid g, float* __restrict__ normals) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  if (node >= g.nodes()) return;
  const uint32_t me = vertexIndex[node];
  if (me >= n) return;  // no vertex (UINT32_MAX), or a stale index: nothing is written
  const uint32_t j = node / g.gw, i = node - j * g.gw;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // the cells (i - 1, j - 1), (i, j - 1), (i - 1, j), (i, j)
    const uint32_t ci = i - ((q & 1) ? 0u : 1u), cj = j - ((q & 2) ? 0u : 1u);  // wraps for a missing cell: above the bounds below
    if (ci >= g.gw - 1 || cj >= g.gh - 1) continue;  // gw, gh >= 2 wherever a cell byte is read: a 1-wide grid has no cell
    const uint32_t byte = cells[(size_t)cj * (g.gw - 1) + ci];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (!((byte >> t) & 1u)) continue;
      uint32_t tri[3];
      triangle_nodes(g.gw, ci, cj, (byte & 4u) != 0u, t, tri);
      if (tri[0] != node && tri[1] != node && tri[2] != node) continue;
      const uint32_t ip = vertexIndex[tri[0]], iq = vertexIndex[tri[1]], ir = vertexIndex[tri[2]];
      if (ip >= n || iq >= n || ir >= n) continue;
      const ssrlcv_float3 P = points[ip], Q = points[iq], R = points[ir];
      const float ux = Q.x - P.x, uy = Q.y - P.y, uz = Q.z - P.z;
      const float vx = R.x - P.x, vy = R.y - P.y, vz = R.z - P.z;
      sx = sx + ((uy * vz) - (uz * vy));
      sy = sy + ((uz * vx) - (ux * vz));
      sz = sz + ((ux * vy) - (uy * vx));
    }
  }
  const float len = sqrtf(((sx * sx) + (sy * sy)) + (sz * sz));  // correctly rounded (HIP's default), as the division is
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (len > 0.0f && len <= 3.4028234663852886e38f) {
    nx = __fdiv_rn(sx, len);
    ny = __fdiv_rn(sy, len);
    nz = __fdiv_rn(sz, len);
  }
  normals[(size_t)me * 3] = nx;
  normals[(size_t)me * 3 + 1] = ny;
  normals[(size_t)me * 3 + 2] = nz;
}

// ---- select
__global__ __launch_bounds__(256) void k_select_map(const uint32_t* __restrict__ keptIndex, uint32_t m, uint32_t nVertices, uint32_t* __restrict__ map) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= m) return;
  const uint32_t old = keptIndex[k];
  if (old < nVertices) map[old] = k;  // keptIndex ascends strictly: one writer an entry
}

__device__ __forceinline__ bool select_keeps(const uint32_t* __restrict__ map, uint32_t nVertices, uint32_t old) {
  return old < nVertices && map[old] != kNone;
}

__global__ __launch_bounds__(256) void k_select_cells(const uint32_t* __restrict__ vertexIndex, const uint32_t* __restrict__ map, uint32_t nVertices,
                                                      Grid g, uint8_t* __restrict__ cells) {
  const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
  if (cell >= g.cells()) return;
  const uint32_t byte = cells[cell];
  if ((byte & 3u) == 0u) {
    if (byte) cells[cell] = 0;  // no triangle: the byte is 0 by contract, whatever a caller left in bit 2
    return;
  }
  const uint32_t cj = cell / (g.gw - 1), ci = cell - cj * (g.gw - 1);
  uint32_t keep = byte & 3u;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (!((byte >> t) & 1u)) continue;
    uint32_t tri[3];
    triangle_nodes(g.gw, ci, cj, (byte & 4u) != 0u, t, tri);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (!select_keeps(map, nVertices, vertexIndex[tri[k]])) keep &= ~(1u << t);
  }
  const uint32_t now = keep ? (keep | (byte & 4u)) : 0u;
  if (now != byte) cells[cell] = (uint8_t)now;
}

__global__ __launch_bounds__(256) void k_select_nodes(uint32_t* __restrict__ vertexIndex, const uint32_t* __restrict__ map, uint32_t nVertices, uint32_t nodes) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  if (node >= nodes) return;
  const uint32_t old = vertexIndex[node];
  const uint32_t now = old < nVertices ? map[old] : kNone;
  if (now != old) vertexIndex[node] = now;
}

// ---- host side
bool grid_fits(uint32_t gw, uint32_t gh) { return (unsigned long long)gw * gh < (1ull << 31); }
size_t compaction_bytes(uint32_t n) { return align256(svc::workspace_words<1, kPerThread>(n) * 4); }
dim3 blocks_for(uint32_t n) { return dim3((n + 255u) / 256u); }

int mesh_params_status(uint32_t w, uint32_t h, const ssrlcv_mesh_params* p) {
  if (!p || p->step == 0 || !(p->maxJump >= 0.0f)) return SSRLCV_ERR_INVALID_ARG;
  if ((unsigned long long)w * h >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  return SSRLCV_OK;
}

}  // namespace

extern "C" {

size_t ssrlcv_hip_disparity_mesh_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_mesh_params* params) {
  if (mesh_params_status(w, h, params)) return 0;
  return compaction_bytes(mesh_grid(w, params->step) * mesh_grid(h, params->step));
}

int ssrlcv_hip_disparity_mesh(const float* disparity, uint32_t w, uint32_t h, const ssrlcv_mesh_params* params, uint32_t* vertexIndex, uint8_t* cells,
                              uint32_t* vertexCount_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (const int rc = mesh_params_status(w, h, params)) return rc;
  const Grid g{mesh_grid(w, params->step), mesh_grid(h, params->step)};
  if (!vertexCount_dev) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (g.nodes() == 0) {  // an empty map: no vertex, and nothing else is looked at
    SSRLCV_HIP_TRY(hipMemsetAsync(vertexCount_dev, 0, 4, st));
    return SSRLCV_OK;
  }
  if (!disparity || !vertexIndex || !workspace || (!cells && g.cells() != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < compaction_bytes(g.nodes())) return SSRLCV_ERR_WORKSPACE;
  hipLaunchKernelGGL(k_mesh_cells, blocks_for(g.nodes()), dim3(256), 0, st, disparity, w, params->step, g, params->maxJump, vertexIndex, cells);
  SSRLCV_LAUNCH_CHECK();
  MeshKeep keep{disparity, w, params->step, g.gw};
  MeshRank rank{vertexIndex};
  uint32_t* totals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(g.nodes(), keep, rank, (uint32_t*)workspace, &totals, st)));
  SSRLCV_HIP_TRY(hipMemcpyAsync(vertexCount_dev, totals + 1, 4, hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

size_t ssrlcv_hip_mesh_triangles_workspace_bytes(uint32_t gw, uint32_t gh) {
  if (!grid_fits(gw, gh)) return 0;
  return compaction_bytes(2u * Grid{gw, gh}.cells());
}

int ssrlcv_hip_mesh_triangles(const uint32_t* vertexIndex, const uint8_t* cells, uint32_t gw, uint32_t gh, uint32_t* out, uint32_t capacity,
                              uint32_t* count_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!grid_fits(gw, gh)) return SSRLCV_ERR_INVALID_ARG;
  const Grid g{gw, gh};
  if (!count_dev || (!out && capacity != 0)) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (g.cells() == 0) {  // no cell: no triangle
    SSRLCV_HIP_TRY(hipMemsetAsync(count_dev, 0, 4, st));
    return SSRLCV_OK;
  }
  if (!vertexIndex || !cells || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < compaction_bytes(2u * g.cells())) return SSRLCV_ERR_WORKSPACE;
  TriKeep keep{cells};
  TriEmit emit{vertexIndex, cells, g, out, capacity};
  uint32_t* totals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kPerThread>(2u * g.cells(), keep, emit, (uint32_t*)workspace, &totals, st)));
  SSRLCV_HIP_TRY(hipMemcpyAsync(count_dev, totals + 1, 4, hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

int ssrlcv_hip_mesh_normals(const ssrlcv_float3* points, uint32_t n, const uint32_t* vertexIndex, const uint8_t* cells, uint32_t gw, uint32_t gh,
                            float* normals, ssrlcv_stream_t stream) {
  if (!grid_fits(gw, gh)) return SSRLCV_ERR_INVALID_ARG;
  const Grid g{gw, gh};
  if (n == 0 || g.nodes() == 0) return SSRLCV_OK;  // no vertex to write
  if (!points || !vertexIndex || !normals || (!cells && g.cells() != 0)) return SSRLCV_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_mesh_normals, blocks_for(g.nodes()), dim3(256), 0, (hipStream_t)stream, points, n, vertexIndex, cells, g, normals);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_mesh_select_workspace_bytes(uint32_t nVertices) { return align256((size_t)nVertices * 4); }

int ssrlcv_hip_mesh_select(uint32_t* vertexIndex, uint8_t* cells, uint32_t gw, uint32_t gh, uint32_t nVertices, const uint32_t* keptIndex, uint32_t m,
                           void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!grid_fits(gw, gh)) return SSRLCV_ERR_INVALID_ARG;
  const Grid g{gw, gh};
  if (g.nodes() == 0) return SSRLCV_OK;
  if (!vertexIndex || (!cells && g.cells() != 0) || (!keptIndex && m != 0) || (!workspace && nVertices != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_mesh_select_workspace_bytes(nVertices)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* map = (uint32_t*)workspace;
  if (nVertices) SSRLCV_HIP_TRY(hipMemsetAsync(map, 0xFF, (size_t)nVertices * 4, st));
  if (m && nVertices) {
    hipLaunchKernelGGL(k_select_map, blocks_for(m), dim3(256), 0, st, keptIndex, m, nVertices, map);
    SSRLCV_LAUNCH_CHECK();
  }
  if (g.cells()) {
    hipLaunchKernelGGL(k_select_cells, blocks_for(g.cells()), dim3(256), 0, st, vertexIndex, map, nVertices, g, cells);
    SSRLCV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_select_nodes, blocks_for(g.nodes()), dim3(256), 0, st, vertexIndex, map, nVertices, g.nodes());
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
