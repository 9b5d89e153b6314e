// ssrlcv_amd/csrc/render.hip -- the grid mesh drawn into a pinhole view for gfx950: a z-buffered rasterisation that gives the
// depth map of the model in the view, the triangle under every pixel and the greys of the vertices carried into the image, and
// the residual of such a picture against the view's own pixels.  The contract is include/ssrlcv_hip.h "mesh render";
// tests/render_ref.py restates it.
//
//   k_render_project  a thread per vertex: the projection of "ortho-image" in float32, the usability tests, the position in
//                     1/256 pixel as int32, the inverse depth and the grey, 16 bytes a vertex in the workspace
//   k_render_scatter  a thread per cell, T0 then T1 from the cell's byte: int32 edge functions over the pixel centres of the
//                     bounding box, and per covered pixel one 64-bit integer atomicMax of (bits(v) << 32) | (0xFFFFFFFF - id)
//                     on the pixel's accumulator -- k_dsm_scatter's winner: the greatest inverse depth, among equal ones the
//                     smallest id, whatever the arrival order.  0 = nothing drawn: v is positive.  At most 8192 blocks walk the
//                     cells; the three counts are summed a block and added by three atomicAdds a block, each counter in a
//                     64-byte line of its own.
//   k_render_resolve  a thread per pixel, no atomics: depth from the accumulator's upper word, and for the shade the winner's
//                     weights again from its three vertices; its first three threads hand the counts out
//   k_image_residual  a thread per pixel: one subtraction where the depth is valid
// Integer max and integer add commute, so the maps are bit-equal run to run; nothing is added up in floating point across
// threads.  The loop of a thread over a triangle is bounded by (maxExtent + 1)^2 pixel centres.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "mesh_corners.h"

namespace {

using dsm::finite_bits;
using dsm::finite_host;
using dsm::too_many_cells;

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr float kFltMax = 3.4028234663852886e38f;
constexpr uint32_t kMaxExtent = 64;

struct Projection {
  float M[9];
  float pos[3];
};

// a projected vertex: iw holds the bits of 1 / W, 0 for a vertex that is not usable (a usable one's are never 0)
struct Vertex {
  int32_t fx, fy;
  uint32_t iw;
  uint32_t grey;
};

__global__ __launch_bounds__(256) void k_render_project(const ssrlcv_float3* __restrict__ points, uint32_t n, const uint8_t* __restrict__ grey,
                                                        Projection v, Vertex* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const ssrlcv_float3 P = points[t];
  Vertex o{0, 0, 0u, grey ? (uint32_t)grey[t] : 0u};
  if (finite_bits(__float_as_uint(P.x)) && finite_bits(__float_as_uint(P.y)) && finite_bits(__float_as_uint(P.z))) {
    const float dx = P.x - v.pos[0], dy = P.y - v.pos[1], dz = P.z - v.pos[2];
    const float X = (v.M[0] * dx + v.M[1] * dy) + v.M[2] * dz;
    const float Y = (v.M[3] * dx + v.M[4] * dy) + v.M[5] * dz;
    const float W = (v.M[6] * dx + v.M[7] * dy) + v.M[8] * dz;
    const float sx = __fdiv_rn(X, W), sy = __fdiv_rn(Y, W);
    const float iw = __fdiv_rn(1.0f, W);
    // a NaN fails every comparison; the bound on |sx| is the finite test as well
    if (W > 0.0f && W <= 0x1p60f && fabsf(sx) <= 1048576.0f && fabsf(sy) <= 1048576.0f && iw <= kFltMax) {
      o.fx = (int32_t)rintf(sx * 256.0f);
      o.fy = (int32_t)rintf(sy * 256.0f);
      o.iw = __float_as_uint(iw);
    }
  }
  out[t] = o;
}

// the edge function of (a, b) at c: below 2^29 in magnitude once the three points lie in a box of 2^14 a side
__device__ __forceinline__ int32_t edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t cx, int32_t cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

struct Triangle {
  Vertex p, q, r;
  int32_t A;  // the signed area's edge value; the edge values are negated where it is negative
};

// the three edge values of a pixel centre, Ep opposite p, and |A|; false if the centre is not covered
__device__ __forceinline__ bool edges_at(const Triangle& t, int32_t cx, int32_t cy, int32_t& ep, int32_t& eq, int32_t& er, int32_t& a) {
  ep = edge(t.q.fx, t.q.fy, t.r.fx, t.r.fy, cx, cy);
  eq = edge(t.r.fx, t.r.fy, t.p.fx, t.p.fy, cx, cy);
  er = edge(t.p.fx, t.p.fy, t.q.fx, t.q.fy, cx, cy);
  a = t.A;
  if (a < 0) {
    ep = -ep;
    eq = -eq;
    er = -er;
    a = -a;
  }
  return ep >= 0 && eq >= 0 && er >= 0;
}

// lp, lq, lr of "per covered pixel"
__device__ __forceinline__ void weights(int32_t ep, int32_t eq, int32_t er, int32_t a, float& lp, float& lq, float& lr) {
  const float fa = (float)a;
  lp = __fdiv_rn((float)ep, fa);
  lq = __fdiv_rn((float)eq, fa);
  lr = __fdiv_rn((float)er, fa);
}

// the three projected vertices of triangle t of a cell; false for an index that is not below n or a vertex that is not usable
__device__ __forceinline__ bool load_triangle(const Vertex* __restrict__ verts, uint32_t n, const uint32_t* __restrict__ vertexIndex, uint32_t gw,
                                              uint32_t ci, uint32_t cj, bool bc, int t, Triangle& tri) {
  uint32_t node[3];
  triangle_nodes(gw, ci, cj, bc, t, node);
  const uint32_t ip = vertexIndex[node[0]], iq = vertexIndex[node[1]], ir = vertexIndex[node[2]];
  if (ip >= n || iq >= n || ir >= n) return false;  // no vertex (UINT32_MAX), or a stale index: nothing is read
  tri.p = verts[ip];
  tri.q = verts[iq];
  tri.r = verts[ir];
  return tri.p.iw != 0u && tri.q.iw != 0u && tri.r.iw != 0u;
}

__device__ __forceinline__ int32_t min3(int32_t a, int32_t b, int32_t c) { return min(a, min(b, c)); }
__device__ __forceinline__ int32_t max3(int32_t a, int32_t b, int32_t c) { return max(a, max(b, c)); }

constexpr uint32_t kScatterBlocks = 8192;  // a few rounds of the blocks the chip holds at once, so that the last round is a small part
constexpr uint32_t kCounterStride = 16;    // words: each of the three counters has a 64-byte line of its own

__global__ __launch_bounds__(256) void k_render_scatter(const Vertex* __restrict__ verts, uint32_t n, const uint32_t* __restrict__ vertexIndex,
                                                        const uint8_t* __restrict__ cells, uint32_t gw, uint32_t numCells, uint32_t w, uint32_t h,
                                                        int32_t maxSpan, unsigned long long* __restrict__ acc, uint32_t* __restrict__ counts) {
  uint32_t tally[3] = {0u, 0u, 0u};  // drawn, too large, unusable
  // The blocks walk the cells 256 at a time, so the counts cost three atomics a block.  One atomic a wave on one word -- 262 144
  // of them for a 4096^2 map -- took 3.0 of the call's 3.3 ms, whatever the view: atomics on one address are served one after
  // the other (profiles/render_bench.txt).
  for (uint32_t base = blockIdx.x * 256u; base < numCells; base += gridDim.x * 256u) {  // numCells < 2^31: no wrap
    const uint32_t cell = base + threadIdx.x;
    const uint32_t byte = cell < numCells ? (uint32_t)cells[cell] : 0u;
    if (!(byte & 3u)) continue;
    const uint32_t cj = cell / (gw - 1u), ci = cell - cj * (gw - 1u);
    for (int t = 0; t < 2; ++t) {
      if (!((byte >> t) & 1u)) continue;
      Triangle tri;
      if (!load_triangle(verts, n, vertexIndex, gw, ci, cj, (byte & 4u) != 0u, t, tri)) {
        ++tally[2];
        continue;
      }
      const int32_t minx = min3(tri.p.fx, tri.q.fx, tri.r.fx), maxx = max3(tri.p.fx, tri.q.fx, tri.r.fx);
      const int32_t miny = min3(tri.p.fy, tri.q.fy, tri.r.fy), maxy = max3(tri.p.fy, tri.q.fy, tri.r.fy);
      if (maxx - minx > maxSpan || maxy - miny > maxSpan) {  // |f| <= 2^28: the differences fit
        ++tally[1];
        continue;
      }
      tri.A = edge(tri.p.fx, tri.p.fy, tri.q.fx, tri.q.fy, tri.r.fx, tri.r.fy);
      if (tri.A == 0) {
        ++tally[2];
        continue;
      }
      // the pixel centres 256 x inside the box: floor and ceiling by an arithmetic shift, right for negative coordinates
      const int32_t x0 = max((minx + 255) >> 8, 0), x1 = min(maxx >> 8, (int32_t)w - 1);
      const int32_t y0 = max((miny + 255) >> 8, 0), y1 = min(maxy >> 8, (int32_t)h - 1);
      if (x0 > x1 || y0 > y1) continue;  // no pixel centre of the image in the box: neither drawn nor skipped
      ++tally[0];
      const uint32_t id = 2u * cell + (uint32_t)t;
      const float iwp = __uint_as_float(tri.p.iw), iwq = __uint_as_float(tri.q.iw), iwr = __uint_as_float(tri.r.iw);
      for (int32_t y = y0; y <= y1; ++y) {
        for (int32_t x = x0; x <= x1; ++x) {
          int32_t ep, eq, er, a;
          if (!edges_at(tri, x << 8, y << 8, ep, eq, er, a)) continue;
          float lp, lq, lr;
          weights(ep, eq, er, a, lp, lq, lr);
          const float v = ((lp * iwp) + (lq * iwq)) + (lr * iwr);
          atomicMax(acc + ((size_t)y * w + (size_t)x), ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(kNone - id));
        }
      }
    }
  }
  __shared__ uint32_t part[4][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tally[k] += (uint32_t)__shfl_xor(tally[k], o, 64);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][k] = tally[k];
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    const uint32_t c = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (c) atomicAdd(counts + kCounterStride * threadIdx.x, c);
  }
}

__global__ __launch_bounds__(256) void k_render_resolve(const unsigned long long* __restrict__ acc, uint32_t pixels, uint32_t w,
                                                        const Vertex* __restrict__ verts, uint32_t n, const uint32_t* __restrict__ vertexIndex,
                                                        const uint8_t* __restrict__ cells, uint32_t gw, const uint32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ depth, uint32_t* __restrict__ triangle, uint8_t* __restrict__ shade,
                                                        uint32_t* __restrict__ countsOut) {
  const uint32_t px = blockIdx.x * 256u + threadIdx.x;
  if (px < 3u && countsOut) countsOut[px] = counts[kCounterStride * px];  // block 0 always has its first three threads
  if (px >= pixels) return;
  const unsigned long long a = acc[px];
  uint32_t d = kNaN, id = kNone, s = 0u;
  if (a != 0ull) {
    d = __float_as_uint(__fdiv_rn(1.0f, __uint_as_float((uint32_t)(a >> 32))));
    id = kNone - (uint32_t)a;
    if (shade) {  // the winner was drawn by the scatter: its cell, its indices and its vertices passed every test there
      const uint32_t cell = id >> 1, cj = cell / (gw - 1u), ci = cell - cj * (gw - 1u);
      Triangle tri;
      load_triangle(verts, n, vertexIndex, gw, ci, cj, (cells[cell] & 4u) != 0u, (int)(id & 1u), tri);
      tri.A = edge(tri.p.fx, tri.p.fy, tri.q.fx, tri.q.fy, tri.r.fx, tri.r.fy);
      const uint32_t y = px / w, x = px - y * w;
      int32_t ep, eq, er, area;
      edges_at(tri, (int32_t)x << 8, (int32_t)y << 8, ep, eq, er, area);
      float lp, lq, lr;
      weights(ep, eq, er, area, lp, lq, lr);
      const float g = ((lp * (float)tri.p.grey) + (lq * (float)tri.q.grey)) + (lr * (float)tri.r.grey);
      s = (uint32_t)fminf(fmaxf(floorf(g + 0.5f), 0.0f), 255.0f);
    }
  }
  depth[px] = d;
  if (triangle) triangle[px] = id;
  if (shade) shade[px] = (uint8_t)s;
}

__global__ __launch_bounds__(256) void k_image_residual(const uint8_t* __restrict__ image, const uint8_t* __restrict__ shade,
                                                        const uint32_t* __restrict__ depth, uint32_t pixels, uint32_t* __restrict__ out) {
  const uint32_t px = blockIdx.x * 256u + threadIdx.x;
  if (px >= pixels) return;
  out[px] = depth[px] != kNaN ? __float_as_uint((float)image[px] - (float)shade[px]) : kNaN;
}

// ---- host side
constexpr size_t kCounterBytes = 256;

dim3 blocks_for(uint32_t items) { return dim3((items + 255u) / 256u); }

uint32_t cells_of(uint32_t gw, uint32_t gh) { return gw >= 2 && gh >= 2 ? (gw - 1) * (gh - 1) : 0u; }

size_t acc_bytes(uint32_t w, uint32_t h) { return align256((size_t)w * h * 8); }

}  // namespace

extern "C" {

size_t ssrlcv_hip_mesh_render_workspace_bytes(uint32_t n, uint32_t w, uint32_t h) {
  if (too_many_cells(w, h)) return 0;
  return kCounterBytes + acc_bytes(w, h) + align256((size_t)n * sizeof(Vertex));
}

int ssrlcv_hip_mesh_render(const ssrlcv_float3* points, uint32_t n, const uint8_t* grey, const uint32_t* vertexIndex, const uint8_t* cells, uint32_t gw,
                           uint32_t gh, const ssrlcv_ortho_view* view, const ssrlcv_render_params* params, float* depth, uint32_t* triangle,
                           uint8_t* shade, uint32_t* counts_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!params || params->maxExtent == 0 || params->maxExtent > kMaxExtent || !view) return SSRLCV_ERR_INVALID_ARG;
  for (int k = 0; k < 9; ++k)
    if (!finite_host(view->M[k])) return SSRLCV_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k)
    if (!finite_host(view->pos[k])) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t w = view->w, h = view->h;
  if (too_many_cells(w, h) || too_many_cells(gw, gh)) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (w == 0 || h == 0) {  // an empty view: no output has an entry and no triangle is on the image
    if (counts_dev) SSRLCV_HIP_TRY(hipMemsetAsync(counts_dev, 0, 12, st));
    return SSRLCV_OK;
  }
  const uint32_t numCells = cells_of(gw, gh);
  const bool draws = numCells != 0 && n != 0;
  if (!depth || !workspace || (draws && (!points || !vertexIndex || !cells))) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_mesh_render_workspace_bytes(n, w, h)) return SSRLCV_ERR_WORKSPACE;
  uint32_t* counts = (uint32_t*)workspace;
  unsigned long long* acc = (unsigned long long*)((char*)workspace + kCounterBytes);
  Vertex* verts = (Vertex*)((char*)acc + acc_bytes(w, h));
  const uint32_t pixels = w * h;
  SSRLCV_HIP_TRY(hipMemsetAsync(workspace, 0, kCounterBytes + (size_t)pixels * 8, st));  // the counters and every accumulator
  if (draws) {
    Projection pr;
    for (int k = 0; k < 9; ++k) pr.M[k] = view->M[k];
    for (int k = 0; k < 3; ++k) pr.pos[k] = view->pos[k];
    hipLaunchKernelGGL(k_render_project, blocks_for(n), dim3(256), 0, st, points, n, grey, pr, verts);
    SSRLCV_LAUNCH_CHECK();
    const unsigned blocks = (numCells + 255u) / 256u;
    hipLaunchKernelGGL(k_render_scatter, dim3(blocks < kScatterBlocks ? blocks : kScatterBlocks), dim3(256), 0, st, verts, n, vertexIndex, cells, gw, numCells, w, h,
                       (int32_t)(256u * params->maxExtent), acc, counts);
    SSRLCV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_render_resolve, blocks_for(pixels), dim3(256), 0, st, acc, pixels, w, verts, n, vertexIndex, cells, gw, counts,
                     (uint32_t*)depth, triangle, shade, counts_dev);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

int ssrlcv_hip_image_residual(const uint8_t* image, const uint8_t* shade, const float* depth, uint32_t w, uint32_t h, float* out,
                              ssrlcv_stream_t stream) {
  if (too_many_cells(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (w == 0 || h == 0) return SSRLCV_OK;
  if (!image || !shade || !depth || !out) return SSRLCV_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_image_residual, blocks_for(w * h), dim3(256), 0, (hipStream_t)stream, image, shade, (const uint32_t*)depth, w * h,
                     (uint32_t*)out);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
