// ssrlcv_amd/csrc/register.hip -- surface registration for gfx950: the normal equations of the point-to-plane alignment of a cloud
// to a reference height map over seven unknowns (translation, rotation, scale), a pose applied to a cloud, and the host steps
// between them.  The contract is include/ssrlcv_hip.h "surface registration"; tests/register_ref.py restates it.
//
//   k_register_terms   a block walks tiles of 4096 points.  Per point, in fixed-order float32: the pose, the MESH lookup of surface
//                      accuracy (mesh_lookup.h: the difference d and the slopes of the triangle under the point), the gradient of d
//                      in the world, the Jacobian row J[7] and the residual e.  The 36 sums -- 28 of J J^T, 7 of J e, e e -- are
//                      float64 in the shape of surface accuracy's `sum`: a lane adds its entries l + 256 r in order, every product of
//                      two floats exact in float64 (so the fused multiply-add is the same sum), the 256 lane sums of a tile fold by
//                      halves, twelve sums a round through 24 KB of LDS and then inside wave 0; one partial row a tile.  The two
//                      counts are one integer atomic each a block.
//   k_register_reduce  the partial rows by the same shape again: a block a sum of a tile of 4096 rows
//   k_transform_points a thread per point: the pose's row expression; a skipped point is copied bit for bit
// No float atomics, no block waits for another: the record is bit-equal run to run and to the restatement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "mesh_lookup.h"

namespace {

using dsm::finite_bits;
using dsm::finite_host;
using dsm::frame_ok;
using dsm::too_long_a_side;
using dsm::too_many_cells;

constexpr uint32_t kTile = 4096;       // points a tile: 256 lanes x 16 entries
constexpr uint32_t kSums = 36;         // jtj[28], jte[7], ee: the record's doubles in its order
constexpr uint32_t kGroup = 12;        // sums folded a round: 12 x 256 doubles of LDS
constexpr uint32_t kMaxBlocks = 2048;  // 256 CUs x 8 blocks of 4 waves
static_assert(sizeof(ssrlcv_register_terms) == 304 && sizeof(ssrlcv_register_pose) == 60 && sizeof(ssrlcv_register_params) == 8, "the records of the header");
static_assert(kSums % kGroup == 0, "whole rounds");

__device__ __forceinline__ bool finite_f(float v) { return finite_bits(__float_as_uint(v)); }

// a point the rasterize rule skips: a component that is not finite, or (0, 0, 0) with either sign of zero
__device__ __forceinline__ bool skipped(const ssrlcv_float3& p) {
  const uint32_t bx = __float_as_uint(p.x), by = __float_as_uint(p.y), bz = __float_as_uint(p.z);
  return !finite_bits(bx) || !finite_bits(by) || !finite_bits(bz) || ((bx | by | bz) & 0x7FFFFFFFu) == 0u;
}

// p' = M p + T, a row (((m0 p.x) + (m1 p.y)) + (m2 p.z)) + m3
__device__ __forceinline__ ssrlcv_float3 posed(const ssrlcv_float3& p, const ssrlcv_register_pose& g) {
  ssrlcv_float3 q;
  q.x = (((g.m[0] * p.x) + (g.m[1] * p.y)) + (g.m[2] * p.z)) + g.m[3];
  q.y = (((g.m[4] * p.x) + (g.m[5] * p.y)) + (g.m[6] * p.z)) + g.m[7];
  q.z = (((g.m[8] * p.x) + (g.m[9] * p.y)) + (g.m[10] * p.z)) + g.m[11];
  return q;
}

// The row of one point: J[0..6] and J[7] = e, all zero for a point that is not used (its products are then +0.0).
__device__ __forceinline__ void point_row(const ssrlcv_float3& p, const ssrlcv_register_pose& g, const ssrlcv_dsm_frame& f, const float* __restrict__ height,
                                          const uint8_t* __restrict__ cells, float center, float gate, float (&J)[8], bool& inside, bool& used) {
  inside = used = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) J[k] = 0.0f;
  if (skipped(p)) return;
  const ssrlcv_float3 q = posed(p, g);
  float u, v, z, d, rs, rt;
  if (!dsm::point_uvz(q, f, u, v, z) || !finite_f(z)) return;
  if (!dsm::mesh_difference(u, v, z, height, cells, f.w, f.h, d, rs, rt)) return;
  inside = true;
  const float gu = __fdiv_rn(rs, f.cell), gv = __fdiv_rn(rt, f.cell);
  const float Gx = (f.ez[0] - (gu * f.ex[0])) - (gv * f.ey[0]);
  const float Gy = (f.ez[1] - (gu * f.ex[1])) - (gv * f.ey[1]);
  const float Gz = (f.ez[2] - (gu * f.ex[2])) - (gv * f.ey[2]);
  const float len = sqrtf(((Gx * Gx) + (Gy * Gy)) + (Gz * Gz));  // correctly rounded (HIP's default), as the divisions are
  const float Nx = __fdiv_rn(Gx, len), Ny = __fdiv_rn(Gy, len), Nz = __fdiv_rn(Gz, len);
  const float e = __fdiv_rn(d, len);
  const float Lx = q.x - g.pivot[0], Ly = q.y - g.pivot[1], Lz = q.z - g.pivot[2];
  float R[8];
  R[0] = Nx, R[1] = Ny, R[2] = Nz;
  R[3] = (Ly * Nz) - (Lz * Ny);
  R[4] = (Lz * Nx) - (Lx * Nz);
  R[5] = (Lx * Ny) - (Ly * Nx);
  R[6] = ((Lx * Nx) + (Ly * Ny)) + (Lz * Nz);
  R[7] = e;
  bool fin = fabsf(d - center) <= gate;  // false for a NaN
#pragma unroll
  for (int k = 0; k < 8; ++k) fin = fin && finite_f(R[k]);
  if (!fin) return;
  used = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) J[k] = R[k];
}

// the 256 lane values of kGroup sums folded by halves (128, 64 through LDS; 32 .. 1 inside wave 0): thread 0 holds the tile's sums
__device__ __forceinline__ void fold_group(double* v, double (*fold)[256]) {
  const uint32_t l = threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kGroup; ++k) fold[k][l] = v[k];
  __syncthreads();
  if (l < 64u) {
#pragma unroll
    for (uint32_t k = 0; k < kGroup; ++k) {
      double s = (fold[k][l] + fold[k][l + 128u]) + (fold[k][l + 64u] + fold[k][l + 192u]);
#pragma unroll
      for (int half = 32; half >= 1; half >>= 1) s += __shfl_down(s, half, 64);
      v[k] = s;
    }
  }
  __syncthreads();  // the fold arrays are free again
}

// sums[i * stride + tile], i < 36: the sums of a tile
__global__ __launch_bounds__(256) void k_register_terms(const ssrlcv_float3* __restrict__ points, uint32_t n, uint32_t tiles, ssrlcv_register_pose g,
                                                        const float* __restrict__ height, ssrlcv_dsm_frame f, const uint8_t* __restrict__ cells,
                                                        float center, float gate, ssrlcv_register_terms* __restrict__ out, double* __restrict__ sums,
                                                        uint32_t stride) {
  __shared__ double fold[kGroup][256];
  __shared__ uint32_t red[4][2];
  const uint32_t l = threadIdx.x;
  uint32_t nInside = 0, nUsed = 0;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned long long base = (unsigned long long)tile * kTile + l;
    double acc[kSums];
#pragma unroll
    for (uint32_t i = 0; i < kSums; ++i) acc[i] = 0.0;
#pragma unroll 2  // measured: 2 (120 VGPRs, 4 waves a SIMD) beats 4, 8 and 16 in raster order (profiles/register_bench.txt)
    for (int r = 0; r < 16; ++r) {
      const unsigned long long at = base + 256u * (unsigned)r;
      float J[8];
      bool inside = false, used = false;
      if (at < n) {
        point_row(points[at], g, f, height, cells, center, gate, J, inside, used);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) J[k] = 0.0f;  // padding adds +0.0
      }
      nInside += inside ? 1u : 0u;
      nUsed += used ? 1u : 0u;
      double D[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) D[k] = (double)J[k];
      // a product of two floats is exact in float64, so the fused multiply-add rounds once, as the product and the sum would
      uint32_t at36 = 0;
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = i; j < 7; ++j) {
          acc[at36] = fma(D[i], D[j], acc[at36]);
          ++at36;
        }
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[28 + i] = fma(D[i], D[7], acc[28 + i]);
      acc[35] = fma(D[7], D[7], acc[35]);
    }
#pragma unroll
    for (uint32_t gr = 0; gr < kSums; gr += kGroup) fold_group(acc + gr, fold);
    if (l == 0u) {
#pragma unroll
      for (uint32_t i = 0; i < kSums; ++i) sums[(size_t)i * stride + tile] = acc[i];
    }
  }
  // the block's counts: shuffles inside a wave, two words a wave through LDS, one atomic each
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    nInside += __shfl_down(nInside, o, 64);
    nUsed += __shfl_down(nUsed, o, 64);
  }
  if ((l & 63u) == 0u) red[l >> 6][0] = nInside, red[l >> 6][1] = nUsed;
  __syncthreads();
  if (l == 0u) {
    atomicAdd(&out->inside, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    atomicAdd(&out->used, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
    if (blockIdx.x == 0u) out->n = n;  // the head of the record was cleared before the launch
  }
}

// out[i * outStride + blockIdx.x] = the sum of in[i * count + ...], a tile of 4096 partials, i = blockIdx.y
__global__ __launch_bounds__(256) void k_register_reduce(const double* __restrict__ in, uint32_t count, double* __restrict__ out, uint32_t outStride) {
  __shared__ double fold[256];
  const uint32_t l = threadIdx.x;
  const double* row = in + (size_t)blockIdx.y * count;
  const unsigned long long base = (unsigned long long)blockIdx.x * kTile + l;
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const unsigned long long at = base + 256u * (unsigned)r;
    s += at < count ? row[at] : 0.0;
  }
  fold[l] = s;
  __syncthreads();
  if (l < 64u) {
    s = (fold[l] + fold[l + 128u]) + (fold[l + 64u] + fold[l + 192u]);
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) s += __shfl_down(s, half, 64);
    if (l == 0u) out[(size_t)blockIdx.y * outStride + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void k_transform_points(const ssrlcv_float3* points, uint32_t n, ssrlcv_register_pose g, ssrlcv_float3* out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // below 2^32: at most 2^24 blocks
  if (t >= n) return;
  const ssrlcv_float3 p = points[t];  // out may be points: a thread reads its point before it writes it
  out[t] = skipped(p) ? p : posed(p, g);
}

// ---- host side
uint32_t tiles_of(uint32_t n) { return (uint32_t)(((unsigned long long)n + kTile - 1u) / kTile); }
size_t partial_bytes(uint32_t rows) { return align256((size_t)rows * kSums * sizeof(double)); }
size_t terms_bytes(uint32_t n) { return partial_bytes(tiles_of(n)) + partial_bytes(tiles_of(tiles_of(n))); }

bool pose_ok(const ssrlcv_register_pose* p) {
  if (!p) return false;
  for (int k = 0; k < 12; ++k)
    if (!finite_host(p->m[k])) return false;
  return finite_host(p->pivot[0]) && finite_host(p->pivot[1]) && finite_host(p->pivot[2]);
}

bool params_ok(const ssrlcv_register_params* p) { return p && finite_host(p->center) && p->gate >= 0.0f; }  // a NaN gate fails; +inf is legal

bool finite_d(double v) { return v - v == 0.0; }

}  // namespace

extern "C" {

size_t ssrlcv_hip_register_terms_workspace_bytes(uint32_t n) { return terms_bytes(n); }

int ssrlcv_hip_register_terms(const ssrlcv_float3* points, uint32_t n, const ssrlcv_register_pose* pose, const float* height, const ssrlcv_dsm_frame* frame,
                              const uint8_t* cells, const ssrlcv_register_params* params, ssrlcv_register_terms* out_dev, void* workspace,
                              size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (!frame_ok(frame) || too_many_cells(frame->w, frame->h)) return SSRLCV_ERR_INVALID_ARG;
  if (!pose_ok(pose) || !params_ok(params)) return SSRLCV_ERR_INVALID_ARG;
  if (too_long_a_side(frame->w, frame->h)) return SSRLCV_ERR_UNSUPPORTED;
  if (!out_dev) return SSRLCV_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // the empty record -- zeros and +0.0 -- and nothing else is looked at
    SSRLCV_HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(ssrlcv_register_terms), st));
    return SSRLCV_OK;
  }
  if (!points || !height || !cells || !workspace) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < terms_bytes(n)) return SSRLCV_ERR_WORKSPACE;
  const uint32_t t1 = tiles_of(n), t2 = tiles_of(t1);
  double* partial1 = (double*)workspace;
  double* partial2 = (double*)((unsigned char*)workspace + partial_bytes(t1));
  double* record = out_dev->jtj;  // jtj, jte and ee: 36 doubles in a row
  SSRLCV_HIP_TRY(hipMemsetAsync(out_dev, 0, 16, st));  // n, inside, used, reserved
  const dim3 walkers(t1 < kMaxBlocks ? t1 : kMaxBlocks);
  // one tile: its sums are the record's
  hipLaunchKernelGGL(k_register_terms, walkers, dim3(256), 0, st, points, n, t1, *pose, height, *frame, cells, params->center, params->gate, out_dev,
                     t1 > 1u ? partial1 : record, t1 > 1u ? t1 : 1u);
  SSRLCV_LAUNCH_CHECK();
  if (t1 > 1u) {
    hipLaunchKernelGGL(k_register_reduce, dim3(t2, kSums), dim3(256), 0, st, partial1, t1, t2 > 1u ? partial2 : record, t2 > 1u ? t2 : 1u);
    SSRLCV_LAUNCH_CHECK();
    if (t2 > 1u) {  // at most 256 second-level rows: the third level is one tile
      hipLaunchKernelGGL(k_register_reduce, dim3(1, kSums), dim3(256), 0, st, partial2, t2, record, 1u);
      SSRLCV_LAUNCH_CHECK();
    }
  }
  return SSRLCV_OK;
}

int ssrlcv_hip_transform_points(const ssrlcv_float3* points, uint32_t n, const ssrlcv_register_pose* pose, ssrlcv_float3* out, ssrlcv_stream_t stream) {
  if (!pose_ok(pose)) return SSRLCV_ERR_INVALID_ARG;
  if (n == 0) return SSRLCV_OK;
  if (!points || !out) return SSRLCV_ERR_INVALID_ARG;
  if (out != points) {  // partial overlap
    const uintptr_t a = (uintptr_t)points, b = (uintptr_t)out, bytes = (uintptr_t)n * sizeof(ssrlcv_float3);
    if (a < b + bytes && b < a + bytes) return SSRLCV_ERR_INVALID_ARG;
  }
  const dim3 blocks((uint32_t)(((unsigned long long)n + 255u) / 256u));
  hipLaunchKernelGGL(k_transform_points, blocks, dim3(256), 0, (hipStream_t)stream, points, n, *pose, out);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

// H delta = -jte over the masked unknowns, H = jtj with its diagonal times (1 + lambda), by Cholesky in its root-free form
// L D L^T: a pivot D_k that is not above 2^-30 of the diagonal entry it started as is a direction the points do not hold.
int ssrlcv_register_step_host(const ssrlcv_register_terms* record, uint32_t dofMask, double lambda, double* delta) {
  if (!record || !delta || dofMask == 0u || dofMask > 0x7Fu || !(lambda >= 0.0) || !finite_d(lambda)) return SSRLCV_ERR_INVALID_ARG;
  if (record->used == 0u) return SSRLCV_ERR_UNSUPPORTED;
  double full[7][7];
  for (int i = 0, at = 0; i < 7; ++i)
    for (int j = i; j < 7; ++j, ++at) full[i][j] = full[j][i] = record->jtj[at];
  int idx[7], m = 0;
  for (int k = 0; k < 7; ++k)
    if (dofMask >> k & 1u) idx[m++] = k;
  double A[7][7], L[7][7], D[7], y[7];
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) A[i][j] = full[idx[i]][idx[j]] * (i == j ? 1.0 + lambda : 1.0);
  for (int k = 0; k < m; ++k) {
    double d = A[k][k];
    for (int j = 0; j < k; ++j) d -= L[k][j] * L[k][j] * D[j];
    if (!(d > A[k][k] * 0x1p-30) || !finite_d(d)) return SSRLCV_ERR_UNSUPPORTED;
    D[k] = d;
    for (int i = k + 1; i < m; ++i) {
      double s = A[i][k];
      for (int j = 0; j < k; ++j) s -= L[i][j] * L[k][j] * D[j];
      L[i][k] = s / d;
    }
  }
  for (int i = 0; i < m; ++i) {  // L y = -jte
    double s = -record->jte[idx[i]];
    for (int j = 0; j < i; ++j) s -= L[i][j] * y[j];
    y[i] = s;
  }
  double x[7];
  for (int i = m - 1; i >= 0; --i) {  // L^T x = y / D
    double s = y[i] / D[i];
    for (int j = i + 1; j < m; ++j) s -= L[j][i] * x[j];
    x[i] = s;
  }
  for (int k = 0; k < m; ++k)
    if (!finite_d(x[k])) return SSRLCV_ERR_UNSUPPORTED;
  for (int k = 0; k < 7; ++k) delta[k] = 0.0;
  for (int k = 0; k < m; ++k) delta[idx[k]] = x[k];
  return SSRLCV_OK;
}

// p'' = pivot + (1 + ds) R(dw) (p' - pivot) + dt: M <- (1 + ds) R M, T <- pivot + (1 + ds) R (T - pivot) + dt, in double, rounded once
int ssrlcv_register_compose_host(const ssrlcv_register_pose* pose, const double* delta, ssrlcv_register_pose* out) {
  if (!pose_ok(pose) || !delta || !out) return SSRLCV_ERR_INVALID_ARG;
  for (int k = 0; k < 7; ++k)
    if (!finite_d(delta[k])) return SSRLCV_ERR_INVALID_ARG;
  const double wx = delta[3], wy = delta[4], wz = delta[5];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  double a = 1.0, b = 0.5;  // sin(theta) / theta and (1 - cos(theta)) / theta^2, their limits below 2^-26
  if (theta >= 0x1p-26) {
    const double h = sin(0.5 * theta) / (0.5 * theta);
    a = sin(theta) / theta;
    b = 0.5 * h * h;
  }
  // Rodrigues: R = I + a K + b K^2, K the cross-product matrix of the rotation vector
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double R[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double k2 = 0.0;
      for (int k = 0; k < 3; ++k) k2 += K[i][k] * K[k][j];
      R[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * k2;
    }
  const double s = 1.0 + delta[6];
  ssrlcv_register_pose next;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += R[i][k] * (double)pose->m[4 * k + j];
      next.m[4 * i + j] = (float)(s * v);
    }
    double v = 0.0;
    for (int k = 0; k < 3; ++k) v += R[i][k] * ((double)pose->m[4 * k + 3] - (double)pose->pivot[k]);
    next.m[4 * i + 3] = (float)(((double)pose->pivot[i] + s * v) + delta[i]);
    next.pivot[i] = pose->pivot[i];
  }
  for (int k = 0; k < 12; ++k)
    if (!finite_host(next.m[k])) return SSRLCV_ERR_UNSUPPORTED;
  *out = next;
  return SSRLCV_OK;
}

}  // extern "C"
