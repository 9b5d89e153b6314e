// ssrlcv_amd/csrc/ransac.hip -- PoseEstimator::estimatePoseRANSAC on the device: 7-point fundamental-matrix RANSAC with a
// fixed sample count, one least-squares refit, and the relative pose from the essential matrix.  The conventions (match
// layout, normalisation, sample hash, scoring, tie-breaks) are stated in include/ssrlcv_hip.h and DESIGN.md section 4.
//
// Stream-ordered pipeline of ssrlcv_hip_fmatrix_ransac (no host round trip, capturable):
//   k_bbox / k_norm      bounding box of the valid match locations -> one similarity transform per image, common scale
//   k_sample_solve       one thread per sample: hash -> 7 indices -> float64 7x9 null space -> cubic -> <= 3 candidates
//   k_fmatrix_score      THE HOT PATH: candidates x matches Sampson tests, integer counts (ballot + popcount)
//   k_best               argmax (count, lowest slot) through one 64-bit atomicMax per wave
//   k_refit_accum/solve  9x9 float64 normal matrix over the winner's inliers (per-block partials, fixed-order sum),
//                        Jacobi eigenvector in one wave, rank 2 through the smallest right singular vector
//   k_fmatrix_score      the refit, then k_finalize keeps it when it has at least as many inliers
#include <hip/hip_runtime.h>
#include <cmath>
#include "align256.h"
#include "device_math.h"
#include "ssrlcv_hip.h"

namespace {

// Workspace header (the first kHdrBytes of every workspace this file uses).  Zeroed by hipMemsetAsync before use: the
// box holds order-preserving keys, maxima as max(key) and minima as max(~key), so zero is the identity of both.
struct FmHdr {
  uint32_t boxMaxNot[4];  // ~key(min) of q.x, q.y, t.x, t.y
  uint32_t boxMax[4];     // key(max)
  uint32_t nvalid;
  uint32_t refitCount;
  unsigned long long best;  // (count << 32) | ~slot
  uint32_t votes[4];        // cheirality votes (pose_from_fmatrix)
  uint32_t maskCount;       // scratch count of the final mask pass
  int ok;                   // >= 7 valid matches and a box of non-zero extent
  float cq[2], ct[2], s;    // float transform (scoring): x_n = (x - c) * s
  double dcq[2], dct[2], ds;  // float64 transform (solver, refit, denormalisation)
};
constexpr size_t kHdrBytes = SSRLCV_FMATRIX_AUX_WORKSPACE_BYTES;
static_assert(sizeof(FmHdr) <= kHdrBytes, "FmHdr");

constexpr int kScoreThreads = 256;
constexpr int kScoreP = 4;                               // matches per lane
constexpr int kScoreMatchTile = kScoreThreads * kScoreP;  // matches per block
constexpr int kScoreChunk = 256;                          // candidates staged in LDS at a time
constexpr int kRefitBlocksMax = 256;

inline uint32_t refit_blocks(uint32_t n) {
  uint32_t b = (n + 255) / 256;
  return b < 1 ? 1 : b > kRefitBlocksMax ? kRefitBlocksMax : b;
}

struct RansacLayout {
  size_t cand, counts, refitF, partials, total;
};
inline RansacLayout ransac_layout(uint32_t numMatches, uint32_t numSamples) {
  RansacLayout L;
  L.cand = kHdrBytes;
  L.counts = L.cand + align256((size_t)27 * numSamples * sizeof(float));
  L.refitF = L.counts + align256((size_t)3 * numSamples * sizeof(uint32_t));
  L.partials = L.refitF + 256;
  L.total = L.partials + align256((size_t)refit_blocks(numMatches) * 45 * sizeof(double));
  return L;
}

__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fdekey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void k_bbox(const ssrlcv_match* __restrict__ m, uint32_t n, FmHdr* __restrict__ h) {
  float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  uint32_t valid = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (m[i].invalid) continue;
    const float v[4] = {m[i].keyPoints[0].loc.x, m[i].keyPoints[0].loc.y, m[i].keyPoints[1].loc.x, m[i].keyPoints[1].loc.y};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo[k] = fminf(lo[k], v[k]);
      hi[k] = fmaxf(hi[k], v[k]);
    }
    ++valid;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64));
    }
    valid += __shfl_xor(valid, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && valid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      atomicMax(&h->boxMaxNot[k], ~fkey(lo[k]));
      atomicMax(&h->boxMax[k], fkey(hi[k]));
    }
    atomicAdd(&h->nvalid, valid);
  }
}

__global__ void k_norm(FmHdr* __restrict__ h) {
  double lo[4], hi[4], ext = 0;
  for (int k = 0; k < 4; ++k) {
    lo[k] = h->nvalid ? (double)fdekey(~h->boxMaxNot[k]) : 0.0;
    hi[k] = h->nvalid ? (double)fdekey(h->boxMax[k]) : 0.0;
    ext = fmax(ext, hi[k] - lo[k]);
  }
  h->ok = h->nvalid >= 7 && ext > 0;
  h->ds = ext > 0 ? 2.0 / ext : 1.0;
  h->s = (float)h->ds;
  for (int k = 0; k < 2; ++k) {
    h->dcq[k] = 0.5 * (lo[k] + hi[k]);
    h->dct[k] = 0.5 * (lo[k + 2] + hi[k + 2]);
    h->cq[k] = (float)h->dcq[k];
    h->ct[k] = (float)h->dct[k];
  }
}

// ---------------------------------------------------------------------------------------------- shared F arithmetic
// pixel F -> normalised F:  F_n = A_t^T F A_q,  A = T^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]], scaled to unit
// Frobenius norm; computed in float64 from the float pixel entries, so every kernel that scores a given pixel F tests
// the matches against the same float F_n.
__device__ __forceinline__ void normalise_f(const float* __restrict__ Fp, const FmHdr* __restrict__ h, float (&Fn)[9]) {
  double F[9], M[9];
  for (int i = 0; i < 9; ++i) F[i] = Fp[i];
  const double is = 1.0 / h->ds;
  for (int r = 0; r < 3; ++r) {
    M[3 * r + 0] = F[3 * r + 0] * is;
    M[3 * r + 1] = F[3 * r + 1] * is;
    M[3 * r + 2] = h->dcq[0] * F[3 * r + 0] + h->dcq[1] * F[3 * r + 1] + F[3 * r + 2];
  }
  double nrm = 0;
  for (int c = 0; c < 3; ++c) {
    F[c] = M[c] * is;
    F[3 + c] = M[3 + c] * is;
    F[6 + c] = h->dct[0] * M[c] + h->dct[1] * M[3 + c] + M[6 + c];
  }
  for (int i = 0; i < 9; ++i) nrm += F[i] * F[i];
  const double inv = nrm > 0 ? 1.0 / sqrt(nrm) : 0.0;
  for (int i = 0; i < 9; ++i) Fn[i] = (float)(F[i] * inv);
}

// normalised float64 F -> pixel float F (F_p = T_t^T F_n T_q), unit Frobenius norm, largest |entry| positive
__device__ void denormalise_f(const double (&Fn)[9], const FmHdr* __restrict__ h, float* __restrict__ out) {
  double M[9], F[9];
  const double s = h->ds;
  for (int r = 0; r < 3; ++r) {
    M[3 * r + 0] = s * Fn[3 * r + 0];
    M[3 * r + 1] = s * Fn[3 * r + 1];
    M[3 * r + 2] = Fn[3 * r + 2] - s * h->dcq[0] * Fn[3 * r + 0] - s * h->dcq[1] * Fn[3 * r + 1];
  }
  for (int c = 0; c < 3; ++c) {
    F[c] = s * M[c];
    F[3 + c] = s * M[3 + c];
    F[6 + c] = M[6 + c] - s * h->dct[0] * M[c] - s * h->dct[1] * M[3 + c];
  }
  double nrm = 0;
  for (int i = 0; i < 9; ++i) nrm += F[i] * F[i];
  const double inv = nrm > 0 ? 1.0 / sqrt(nrm) : 0.0;
  float f[9];
  int big = 0;
  for (int i = 0; i < 9; ++i) {
    f[i] = (float)(F[i] * inv);
    if (fabsf(f[i]) > fabsf(f[big])) big = i;
  }
  const float sign = f[big] < 0 ? -1.0f : 1.0f;
  for (int i = 0; i < 9; ++i) out[i] = sign * f[i];
}

// normalised coordinates of match i; NaN for an invalid or absent match (a NaN never passes the inlier test)
__device__ __forceinline__ void load_norm(const ssrlcv_match* __restrict__ m, uint32_t n, uint32_t i,
                                          const FmHdr* __restrict__ h, float& x, float& y, float& u, float& v) {
  x = y = u = v = __builtin_nanf("");
  if (i < n && !m[i].invalid) {
    const ssrlcv_float2 q = m[i].keyPoints[0].loc, t = m[i].keyPoints[1].loc;
    x = (q.x - h->cq[0]) * h->s;
    y = (q.y - h->cq[1]) * h->s;
    u = (t.x - h->ct[0]) * h->s;
    v = (t.y - h->ct[1]) * h->s;
  }
}

// Sampson test r^2 < thr2 * den, written as fma(-thr2, den, r^2) < 0: false for den == 0 and for NaN
__device__ __forceinline__ bool sampson_in(float f0, float f1, float f2, float f3, float f4, float f5, float f6,
                                           float f7, float f8, float x, float y, float u, float v, float thr2) {
  const float a = fmaf(f0, x, fmaf(f1, y, f2));  // (F q)_0
  const float b = fmaf(f3, x, fmaf(f4, y, f5));  // (F q)_1
  const float c = fmaf(f6, x, fmaf(f7, y, f8));  // (F q)_2
  const float d = fmaf(f0, u, fmaf(f3, v, f6));  // (F^T t)_0
  const float e = fmaf(f1, u, fmaf(f4, v, f7));  // (F^T t)_1
  const float r = fmaf(u, a, fmaf(v, b, c));     // t^T F q
  const float den = fmaf(a, a, fmaf(b, b, fmaf(d, d, e * e)));
  return fmaf(-thr2, den, r * r) < 0.0f;
}

// ---------------------------------------------------------------------------------------------- the hot path
// grid (match tiles, candidate ranges).  Each lane holds kScoreP matches in VGPRs; the block stages up to kScoreChunk
// normalised candidates in LDS and every wave walks them: per candidate 9 broadcast LDS reads into VGPRs, then per
// match one Sampson test whose v_cmp mask is popcounted into a scalar.  Per-wave counts meet in LDS; one atomicAdd per
// (block, candidate) with a non-zero count.  kMask (k == 1 only): the per-match result is written as well.
template <bool kMask>
__global__ __launch_bounds__(kScoreThreads) void k_fmatrix_score(const ssrlcv_match* __restrict__ m, uint32_t n,
                                                                 const float* __restrict__ F, uint32_t k,
                                                                 uint32_t candPerBlock, float threshold,
                                                                 const FmHdr* __restrict__ h,
                                                                 uint32_t* __restrict__ counts,
                                                                 uint8_t* __restrict__ mask) {
  __shared__ float sF[kScoreChunk][9];
  __shared__ uint32_t sCount[kScoreThreads / 64][kScoreChunk];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  float x[kScoreP], y[kScoreP], u[kScoreP], v[kScoreP];
  const uint32_t base = blockIdx.x * kScoreMatchTile + tid;
#pragma unroll
  for (int p = 0; p < kScoreP; ++p) load_norm(m, n, base + p * kScoreThreads, h, x[p], y[p], u[p], v[p]);
  const float ts = h->s * threshold, thr2 = ts * ts;
  const uint32_t c0 = blockIdx.y * candPerBlock, c1 = min(k, c0 + candPerBlock);
  for (uint32_t cb = c0; cb < c1; cb += kScoreChunk) {
    const uint32_t nc = min((uint32_t)kScoreChunk, c1 - cb);
    if (tid < nc) {
      float Fn[9];
      normalise_f(F + 9 * (size_t)(cb + tid), h, Fn);
#pragma unroll
      for (int i = 0; i < 9; ++i) sF[tid][i] = Fn[i];
    }
    __syncthreads();
    for (uint32_t c = 0; c < nc; ++c) {
      const float f0 = sF[c][0], f1 = sF[c][1], f2 = sF[c][2], f3 = sF[c][3], f4 = sF[c][4], f5 = sF[c][5],
                  f6 = sF[c][6], f7 = sF[c][7], f8 = sF[c][8];
      uint32_t cnt = 0;
#pragma unroll
      for (int p = 0; p < kScoreP; ++p) {
        const bool in = sampson_in(f0, f1, f2, f3, f4, f5, f6, f7, f8, x[p], y[p], u[p], v[p], thr2);
        cnt += __popcll(__ballot(in));
        if (kMask) {
          const uint32_t i = base + p * kScoreThreads;
          if (i < n) mask[i] = in;
        }
      }
      if ((tid & 63) == 0) sCount[wave][c] = cnt;
    }
    __syncthreads();
    if (tid < nc) {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < kScoreThreads / 64; ++w) s += sCount[w][tid];
      if (s) atomicAdd(counts + cb + tid, s);
    }
    __syncthreads();
  }
}

// launch shape: enough (match tile, candidate range) blocks to give every CU several, candidate ranges never below one
// LDS chunk's worth unless k itself is smaller
inline int launch_score(const ssrlcv_match* m, uint32_t n, const float* F, uint32_t k, float threshold, const FmHdr* h,
                        uint32_t* counts, uint8_t* mask, hipStream_t st) {
  const uint32_t tiles = (n + kScoreMatchTile - 1) / kScoreMatchTile;
  const uint32_t want = 2048;  // 256 CUs x 8 blocks
  uint32_t ranges = (want + tiles - 1) / tiles;
  const uint32_t maxRanges = (k + 31) / 32;  // at least 32 candidates per block
  if (ranges > maxRanges) ranges = maxRanges;
  if (ranges < 1) ranges = 1;
  const uint32_t per = (k + ranges - 1) / ranges;
  ranges = (k + per - 1) / per;
  if (mask)
    hipLaunchKernelGGL(k_fmatrix_score<true>, dim3(tiles, ranges), dim3(kScoreThreads), 0, st, m, n, F, k, per, threshold,
                       h, counts, mask);
  else
    hipLaunchKernelGGL(k_fmatrix_score<false>, dim3(tiles, ranges), dim3(kScoreThreads), 0, st, m, n, F, k, per, threshold,
                       h, counts, mask);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

// ---------------------------------------------------------------------------------------------- sampler + solver
__device__ __forceinline__ uint32_t sample_index(uint64_t seed, uint32_t h, uint32_t j, uint32_t n) {
  uint64_t z = seed + (((uint64_t)h << 32) + j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);
}

__device__ double det3(const double (&F)[9]) {
  return F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
}

// real roots of c3 a^3 + c2 a^2 + c1 a + c0, ascending; the degree drops when the leading coefficient vanishes
// (|c3| <= 1e-12 of the largest coefficient)
__device__ int real_roots(double c3, double c2, double c1, double c0, double (&r)[3]) {
  const double big = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
  if (big == 0) return 0;
  int nr = 0;
  if (fabs(c3) <= 1e-12 * big) {
    if (fabs(c2) <= 1e-12 * big) {
      if (c1 == 0) return 0;
      r[0] = -c0 / c1;
      return 1;
    }
    const double disc = c1 * c1 - 4 * c2 * c0;
    if (disc < 0) return 0;
    const double q = -0.5 * (c1 + (c1 < 0 ? -sqrt(disc) : sqrt(disc)));
    r[nr++] = q / c2;
    if (q != 0) r[nr++] = c0 / q;
  } else {
    const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const double Q = (a * a - 3 * b) / 9, R = (2 * a * a * a - 9 * a * b + 27 * c) / 54;
    const double Q3 = Q * Q * Q;
    if (R * R < Q3) {
      const double th = acos(R / sqrt(Q3)), sq = -2 * sqrt(Q);
      r[0] = sq * cos(th / 3) - a / 3;
      r[1] = sq * cos((th + 2 * M_PI) / 3) - a / 3;
      r[2] = sq * cos((th - 2 * M_PI) / 3) - a / 3;
      nr = 3;
    } else {
      double A = -cbrt(fabs(R) + sqrt(R * R - Q3));
      if (R < 0) A = -A;
      const double B = A != 0 ? Q / A : 0;
      r[0] = A + B - a / 3;
      nr = 1;
    }
    for (int i = 0; i < nr; ++i)  // two Newton steps on the monic cubic
      for (int it = 0; it < 2; ++it) {
        const double x = r[i], f = ((x + a) * x + b) * x + c, df = (3 * x + 2 * a) * x + b;
        if (df != 0) r[i] = x - f / df;
      }
  }
  for (int i = 1; i < nr; ++i)
    for (int j = i; j > 0 && r[j] < r[j - 1]; --j) {
      const double t = r[j];
      r[j] = r[j - 1];
      r[j - 1] = t;
    }
  return nr;
}

__global__ __launch_bounds__(64) void k_sample_solve(const ssrlcv_match* __restrict__ m, uint32_t n, uint32_t S,
                                                     uint64_t seed, const FmHdr* __restrict__ hdr,
                                                     float* __restrict__ cand) {
  const uint32_t hs = blockIdx.x * blockDim.x + threadIdx.x;
  if (hs >= S) return;
  float* out = cand + 27 * (size_t)hs;
  for (int i = 0; i < 27; ++i) out[i] = 0.0f;
  if (!hdr->ok) return;
  uint32_t idx[7];
  int got = 0;
  for (uint32_t j = 0; j < 64 && got < 7; ++j) {
    const uint32_t c = sample_index(seed, hs, j, n);
    bool dup = false;
    for (int i = 0; i < got; ++i) dup |= idx[i] == c;
    if (!dup) idx[got++] = c;
  }
  if (got < 7) return;
  double A[7][9];
  for (int i = 0; i < 7; ++i) {
    const ssrlcv_match& mm = m[idx[i]];
    if (mm.invalid) return;
    const double x = ((double)mm.keyPoints[0].loc.x - hdr->dcq[0]) * hdr->ds, y = ((double)mm.keyPoints[0].loc.y - hdr->dcq[1]) * hdr->ds;
    const double u = ((double)mm.keyPoints[1].loc.x - hdr->dct[0]) * hdr->ds, v = ((double)mm.keyPoints[1].loc.y - hdr->dct[1]) * hdr->ds;
    const double row[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};  // t^T F q with F row-major
    for (int c = 0; c < 9; ++c) A[i][c] = row[c];
  }
  // null space: Householder reflections from the right, A H_0 ... H_6 = [L | 0]; F1, F2 = H_0 ... H_6 e_7, e_8
  double V[7][9];
  for (int kk = 0; kk < 7; ++kk) {
    double nrm = 0;
    for (int c = kk; c < 9; ++c) nrm += A[kk][c] * A[kk][c];
    nrm = sqrt(nrm);
    for (int c = 0; c < 9; ++c) V[kk][c] = 0;
    if (nrm == 0) continue;
    for (int c = kk; c < 9; ++c) V[kk][c] = A[kk][c];
    V[kk][kk] += A[kk][kk] < 0 ? -nrm : nrm;
    double vv = 0;
    for (int c = kk; c < 9; ++c) vv += V[kk][c] * V[kk][c];
    for (int r = kk; r < 7; ++r) {
      double d = 0;
      for (int c = kk; c < 9; ++c) d += A[r][c] * V[kk][c];
      d = 2 * d / vv;
      for (int c = kk; c < 9; ++c) A[r][c] -= d * V[kk][c];
    }
    for (int c = kk; c < 9; ++c) V[kk][c] /= sqrt(vv);  // unit reflector
  }
  double N[2][9];
  for (int b = 0; b < 2; ++b) {
    for (int c = 0; c < 9; ++c) N[b][c] = c == 7 + b ? 1.0 : 0.0;
    for (int kk = 6; kk >= 0; --kk) {
      double d = 0;
      for (int c = 0; c < 9; ++c) d += V[kk][c] * N[b][c];
      for (int c = 0; c < 9; ++c) N[b][c] -= 2 * d * V[kk][c];
    }
  }
  // det(a F1 + (1 - a) F2) = det(F2 + a D): cubic through its values at a = 0, 1, -1, 2
  double G[9], dv[4];
  const double at[4] = {0, 1, -1, 2};
  for (int p = 0; p < 4; ++p) {
    for (int c = 0; c < 9; ++c) G[c] = N[1][c] + at[p] * (N[0][c] - N[1][c]);
    dv[p] = det3(G);
  }
  const double c0 = dv[0], c2 = 0.5 * (dv[1] + dv[2]) - dv[0];
  const double c3 = (dv[3] - 4 * c2 - c0 - (dv[1] - dv[2])) / 6, c1 = 0.5 * (dv[1] - dv[2]) - c3;
  double roots[3];
  const int nr = real_roots(c3, c2, c1, c0, roots);
  for (int r = 0; r < nr; ++r) {
    for (int c = 0; c < 9; ++c) G[c] = roots[r] * N[0][c] + (1 - roots[r]) * N[1][c];
    denormalise_f(G, hdr, out + 9 * r);
  }
}

__global__ __launch_bounds__(256) void k_best(const uint32_t* __restrict__ counts, uint32_t k, FmHdr* __restrict__ h) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long key = i < k ? ((unsigned long long)counts[i] << 32) | (uint32_t)~i : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&h->best, key);
}

// ---------------------------------------------------------------------------------------------- refit
__device__ __forceinline__ const float* best_f(const float* cand, const FmHdr* h) {
  return cand + 9 * (size_t)(~(uint32_t)h->best);
}

// partials[block][45]: upper triangle (row-major, i <= j) of sum a a^T, a = kron(t~_n, q~_n), over the winner's inliers
__global__ __launch_bounds__(256) void k_refit_accum(const ssrlcv_match* __restrict__ m, uint32_t n,
                                                     const float* __restrict__ cand, float threshold,
                                                     const FmHdr* __restrict__ h, double* __restrict__ partials) {
  __shared__ double sw[4][45];
  double acc[45];
  for (int e = 0; e < 45; ++e) acc[e] = 0;
  if ((h->best >> 32) != 0) {
    float Fn[9];
    normalise_f(best_f(cand, h), h, Fn);
    const float ts = h->s * threshold, thr2 = ts * ts;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      float x, y, u, v;
      load_norm(m, n, i, h, x, y, u, v);
      if (!sampson_in(Fn[0], Fn[1], Fn[2], Fn[3], Fn[4], Fn[5], Fn[6], Fn[7], Fn[8], x, y, u, v, thr2)) continue;
      const double a[9] = {(double)u * x, (double)u * y, (double)u, (double)v * x, (double)v * y, (double)v, (double)x, (double)y, 1.0};
      int e = 0;
      for (int r = 0; r < 9; ++r)
        for (int c = r; c < 9; ++c) acc[e++] += a[r] * a[c];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = 0; e < 45; ++e) {
    double s = acc[e];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sw[wave][e] = s;
  }
  __syncthreads();
  if (threadIdx.x < 45)
    partials[45 * (size_t)blockIdx.x + threadIdx.x] =
        ((sw[0][threadIdx.x] + sw[1][threadIdx.x]) + sw[2][threadIdx.x]) + sw[3][threadIdx.x];
}

// cyclic Jacobi on a symmetric n x n matrix (row-major, overwritten); V receives the eigenvectors as columns
__device__ void jacobi_eig(double* A, double* V, int n) {
  for (int i = 0; i < n * n; ++i) V[i] = (i % (n + 1)) == 0 ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0, diag = 0;
    for (int p = 0; p < n; ++p)
      for (int q = 0; q < n; ++q) (p == q ? diag : off) += A[p * n + q] * A[p * n + q];
    if (off <= 1e-30 * diag || off == 0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0) continue;
        const double th = (A[q * n + q] - A[p * n + p]) / (2 * apq);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1));
        const double c = 1 / sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < n; ++k) {  // A <- A J
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {  // A <- J^T A
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
}

// one wave: lanes sum the block partials in block order, lane 0 solves
__global__ __launch_bounds__(64) void k_refit_solve(const double* __restrict__ partials, uint32_t blocks,
                                                    FmHdr* __restrict__ h, float* __restrict__ refitF) {
  __shared__ double sS[45];
  const int lane = threadIdx.x;
  if (lane < 45) {
    double s = 0;
    for (uint32_t b = 0; b < blocks; ++b) s += partials[45 * (size_t)b + lane];
    sS[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  for (int i = 0; i < 9; ++i) refitF[i] = 0.0f;
  if ((h->best >> 32) == 0) return;
  double A[81], V[81];
  int e = 0;
  for (int r = 0; r < 9; ++r)
    for (int c = r; c < 9; ++c) A[r * 9 + c] = A[c * 9 + r] = sS[e++];
  jacobi_eig(A, V, 9);
  int lo = 0;
  for (int i = 1; i < 9; ++i)
    if (A[i * 9 + i] < A[lo * 9 + lo]) lo = i;
  double F[9];
  for (int i = 0; i < 9; ++i) F[i] = V[i * 9 + lo];
  // rank 2: F <- F (I - v v^T), v the right singular vector of the smallest singular value (eigenvector of F^T F)
  double B[9], W[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) B[r * 3 + c] = F[r] * F[c] + F[3 + r] * F[3 + c] + F[6 + r] * F[6 + c];
  jacobi_eig(B, W, 3);
  int l3 = 0;
  for (int i = 1; i < 3; ++i)
    if (B[i * 3 + i] < B[l3 * 3 + l3]) l3 = i;
  const double v[3] = {W[0 * 3 + l3], W[1 * 3 + l3], W[2 * 3 + l3]};
  for (int r = 0; r < 3; ++r) {
    const double fv = F[3 * r] * v[0] + F[3 * r + 1] * v[1] + F[3 * r + 2] * v[2];
    for (int c = 0; c < 3; ++c) F[3 * r + c] -= fv * v[c];
  }
  denormalise_f(F, h, refitF);
}

__global__ void k_finalize(const float* __restrict__ cand, const float* __restrict__ refitF, const FmHdr* __restrict__ h,
                           float* __restrict__ F_out, uint32_t* __restrict__ count_out) {
  const uint32_t bestCount = (uint32_t)(h->best >> 32);
  const float* src = nullptr;
  uint32_t cnt = 0;
  if (bestCount > 0) {
    const bool refit = h->refitCount >= bestCount;
    src = refit ? refitF : best_f(cand, h);
    cnt = refit ? h->refitCount : bestCount;
  }
  for (int i = 0; i < 9; ++i) F_out[i] = src ? src[i] : 0.0f;
  *count_out = cnt;
}

// ---------------------------------------------------------------------------------------------- cheirality
struct CheiralArgs {
  float R[4][9];  // pose rotation (target ray -> query frame), row-major
  float C[4][3];  // target centre in the query frame
  float qd[2], qc[2], qf, td[2], tc[2], tf;  // ray model of each camera: (dpix.x (x - size.x / 2), ..., foc)
};

__global__ __launch_bounds__(256) void k_cheirality(const ssrlcv_match* __restrict__ m, uint32_t n,
                                                    const uint8_t* __restrict__ mask, CheiralArgs a,
                                                    uint32_t* __restrict__ votes) {
  uint32_t mine[4] = {0, 0, 0, 0};
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    bool use = i < n && !m[i].invalid && (!mask || mask[i]);
    float d1[3] = {0, 0, 0}, tr[3] = {0, 0, 0};
    if (use) {
      const ssrlcv_float2 q = m[i].keyPoints[0].loc, t = m[i].keyPoints[1].loc;
      d1[0] = a.qd[0] * (q.x - a.qc[0]);
      d1[1] = a.qd[1] * (q.y - a.qc[1]);
      d1[2] = a.qf;
      tr[0] = a.td[0] * (t.x - a.tc[0]);
      tr[1] = a.td[1] * (t.y - a.tc[1]);
      tr[2] = a.tf;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float d2[3];
      for (int r = 0; r < 3; ++r) d2[r] = a.R[c][3 * r] * tr[0] + a.R[c][3 * r + 1] * tr[1] + a.R[c][3 * r + 2] * tr[2];
      // least squares lq d1 - lt d2 = C
      const float aa = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
      const float bb = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
      const float cc = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
      const float ee = d1[0] * a.C[c][0] + d1[1] * a.C[c][1] + d1[2] * a.C[c][2];
      const float ff = d2[0] * a.C[c][0] + d2[1] * a.C[c][1] + d2[2] * a.C[c][2];
      const float det = bb * bb - aa * cc;
      const float lq = (bb * ff - cc * ee) / det, lt = (aa * ff - bb * ee) / det;
      const bool front = use && det != 0 && lq > 0 && lt > 0;
      mine[c] += (uint32_t)__popcll(__ballot(front));
    }
  }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 4; ++c)
      if (mine[c]) atomicAdd(votes + c, mine[c]);
}

// ---------------------------------------------------------------------------------------------- host 3x3 helpers
void host_jacobi3(double (&A)[3][3], double (&V)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j;
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    if (off <= 1e-30 * (A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2]) || off == 0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0) continue;
        const double th = (A[q][q] - A[p][p]) / (2 * A[p][q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}
void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
void unit3(double* a) {
  const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  if (l > 0)
    for (int i = 0; i < 3; ++i) a[i] /= l;
}

}  // namespace

extern "C" {

size_t ssrlcv_hip_fmatrix_ransac_workspace_bytes(uint32_t numMatches, uint32_t numSamples) {
  return ransac_layout(numMatches, numSamples).total;
}

int ssrlcv_hip_fmatrix_score(const ssrlcv_match* matches, uint32_t numMatches, const float* F, uint32_t k, float threshold,
                             void* workspace, size_t workspaceBytes, uint32_t* counts_out, uint8_t* inlierMask_out,
                             ssrlcv_stream_t stream) {
  if (!matches || !F || !counts_out || !workspace || k == 0 || !(threshold > 0) || !std::isfinite(threshold) ||
      (inlierMask_out && k != 1))
    return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < kHdrBytes) return SSRLCV_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  FmHdr* h = (FmHdr*)workspace;
  SSRLCV_HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)k * sizeof(uint32_t), st));
  if (numMatches == 0) return SSRLCV_OK;
  SSRLCV_HIP_TRY(hipMemsetAsync(h, 0, kHdrBytes, st));
  hipLaunchKernelGGL(k_bbox, dim3(refit_blocks(numMatches)), dim3(256), 0, st, matches, numMatches, h);
  hipLaunchKernelGGL(k_norm, dim3(1), dim3(1), 0, st, h);
  SSRLCV_LAUNCH_CHECK();
  return launch_score(matches, numMatches, F, k, threshold, h, counts_out, inlierMask_out, st);
}

int ssrlcv_hip_fmatrix_ransac(const ssrlcv_match* matches, uint32_t numMatches, uint32_t numSamples, float threshold,
                              uint64_t seed, void* workspace, size_t workspaceBytes, float* F_out,
                              uint32_t* inlierCount_out, uint8_t* inlierMask_out, float* candidates_out,
                              uint32_t* counts_out, ssrlcv_stream_t stream) {
  if (!matches || !F_out || !inlierCount_out || !workspace || numSamples == 0 || !(threshold > 0) ||
      !std::isfinite(threshold) || numSamples > (1u << 26))
    return SSRLCV_ERR_INVALID_ARG;
  const RansacLayout L = ransac_layout(numMatches, numSamples);
  if (workspaceBytes < L.total) return SSRLCV_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  FmHdr* h = (FmHdr*)ws;
  float* cand = (float*)(ws + L.cand);
  uint32_t* counts = (uint32_t*)(ws + L.counts);
  float* refitF = (float*)(ws + L.refitF);
  double* partials = (double*)(ws + L.partials);
  const uint32_t K = 3 * numSamples;
  if (numMatches < 7) {  // no sample can be drawn: empty result, stream-ordered like the full path
    SSRLCV_HIP_TRY(hipMemsetAsync(F_out, 0, 9 * sizeof(float), st));
    SSRLCV_HIP_TRY(hipMemsetAsync(inlierCount_out, 0, sizeof(uint32_t), st));
    if (inlierMask_out && numMatches) SSRLCV_HIP_TRY(hipMemsetAsync(inlierMask_out, 0, numMatches, st));
    if (candidates_out) SSRLCV_HIP_TRY(hipMemsetAsync(candidates_out, 0, (size_t)9 * K * sizeof(float), st));
    if (counts_out) SSRLCV_HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)K * sizeof(uint32_t), st));
    return SSRLCV_OK;
  }
  SSRLCV_HIP_TRY(hipMemsetAsync(h, 0, kHdrBytes, st));
  SSRLCV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)K * sizeof(uint32_t), st));
  const uint32_t rb = refit_blocks(numMatches);
  hipLaunchKernelGGL(k_bbox, dim3(rb), dim3(256), 0, st, matches, numMatches, h);
  hipLaunchKernelGGL(k_norm, dim3(1), dim3(1), 0, st, h);
  hipLaunchKernelGGL(k_sample_solve, dim3((numSamples + 63) / 64), dim3(64), 0, st, matches, numMatches, numSamples, seed,
                     h, cand);
  SSRLCV_LAUNCH_CHECK();
  int rc = launch_score(matches, numMatches, cand, K, threshold, h, counts, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_best, dim3((K + 255) / 256), dim3(256), 0, st, counts, K, h);
  hipLaunchKernelGGL(k_refit_accum, dim3(rb), dim3(256), 0, st, matches, numMatches, cand, threshold, h, partials);
  hipLaunchKernelGGL(k_refit_solve, dim3(1), dim3(64), 0, st, partials, rb, h, refitF);
  SSRLCV_LAUNCH_CHECK();
  rc = launch_score(matches, numMatches, refitF, 1, threshold, h, &h->refitCount, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1), 0, st, cand, refitF, h, F_out, inlierCount_out);
  SSRLCV_LAUNCH_CHECK();
  if (inlierMask_out) {
    rc = launch_score(matches, numMatches, F_out, 1, threshold, h, &h->maskCount, inlierMask_out, st);
    if (rc) return rc;
  }
  if (candidates_out)
    SSRLCV_HIP_TRY(hipMemcpyAsync(candidates_out, cand, (size_t)9 * K * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (counts_out)
    SSRLCV_HIP_TRY(hipMemcpyAsync(counts_out, counts, (size_t)K * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

int ssrlcv_hip_pose_from_fmatrix(const ssrlcv_match* matches, uint32_t numMatches, const uint8_t* inlierMask,
                                 const float* F, const ssrlcv_camera* query_host, const ssrlcv_camera* target_host,
                                 void* workspace, size_t workspaceBytes, ssrlcv_pose* pose_host, ssrlcv_stream_t stream) {
  const ssrlcv_camera *query = query_host, *target = target_host;
  ssrlcv_pose* pose = pose_host;
  if (!matches || !F || !query || !target || !workspace || !pose) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < kHdrBytes) return SSRLCV_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float Fh[9];
  SSRLCV_HIP_TRY(hipMemcpyAsync(Fh, F, sizeof Fh, hipMemcpyDeviceToHost, st));
  SSRLCV_HIP_TRY(hipStreamSynchronize(st));
  // E = K_t^T F K_q with K = [[foc / dpix.x, 0, size.x / 2], [0, foc / dpix.y, size.y / 2], [0, 0, 1]]
  const ssrlcv_camera* cams[2] = {query, target};
  double Kc[2][3][3] = {};
  for (int c = 0; c < 2; ++c) {
    Kc[c][0][0] = (double)cams[c]->foc / cams[c]->dpix.x;
    Kc[c][1][1] = (double)cams[c]->foc / cams[c]->dpix.y;
    Kc[c][0][2] = cams[c]->size.x / 2.0;
    Kc[c][1][2] = cams[c]->size.y / 2.0;
    Kc[c][2][2] = 1;
  }
  double FK[3][3], E[3][3], nrm = 0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      FK[r][c] = 0;
      for (int k = 0; k < 3; ++k) FK[r][c] += (double)Fh[3 * r + k] * Kc[0][k][c];
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      E[r][c] = 0;
      for (int k = 0; k < 3; ++k) E[r][c] += Kc[1][k][r] * FK[k][c];
      nrm += E[r][c] * E[r][c];
    }
  if (!(nrm > 0) || !std::isfinite(nrm)) return SSRLCV_ERR_INVALID_ARG;
  // SVD through the eigenvectors of E^T E: V (columns by descending eigenvalue, det +1), u_i = E v_i / |E v_i|,
  // u3 = u1 x u2; singular values projected to (1, 1, 0)
  double S[3][3], W[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[r][c] = E[0][r] * E[0][c] + E[1][r] * E[1][c] + E[2][r] * E[2][c];
  host_jacobi3(S, W);
  int ord[3] = {0, 1, 2};
  for (int i = 1; i < 3; ++i)
    for (int j = i; j > 0 && S[ord[j]][ord[j]] > S[ord[j - 1]][ord[j - 1]]; --j) {
      const int t = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = t;
    }
  double v[3][3], u[3][3];  // v[i], u[i]: the i-th singular vectors
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) v[i][k] = W[k][ord[i]];
  cross3(v[0], v[1], v[2]);
  for (int i = 0; i < 2; ++i) {
    for (int r = 0; r < 3; ++r) u[i][r] = E[r][0] * v[i][0] + E[r][1] * v[i][1] + E[r][2] * v[i][2];
    unit3(u[i]);
  }
  cross3(u[0], u[1], u[2]);
  // R = U W V^T or U W^T V^T with W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; t = +-u3.  x_t = R x_q + t; the pose is the
  // inverse: rotation R^T, target centre C = -R^T t.
  CheiralArgs a;
  for (int cnd = 0; cnd < 4; ++cnd) {
    const double sw = cnd < 2 ? 1.0 : -1.0, st3 = (cnd & 1) ? -1.0 : 1.0;
    double R[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)  // U W V^T = u1 (w-th) ... : column 0 of U W = sw u2, column 1 = -sw u1, column 2 = u3
        R[r][c] = sw * u[1][r] * v[0][c] - sw * u[0][r] * v[1][c] + u[2][r] * v[2][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) a.R[cnd][3 * r + c] = (float)R[c][r];
    for (int r = 0; r < 3; ++r) a.C[cnd][r] = (float)(-st3 * (R[0][r] * u[2][0] + R[1][r] * u[2][1] + R[2][r] * u[2][2]));
  }
  a.qd[0] = query->dpix.x, a.qd[1] = query->dpix.y, a.qc[0] = query->size.x / 2.0f, a.qc[1] = query->size.y / 2.0f;
  a.qf = query->foc;
  a.td[0] = target->dpix.x, a.td[1] = target->dpix.y, a.tc[0] = target->size.x / 2.0f, a.tc[1] = target->size.y / 2.0f;
  a.tf = target->foc;
  FmHdr* h = (FmHdr*)workspace;
  SSRLCV_HIP_TRY(hipMemsetAsync(h->votes, 0, sizeof h->votes, st));
  if (numMatches)
    hipLaunchKernelGGL(k_cheirality, dim3(refit_blocks(numMatches)), dim3(256), 0, st, matches, numMatches, inlierMask, a,
                       h->votes);
  SSRLCV_LAUNCH_CHECK();
  uint32_t votes[4];
  SSRLCV_HIP_TRY(hipMemcpyAsync(votes, h->votes, sizeof votes, hipMemcpyDeviceToHost, st));
  SSRLCV_HIP_TRY(hipStreamSynchronize(st));
  int best = 0;
  for (int c = 1; c < 4; ++c)
    if (votes[c] > votes[best]) best = c;
  const float* Rp = a.R[best];  // getAxisRotations (matrix_util.hpp), float like stage::relativePose
  const float rx = atan2f(Rp[7], Rp[8]);
  pose->roll = rx;
  pose->pitch = atan2f(-Rp[6], Rp[8] / cosf(rx));
  pose->yaw = atan2f(Rp[3], Rp[0]);
  double C[3] = {a.C[best][0], a.C[best][1], a.C[best][2]};
  unit3(C);
  const double dx = (double)target->cam_pos.x - query->cam_pos.x, dy = (double)target->cam_pos.y - query->cam_pos.y,
               dz = (double)target->cam_pos.z - query->cam_pos.z;
  const double scale = std::sqrt(dx * dx + dy * dy + dz * dz) / 1000.0;
  pose->x = (float)(C[0] * scale);
  pose->y = (float)(C[1] * scale);
  pose->z = (float)(C[2] * scale);
  return SSRLCV_OK;
}

}  // extern "C"
