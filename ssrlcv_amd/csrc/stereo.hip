// ssrlcv_amd/csrc/stereo.hip -- dense stereo for gfx950: SAD block matching of a rectified u8 pair (the reference's
// Window_NxN descriptors + disparity matchers, worked from the two images directly), its Match records and
// PointCloudFactory::stereo_disparity.  The contract is include/ssrlcv_hip.h "dense stereo"; tests/stereo_ref.py restates it.
//
//   k_stereo_fill    every pixel of both maps invalid (the border and the pixels without a candidate stay that way)
//   k_stereo_sad     the cost pass.  A block owns a strip of TX columns and marches down TY rows of it.  A lane owns FOUR
//                    neighbouring columns and EIGHT neighbouring disparities: 32 running window sums in registers.  No cost
//                    volume and no per-pixel window exists anywhere: the window sum is separable,
//                      h(x, y, d) = sum over the 2r + 1 columns of |B(x + i, y) - O(x + i -/+ d, y)|      (v_sad_u8, 4 bytes each)
//                      V(x, y, d) = V(x, y - 1, d) + h(x, y + r, d) - h(x, y - r - 1, d)
//                    and the leaving row's h is recomputed from a ring of 2r + 3 staged rows of both images in LDS (a ring
//                    of the h themselves would be 2r + 1 times the register state).  Work per (pixel, disparity) and row is
//                    2 ceil((2r + 1) / 4) SADs whatever the window's height.  The rows are staged with the strip's first
//                    window column on a dword boundary, so every unaligned dword a lane needs is v_alignbyte_b32 of two
//                    aligned ones at a compile-time shift; the window's last, partial dword is masked on both sides.
//                    The winner of a pixel is one min over keys (cost << 8 | k): least cost, smallest disparity on ties;
//                    the eight-disparity groups of a pixel sit in neighbouring lanes and meet through a shuffle butterfly;
//                    the lane that owns the winner has its two neighbours' costs (its own registers, or one shuffle from
//                    the next group) and writes the pixel: cost limit, sub-pixel offset, disparity, cost, k.
//                    RIGHT = true is the same pass seen from the right image (partner at x + d): the right winners of the
//                    left-right check, as a second pass (it runs only when the check is asked for).
//   k_stereo_lr      the left-right check over the two k maps
//   StereoKeep / StereoEmit + compact.h   the valid pixels of the sampling grid as Match records, in raster order
//   k_stereo_points  upstream's stereo_disparity
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "compact.h"
#include "device_math.h"

namespace {

constexpr int kXs = 4;                      // columns per lane
constexpr int kDc = 8;                      // disparities per lane
constexpr int kMaxG = 8;                    // dwords of the widest window row (31 bytes)
constexpr int kPre = 10;                    // staged bytes per thread and row, at most
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kMatchPerThread = 16;

struct StereoArgs {
  int w, h, r, G;          // G dwords cover the 2r + 1 window bytes; the last one holds `rem` of them
  uint32_t remMask;
  int D, dmin;
  int nD, nDlog;           // lanes per pixel group (a power of two): nD * 8 >= D
  int TX, TY, tilesX;
  int pitchB, pitchO, ring;
  int threads;
  uint32_t maxCost;
  int subpixel;
};

// horizontal sums of one staged row: acc[xi][dk] += sum over the window of |B - O|
template <bool RIGHT>
__device__ __forceinline__ void row_sums(const uint8_t* __restrict__ rowB, const uint8_t* __restrict__ rowO, int G, uint32_t remMask,
                                         uint32_t (&acc)[kXs][kDc]) {
  const uint32_t* pB = reinterpret_cast<const uint32_t*>(rowB);
  const uint32_t* pO = reinterpret_cast<const uint32_t*>(rowO);
  uint32_t A[kMaxG + 1], O[kMaxG + 3];
#pragma unroll
  for (int j = 0; j <= kMaxG; ++j) A[j] = j <= G ? pB[j] : 0u;
#pragma unroll
  for (int j = 0; j <= kMaxG + 2; ++j) O[j] = j <= G + 2 ? pO[j] : 0u;
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) {
    if (g < G) {  // wave-uniform
      const uint32_t m = g == G - 1 ? remMask : 0xFFFFFFFFu;
      uint32_t L[kXs], U[kXs + kDc - 1];
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi) L[xi] = (xi == 0 ? A[g] : __builtin_amdgcn_alignbyte(A[g + 1], A[g], (uint32_t)xi)) & m;
#pragma unroll
      for (int o = 0; o < kXs + kDc - 1; ++o)
        U[o] = ((o & 3) == 0 ? O[g + (o >> 2)] : __builtin_amdgcn_alignbyte(O[g + (o >> 2) + 1], O[g + (o >> 2)], (uint32_t)(o & 3))) & m;
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) acc[xi][dk] = __builtin_amdgcn_sad_u8(L[xi], U[xi + (RIGHT ? dk : kDc - 1 - dk)], acc[xi][dk]);
    }
  }
}

__global__ __launch_bounds__(256) void k_stereo_fill(float* __restrict__ disparity, uint32_t* __restrict__ cost, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    disparity[i] = __uint_as_float(kNaN);
    if (cost) cost[i] = 0xFFFFFFFFu;
  }
}

// RIGHT = false: base = left image, other = right, partner of (x, d) at x - d; writes disparity, cost and kwin.
// RIGHT = true:  base = right image, other = left, partner at x + d; writes kwin alone.
template <bool RIGHT>
__global__ __launch_bounds__(256) void k_stereo_sad(const uint8_t* __restrict__ base, const uint8_t* __restrict__ other, StereoArgs a,
                                                    float* __restrict__ disparity, uint32_t* __restrict__ cost, uint8_t* __restrict__ kwin) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* sB = smem;                                   // [ring][pitchB]
  uint8_t* sO = smem + (size_t)a.ring * a.pitchB;       // [ring][pitchO]
  const int tid = threadIdx.x;
  const int dl = tid & (a.nD - 1), xl = tid >> a.nDlog;
  const int tx = blockIdx.x % a.tilesX, ty = blockIdx.x / a.tilesX;
  const int X0 = a.r + tx * a.TX;
  const int Y0 = a.r + ty * a.TY;
  const int Y1 = min(Y0 + a.TY, a.h - a.r);
  const int Dtile = a.nD * kDc;
  // global column of staged byte 0 of either image
  const int cb0 = X0 - a.r;
  const int co0 = RIGHT ? X0 - a.r + a.dmin : X0 - a.r - (a.dmin + Dtile - 1);
  const int offB = kXs * xl;
  const int offO = kXs * xl + kDc * (RIGHT ? dl : a.nD - 1 - dl);
  const int nb = a.pitchB + a.pitchO;

  // which of this lane's (column, disparity) pairs are candidates: the same for every row
  uint32_t valid[kXs];
#pragma unroll
  for (int xi = 0; xi < kXs; ++xi) {
    const int x = X0 + offB + xi;
    uint32_t bits = 0;
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) {
      const int k = dl * kDc + dk, d = a.dmin + k;
      const int partner = RIGHT ? x + d : x - d;
      if (x <= a.w - 1 - a.r && k < a.D && partner >= a.r && partner <= a.w - 1 - a.r) bits |= 1u << dk;
    }
    valid[xi] = bits;
  }

  uint32_t V[kXs][kDc];
#pragma unroll
  for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) V[xi][dk] = 0;

  uint8_t pre[kPre];
  auto fetch = [&](int row) {
    const size_t rowAt = (size_t)row * a.w;
#pragma unroll
    for (int q = 0; q < kPre; ++q) {
      const int i = tid + q * a.threads;
      uint8_t v = 0;
      if (i < nb) {
        const bool inB = i < a.pitchB;
        const int col = inB ? cb0 + i : co0 + (i - a.pitchB);
        if (col >= 0 && col < a.w) v = (inB ? base : other)[rowAt + col];
      }
      pre[q] = v;
    }
  };

  const int T0 = Y0 - a.r, T1 = Y1 - 1 + a.r;  // rows this block reads: all inside the image
  fetch(T0);
  for (int t = T0; t <= T1; ++t) {
    {
      const int slot = t % a.ring;
#pragma unroll
      for (int q = 0; q < kPre; ++q) {
        const int i = tid + q * a.threads;
        if (i < nb) {
          if (i < a.pitchB) sB[slot * a.pitchB + i] = pre[q];
          else sO[slot * a.pitchO + (i - a.pitchB)] = pre[q];
        }
      }
    }
    __syncthreads();  // row t is staged; the slot it took was last read two iterations ago (ring = 2r + 3)
    if (t < T1) fetch(t + 1);

    {
      const int slot = t % a.ring;
      uint32_t acc[kXs][kDc];
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) acc[xi][dk] = V[xi][dk];
      row_sums<RIGHT>(sB + slot * a.pitchB + offB, sO + slot * a.pitchO + offO, a.G, a.remMask, acc);
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) V[xi][dk] = acc[xi][dk];
    }
    const int leaving = t - 2 * a.r - 1;
    if (leaving >= T0) {  // block-uniform
      const int slot = leaving % a.ring;
      uint32_t acc[kXs][kDc];
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) acc[xi][dk] = 0;
      row_sums<RIGHT>(sB + slot * a.pitchB + offB, sO + slot * a.pitchO + offO, a.G, a.remMask, acc);
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) V[xi][dk] -= acc[xi][dk];
    }
    const int y = t - a.r;
    if (y < Y0) continue;  // block-uniform: the window is not full yet

#pragma unroll
    for (int xi = 0; xi < kXs; ++xi) {
      uint32_t best = kNoKey;
#pragma unroll
      for (int dk = 0; dk < kDc; ++dk) {
        const uint32_t key = (V[xi][dk] << 8) | (uint32_t)(dl * kDc + dk);
        best = min(best, (valid[xi] >> dk) & 1u ? key : kNoKey);
      }
      for (int s = 1; s < a.nD; s <<= 1) best = min(best, (uint32_t)__shfl_xor((int)best, s, 64));
      // the edge costs of the neighbouring groups, for a winner at either end of a group
      const uint32_t fromBelow = (uint32_t)__shfl_up((int)V[xi][kDc - 1], 1, 64);
      const uint32_t fromAbove = (uint32_t)__shfl_down((int)V[xi][0], 1, 64);
      const int k = (int)(best & 0xFFu);
      if (best != kNoKey && (k >> 3) == dl) {
        const int x = X0 + offB + xi;
        const size_t p = (size_t)y * a.w + x;
        kwin[p] = (uint8_t)k;
        if (!RIGHT) {
          const uint32_t c = best >> 8;
          if (c <= a.maxCost) {
            const int d = a.dmin + k;
            float disp = (float)d;
            if (a.subpixel) {
              const int partner = x - d, lo = a.r, hi = a.w - 1 - a.r;
              const bool hasM = k >= 1 && partner + 1 >= lo && partner + 1 <= hi;
              const bool hasP = k + 1 < a.D && partner - 1 >= lo && partner - 1 <= hi;
              if (hasM && hasP) {
                const int idx = k & 7;
                uint32_t cm = fromBelow, cp = fromAbove;
#pragma unroll
                for (int dk = 0; dk < kDc; ++dk) {
                  if (idx == dk + 1) cm = V[xi][dk];
                  if (idx + 1 == dk) cp = V[xi][dk];
                }
                const int den = (int)cm - 2 * (int)c + (int)cp;
                if (den != 0) disp = (float)d + __fdiv_rn((float)((int)cm - (int)cp), (float)(2 * den));
              }
            }
            disparity[p] = disp;
            if (cost) cost[p] = c;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_stereo_lr(float* __restrict__ disparity, uint32_t* __restrict__ cost, const uint8_t* __restrict__ kL,
                                                   const uint8_t* __restrict__ kR, int w, size_t n, int dmin, int tol) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
    if (__float_as_uint(disparity[p]) == kNaN) continue;
    const int k = kL[p];
    const int kr = kR[(size_t)((long long)p - (dmin + k))];  // same row, column x - d*: inside the row, d* being a candidate
    int diff = kr - k;
    if (diff < 0) diff = -diff;
    if (diff > tol) {
      disparity[p] = __uint_as_float(kNaN);
      if (cost) cost[p] = 0xFFFFFFFFu;
    }
  }
}

// ---- Match records of the valid pixels of the sampling grid (compact.h)
struct StereoKeep {
  const float* disparity;
  uint32_t w, step, nxs;
  __device__ uint32_t operator()(uint32_t i) const {
    const uint32_t ys = i / nxs, xs = i - ys * nxs;
    const size_t p = (size_t)((unsigned long long)ys * step) * w + (size_t)((unsigned long long)xs * step);
    return __float_as_uint(disparity[p]) != kNaN ? 1u : 0u;
  }
};
struct StereoEmit {
  const float* disparity;
  uint32_t w, step, nxs;
  int leftId, rightId;
  ssrlcv_match* out;
  uint32_t capacity;
  __device__ void operator()(uint32_t i, int, uint32_t dst) const {
    if (dst >= capacity) return;
    const uint32_t ys = i / nxs, xs = i - ys * nxs;
    const uint32_t x = xs * step, y = ys * step;  // below w, h
    const float d = disparity[(size_t)y * w + x];
    uint32_t* rec = reinterpret_cast<uint32_t*>(out + dst);  // 40 bytes, padding written as zero
    rec[0] = 0u;  // invalid = 0
    rec[1] = 0u;
    rec[2] = (uint32_t)leftId;
    rec[3] = 0u;
    rec[4] = __float_as_uint((float)x);
    rec[5] = __float_as_uint((float)y);
    rec[6] = (uint32_t)rightId;
    rec[7] = 0u;
    rec[8] = __float_as_uint((float)x - d);
    rec[9] = __float_as_uint((float)y);
  }
};

__global__ __launch_bounds__(256) void k_stereo_points(const ssrlcv_match* __restrict__ matches, uint32_t n, float foc, float baseline, float doffset,
                                                       float cx, float cy, ssrlcv_float3* __restrict__ points) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const ssrlcv_match m = matches[i];
  float X = 0.0f, Y = 0.0f, Z = 0.0f;
  const float s = (m.keyPoints[0].loc.x - m.keyPoints[1].loc.x) + doffset;
  if (m.invalid == 0 && s > 0.0f) {
    Z = __fdiv_rn(foc * baseline, s);
    X = __fdiv_rn((m.keyPoints[0].loc.x - cx) * Z, foc);
    Y = __fdiv_rn((m.keyPoints[0].loc.y - cy) * Z, foc);
  }
  points[i].x = X;
  points[i].y = Y;
  points[i].z = Z;
}

// ---- host side
int stereo_params_status(uint32_t w, uint32_t h, const ssrlcv_stereo_params* p) {
  if (!p) return SSRLCV_ERR_INVALID_ARG;
  if (p->radius == 0 || p->numDisparities == 0 || p->minDisparity < -32768 || p->minDisparity > 32767 || p->subpixel > 1)
    return SSRLCV_ERR_INVALID_ARG;
  if ((unsigned long long)w * h >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  if (p->radius > 15 || p->numDisparities > 256) return SSRLCV_ERR_UNSUPPORTED;
  return SSRLCV_OK;
}

// samples 0, step, 2 step, ... below n: ceil(n / step) without the sum n + step - 1, which wraps for a step near 2^32
uint32_t stereo_grid(uint32_t n, uint32_t step) { return n ? (n - 1) / step + 1 : 0; }

size_t stereo_map_bytes(uint32_t w, uint32_t h) { return align256((size_t)w * h); }

StereoArgs stereo_args(uint32_t w, uint32_t h, const ssrlcv_stereo_params* p) {
  StereoArgs a;
  a.w = (int)w;
  a.h = (int)h;
  a.r = (int)p->radius;
  const int W = 2 * a.r + 1;
  a.G = (W + 3) / 4;
  a.remMask = W - 4 * (a.G - 1) == 1 ? 0xFFu : 0xFFFFFFu;  // W is odd: 1 or 3 bytes in the last dword
  a.D = (int)p->numDisparities;
  a.dmin = p->minDisparity;
  a.nDlog = 0;
  while ((kDc << a.nDlog) < a.D) ++a.nDlog;
  a.nD = 1 << a.nDlog;                                     // 1 .. 32
  const int NX = a.nD >= 4 ? 256 / a.nD : 64;              // column groups per block: at most a wave's worth
  a.threads = NX * a.nD;                                   // 64, 128 or 256
  a.TX = kXs * NX;
  a.pitchB = a.TX + 4 * kMaxG + 8;
  a.pitchO = a.TX + a.nD * kDc + 4 * kMaxG + 8;
  a.ring = 2 * a.r + 3;
  const int wi = a.w - 2 * a.r, hi = a.h - 2 * a.r;        // the interior; both >= 1 here
  a.tilesX = (wi + a.TX - 1) / a.TX;
  // rows per block: enough blocks to fill the chip, but the 2r rows a block spends filling its first window stay a
  // small share of its march
  int segs = (1024 + a.tilesX - 1) / a.tilesX;
  const int minRows = 8 * a.r + 8;
  if (segs > (hi + minRows - 1) / minRows) segs = (hi + minRows - 1) / minRows;
  if (segs < 1) segs = 1;
  a.TY = (hi + segs - 1) / segs;
  a.maxCost = p->maxCost;
  a.subpixel = (int)p->subpixel;
  return a;
}

}  // namespace

extern "C" {

size_t ssrlcv_hip_stereo_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_stereo_params* params) {
  if (stereo_params_status(w, h, params)) return 0;
  return 2 * stereo_map_bytes(w, h) + 256;  // the winners' k of both views, one byte per pixel each
}

int ssrlcv_hip_stereo_sad_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params* params,
                             void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, ssrlcv_stream_t stream) {
  const int rc = stereo_params_status(w, h, params);  // the parameters first: their codes do not depend on the buffers
  if (rc) return rc;
  if (!left || !right || !workspace || !disparity) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_stereo_workspace_bytes(w, h, params)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)w * h;
  if (n == 0) return SSRLCV_OK;
  unsigned fillBlocks = (unsigned)((n + 255) / 256);
  if (fillBlocks > 2048u) fillBlocks = 2048u;
  hipLaunchKernelGGL(k_stereo_fill, dim3(fillBlocks), dim3(256), 0, st, disparity, cost, n);
  const uint32_t side = 2 * params->radius + 1;
  if (w >= side && h >= side) {  // else: no pixel has a window
    const StereoArgs a = stereo_args(w, h, params);
    uint8_t* kL = (uint8_t*)workspace;
    uint8_t* kR = kL + stereo_map_bytes(w, h);
    const int tilesY = ((int)h - 2 * a.r + a.TY - 1) / a.TY;
    const size_t lds = (size_t)a.ring * (a.pitchB + a.pitchO);
    const dim3 grid((unsigned)(a.tilesX * tilesY));
    hipLaunchKernelGGL(k_stereo_sad<false>, grid, dim3(a.threads), lds, st, left, right, a, disparity, cost, kL);
    if (params->lrTolerance >= 0) {
      hipLaunchKernelGGL(k_stereo_sad<true>, grid, dim3(a.threads), lds, st, right, left, a, (float*)nullptr, (uint32_t*)nullptr, kR);
      hipLaunchKernelGGL(k_stereo_lr, dim3(fillBlocks), dim3(256), 0, st, disparity, cost, kL, kR, (int)w, n, a.dmin, params->lrTolerance);
    }
  }
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_stereo_matches_workspace_bytes(uint32_t w, uint32_t h, uint32_t step) {
  if (step == 0 || (unsigned long long)w * h >= (1ull << 31)) return 0;
  const uint32_t nxs = stereo_grid(w, step), nys = stereo_grid(h, step);
  return align256(svc::workspace_words<1, kMatchPerThread>(nxs * nys) * 4);
}

int ssrlcv_hip_stereo_matches(const float* disparity, uint32_t w, uint32_t h, uint32_t step, int leftId, int rightId, ssrlcv_match* out,
                              uint32_t capacity, uint32_t* count_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream) {
  if (step == 0 || (unsigned long long)w * h >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  if (!disparity || !count_dev || !workspace || (!out && capacity != 0)) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < ssrlcv_hip_stereo_matches_workspace_bytes(w, h, step)) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t nxs = stereo_grid(w, step), nys = stereo_grid(h, step);
  StereoKeep keep{disparity, w, step, nxs};
  StereoEmit emit{disparity, w, step, nxs, leftId, rightId, out, capacity};
  uint32_t* totals = nullptr;
  SSRLCV_HIP_TRY((svc::partition<1, kMatchPerThread>(nxs * nys, keep, emit, (uint32_t*)workspace, &totals, st)));
  SSRLCV_HIP_TRY(hipMemcpyAsync(count_dev, totals + 1, 4, hipMemcpyDeviceToDevice, st));
  return SSRLCV_OK;
}

int ssrlcv_hip_stereo_points(const ssrlcv_match* matches, uint32_t n, float foc, float baseline, float doffset, float cx, float cy,
                             ssrlcv_float3* points, ssrlcv_stream_t stream) {
  if (!(fabsf(foc) <= 3.4028234663852886e38f) || foc == 0.0f) return SSRLCV_ERR_INVALID_ARG;
  if (n == 0) return SSRLCV_OK;
  if (!matches || !points) return SSRLCV_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_stereo_points, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, matches, n, foc, baseline, doffset, cx, cy,
                     points);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
