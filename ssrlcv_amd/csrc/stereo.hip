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
//                    The winner form takes the winner of every pixel (below) and writes it: cost limit, sub-pixel offset,
//                    disparity, cost, k.  RIGHT = true is the same pass seen from the right image (partner at x + d): the
//                    right winners of the left-right check, k alone, as a second pass (only when the check is asked for).
//                    VOLUME = true is the cost pass of semi-global matching: the same march and the same 32 running sums,
//                    but a lane stores its eight costs of a column, clamped (costClamp, also for a non-candidate), as eight
//                    uint16 in one 16-byte store (pack8) into the volume M[y][x][k].
//   the winner       of a pixel, for k_stereo_sad over its window sums and for k_sgm_winners over S, either view: winner_key is
//                    one min over keys (cost << 8 | k) of the candidates: least cost, smallest disparity on ties; the
//                    eight-disparity groups of a pixel sit in neighbouring lanes and meet through a shuffle butterfly.  The
//                    lane that owns the winner has the costs of k - 1 and k + 1 (its own registers, or edge_costs: one shuffle
//                    from the next group) and winner_disparity adds the sub-pixel offset of the parabola through the three.
//   k_census         the census cost (include/ssrlcv_hip.h "census cost"; tests/census_ref.py restates it): the code of every pixel
//                    of one view, a uint64 per pixel
//   k_stereo_census  the census sibling of k_stereo_sad: the same ownership, march and three forms over the Hamming distances of
//                    the codes summed over the aggregation window; cost_row_out is the end of a row of either cost pass
//   k_stereo_lr      the left-right check over the two k maps
//   k_sgm_path       semi-global matching (include/ssrlcv_hip.h "semi-global matching"; tests/sgm_ref.py restates it): one
//                    direction's pass.  A group of nD lanes -- 8 disparities a lane, the SAD kernel's ownership -- owns ONE
//                    path from its first pixel of the interior to its last: 64 / nD paths a wave, one wave a block, no block
//                    waits for another.  The state L(q, .) lives in 32-bit registers; a step takes L(q, k -/+ 1) of the group's
//                    edge disparities from the neighbouring lanes (one lane up, one down, the group's ends and k >= D
//                    holding a sentinel no minimum picks and no penalty wraps) and min over k of L(q, k) through the xor
//                    butterfly, both as DPP moves inside a row of 16 lanes (shuffles only for 32-lane groups).  The
//                    addresses of M and S along a path do not depend on the chain: the 16-byte loads of the next kSgmAhead
//                    steps are in flight in a register ring while a step is computed, and S, read ahead with M, is
//                    updated beside the chain (the first selected direction stores S, the others add).
//                    Every pixel of the interior lies on exactly one path of a pass; the passes are ordered on the stream.
//                    Diagonals are enumerated in coordinates flipped so that the direction is (+1, +1): wi paths start on
//                    the first row, hi - 1 on the first column below it.
//   k_sgm_winners    the left winner of every interior pixel from S over its candidates, both maps and kL; and, when the
//                    check is asked for, the right winners into kR for k_stereo_lr: S(x' + d, y, d) reaches right pixel x'
//                    through an LDS tile of the block's row strip, so S is read in whole 16-byte entries only
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
constexpr int kPreCodes = 10;               // staged census codes per thread and row, at most (census_tile)
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
  int ra;                  // census cost pass only: the aggregation radius; r is then the footprint's rho = ra + censusRadius
};

// a lane's eight uint16 of a pixel's entry of either volume, as one 16-byte word
__device__ __forceinline__ uint4 pack8(const uint32_t (&c)[kDc]) {
  return make_uint4(c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16));
}
__device__ __forceinline__ void unpack8(const uint4& v, uint32_t (&o)[kDc]) {
  o[0] = v.x & 0xFFFFu; o[1] = v.x >> 16;
  o[2] = v.y & 0xFFFFu; o[3] = v.y >> 16;
  o[4] = v.z & 0xFFFFu; o[5] = v.z >> 16;
  o[6] = v.w & 0xFFFFu; o[7] = v.w >> 16;
}

// ---- the winner of a pixel.  `c`: the eight costs of lane dl of the pixel's nD lanes (k = 8 dl .. 8 dl + 7); cand[dk]: whether
// k = 8 dl + dk is a candidate, eight bools or the bits of a mask.  Every lane of the group takes winner_key and edge_costs.
struct CandidateBits {
  uint32_t bits;
  __device__ __forceinline__ bool operator[](int dk) const { return (bits >> dk) & 1u; }
};
// the pixel's least key, the same in all its lanes; kNoKey without a candidate
template <class Cand>
__device__ __forceinline__ uint32_t winner_key(const uint32_t (&c)[kDc], const Cand& cand, int dl, int nD) {
  uint32_t best = kNoKey;
#pragma unroll
  for (int dk = 0; dk < kDc; ++dk) {
    const uint32_t key = (c[dk] << 8) | (uint32_t)(dl * kDc + dk);
    best = min(best, cand[dk] ? key : kNoKey);
  }
  for (int s = 1; s < nD; s <<= 1) best = min(best, (uint32_t)__shfl_xor((int)best, s, 64));
  return best;
}

// the edge costs of the neighbouring lanes, for a winner at either end of a lane's eight
struct EdgeCosts { uint32_t below, above; };
__device__ __forceinline__ EdgeCosts edge_costs(const uint32_t (&c)[kDc]) {
  return {(uint32_t)__shfl_up((int)c[kDc - 1], 1, 64), (uint32_t)__shfl_down((int)c[0], 1, 64)};
}

// the disparity of winner k of left pixel x, in the lane that owns it (Args: StereoArgs or SgmArgs)
template <class Args>
__device__ __forceinline__ float winner_disparity(const Args& a, const uint32_t (&c)[kDc], const EdgeCosts& edge, int k, uint32_t cost, int x) {
  const int d = a.dmin + k;
  float disp = (float)d;
  if (a.subpixel) {
    const int partner = x - d, lo = a.r, hi = a.w - 1 - a.r;
    const bool hasM = k >= 1 && partner + 1 >= lo && partner + 1 <= hi;
    const bool hasP = k + 1 < a.D && partner - 1 >= lo && partner - 1 <= hi;
    if (hasM && hasP) {
      const int idx = k & 7;
      uint32_t cm = edge.below, cp = edge.above;
#pragma unroll
      for (int dk = 0; dk < kDc; ++dk) {  // not c[idx -/+ 1]: no run-time register index
        if (idx == dk + 1) cm = c[dk];
        if (idx + 1 == dk) cp = c[dk];
      }
      const int den = (int)cm - 2 * (int)cost + (int)cp;
      if (den != 0) disp = (float)d + __fdiv_rn((float)((int)cm - (int)cp), (float)(2 * den));
    }
  }
  return disp;
}

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

// What a cost pass does with row y of its running sums V, for the lane's four columns x0 .. x0 + 3 and its eight disparities
// (valid[xi]: which of them are candidates).  The winner form takes the winner of every pixel and the lane that owns it writes
// k, and for the left view the disparity and the cost under the limit; VOLUME stores the eight costs, clamped, a non-candidate
// as the clamp itself.  The SAD and the census cost pass both end their row here.
template <bool RIGHT, bool VOLUME>
__device__ __forceinline__ void cost_row_out(const StereoArgs& a, const uint32_t (&V)[kXs][kDc], const uint32_t (&valid)[kXs], int dl, int x0, int y,
                                             float* __restrict__ disparity, uint32_t* __restrict__ cost, uint8_t* __restrict__ kwin,
                                             uint16_t* __restrict__ volume, uint32_t clamp) {
  if constexpr (VOLUME) {
    const int Dtile = a.nD * kDc;
#pragma unroll
    for (int xi = 0; xi < kXs; ++xi) {
      const int x = x0 + xi;
      if (x <= a.w - 1 - a.r) {
        uint32_t c[kDc];
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) c[dk] = (valid[xi] >> dk) & 1u ? min(V[xi][dk], clamp) : clamp;
        *reinterpret_cast<uint4*>(volume + ((size_t)y * a.w + x) * Dtile + dl * kDc) = pack8(c);
      }
    }
  } else {
#pragma unroll
    for (int xi = 0; xi < kXs; ++xi) {
      const uint32_t best = winner_key(V[xi], CandidateBits{valid[xi]}, dl, a.nD);
      const EdgeCosts edge = edge_costs(V[xi]);
      const int k = (int)(best & 0xFFu);
      if (best != kNoKey && (k >> 3) == dl) {  // the lane that owns the winner writes the pixel
        const int x = x0 + xi;
        const size_t p = (size_t)y * a.w + x;
        kwin[p] = (uint8_t)k;
        const uint32_t c = best >> 8;
        if (!RIGHT && c <= a.maxCost) {
          disparity[p] = winner_disparity(a, V[xi], edge, k, c, x);
          if (cost) cost[p] = c;
        }
      }
    }
  }
}

// which of a lane's (column, disparity) pairs are candidates, columns x0 .. x0 + 3: the same for every row
template <bool RIGHT>
__device__ __forceinline__ void candidate_bits(const StereoArgs& a, int dl, int x0, uint32_t (&valid)[kXs]) {
#pragma unroll
  for (int xi = 0; xi < kXs; ++xi) {
    const int x = x0 + xi;
    uint32_t bits = 0;
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) {
      const int k = dl * kDc + dk, d = a.dmin + k;
      const int partner = RIGHT ? x + d : x - d;
      if (x <= a.w - 1 - a.r && k < a.D && partner >= a.r && partner <= a.w - 1 - a.r) bits |= 1u << dk;
    }
    valid[xi] = bits;
  }
}

__global__ __launch_bounds__(256) void k_stereo_fill(float* __restrict__ disparity, uint32_t* __restrict__ cost, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    disparity[i] = __uint_as_float(kNaN);
    if (cost) cost[i] = 0xFFFFFFFFu;
  }
}

// RIGHT = false: base = left image, other = right, partner of (x, d) at x - d; writes disparity, cost (or null) and kwin.
// RIGHT = true:  base = right image, other = left, partner at x + d; writes kwin alone.
// VOLUME = true: stores the costs, clamped to `clamp`, into `volume` (uint16 [y][x][nD * 8]) instead of choosing winners.
// Every output has its own parameter; those a form does not write are null.
template <bool RIGHT, bool VOLUME = false>
__global__ __launch_bounds__(256) void k_stereo_sad(const uint8_t* __restrict__ base, const uint8_t* __restrict__ other, StereoArgs a,
                                                    float* __restrict__ disparity, uint32_t* __restrict__ cost, uint8_t* __restrict__ kwin,
                                                    uint16_t* __restrict__ volume, uint32_t clamp) {
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

  uint32_t valid[kXs];
  candidate_bits<RIGHT>(a, dl, X0 + offB, valid);

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

    cost_row_out<RIGHT, VOLUME>(a, V, valid, dl, X0 + offB, y, disparity, cost, kwin, volume, clamp);
  }
}

// ---- census cost (include/ssrlcv_hip.h "census cost"; tests/census_ref.py restates it)
// The code of every pixel whose (2 C + 1)^2 window lies inside the image, 0 elsewhere: bit b = [I(x + i, y + j) < I(x, y)], the
// offsets numbered row by row with the centre skipped.  Every entry of `codes` is written.
template <int C>
__global__ __launch_bounds__(256) void k_census(const uint8_t* __restrict__ image, int w, int h, uint64_t* __restrict__ codes) {
  const size_t n = (size_t)w * h;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
    const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
    uint64_t code = 0;
    if (x >= C && x <= w - 1 - C && y >= C && y <= h - 1 - C) {
      const uint32_t centre = image[p];
      int b = 0;
#pragma unroll
      for (int j = -C; j <= C; ++j)
#pragma unroll
        for (int i = -C; i <= C; ++i) {
          if (i == 0 && j == 0) continue;
          const uint32_t v = image[(size_t)(y + j) * w + (x + i)];
          code |= (uint64_t)(v < centre ? 1u : 0u) << b;
          ++b;
        }
    }
    codes[p] = code;
  }
}

// acc + popcount(a xor b): v_bcnt_u32_b32 takes the addend, so a distance costs one xor and one count per 32 bits
__device__ __forceinline__ uint32_t hamming_add(uint8_t a, uint8_t b, uint32_t acc) { return (uint32_t)__popc((uint32_t)(a ^ b)) + acc; }
__device__ __forceinline__ uint32_t hamming_add(uint32_t a, uint32_t b, uint32_t acc) { return (uint32_t)__popc(a ^ b) + acc; }
__device__ __forceinline__ uint32_t hamming_add(uint64_t a, uint64_t b, uint32_t acc) {
  const uint64_t v = a ^ b;
  return (uint32_t)__popc((uint32_t)(v >> 32)) + ((uint32_t)__popc((uint32_t)v) + acc);
}

// horizontal sums of one staged row of codes: acc[xi][dk] += sum over the 2 ra + 1 columns of popcount(B xor O)
template <class CW, bool RIGHT>
__device__ __forceinline__ void census_row_sums(const CW* __restrict__ rowB, const CW* __restrict__ rowO, int ra, uint32_t (&acc)[kXs][kDc]) {
  for (int j = 0; j <= 2 * ra; ++j) {  // wave-uniform
    CW B[kXs], O[kXs + kDc - 1];
#pragma unroll
    for (int xi = 0; xi < kXs; ++xi) B[xi] = rowB[j + xi];
#pragma unroll
    for (int o = 0; o < kXs + kDc - 1; ++o) O[o] = rowO[j + o];
#pragma unroll
    for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
      for (int dk = 0; dk < kDc; ++dk) acc[xi][dk] = hamming_add(B[xi], O[xi + (RIGHT ? dk : kDc - 1 - dk)], acc[xi][dk]);
  }
}

// The census sibling of k_stereo_sad: the same ownership (a lane owns four columns and eight disparities, nD lanes share a
// pixel, a block marches down a strip with V += h(entering row) - h(leaving row)) and the same three output forms
// (cost_row_out), over C(x, y, d) = sum over the (2 ra + 1)^2 aggregation window of popcount(T_base xor T_other).  `base` and
// `other` are the code maps k_census wrote; a.r is the footprint radius rho = ra + censusRadius, so the strip, the candidate
// test and everything behind the pass see the interior [rho, w - 1 - rho] x [rho, h - 1 - rho]; the rows and columns the
// pass reads reach ra further, where the codes are still defined.  The rows are staged in LDS as CW, the narrowest type that
// holds the code (uint8 for 3 x 3, uint32 for 5 x 5, uint64 for 7 x 7), in a ring of 2 ra + 3 rows from which the leaving row's
// h is recomputed.  ra = 0 has no leaving row: V is the row's h itself and the ring is the two slots the barrier needs.
// LDS: ring * (pitchB + pitchO) * sizeof(CW) with pitchB = TX + 2 ra, pitchO = TX + 2 ra + 8 nD; census_tile halves the strip's
// width TX from k_stereo_sad's until that is at most 64 KB (only 7 x 7 codes need it: at ra = 7 with nD <= 4 and at ra = 6 with
// nD = 2 or 4, TX = 128; the largest ring is 65280 bytes, ra = 6 at nD = 1).
template <class CW, bool RIGHT, bool VOLUME>
__global__ __launch_bounds__(256) void k_stereo_census(const uint64_t* __restrict__ base, const uint64_t* __restrict__ other, StereoArgs a,
                                                       float* __restrict__ disparity, uint32_t* __restrict__ cost, uint8_t* __restrict__ kwin,
                                                       uint16_t* __restrict__ volume, uint32_t clamp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  CW* sB = reinterpret_cast<CW*>(smem);  // [ring][pitchB]
  CW* sO = sB + a.ring * a.pitchB;       // [ring][pitchO]
  const int tid = threadIdx.x;
  const int dl = tid & (a.nD - 1), xl = tid >> a.nDlog;
  const int tx = blockIdx.x % a.tilesX, ty = blockIdx.x / a.tilesX;
  const int X0 = a.r + tx * a.TX;
  const int Y0 = a.r + ty * a.TY;
  const int Y1 = min(Y0 + a.TY, a.h - a.r);
  const int Dtile = a.nD * kDc;
  // global column of staged entry 0 of either map
  const int cb0 = X0 - a.ra;
  const int co0 = RIGHT ? X0 - a.ra + a.dmin : X0 - a.ra - (a.dmin + Dtile - 1);
  const int offB = kXs * xl;
  const int offO = kXs * xl + kDc * (RIGHT ? dl : a.nD - 1 - dl);
  const int nb = a.pitchB + a.pitchO;

  uint32_t valid[kXs];
  candidate_bits<RIGHT>(a, dl, X0 + offB, valid);

  uint32_t V[kXs][kDc];
#pragma unroll
  for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) V[xi][dk] = 0;

  CW pre[kPreCodes];
  auto fetch = [&](int row) {
    const size_t rowAt = (size_t)row * a.w;
#pragma unroll
    for (int q = 0; q < kPreCodes; ++q) {
      const int i = tid + q * a.threads;
      CW v = 0;
      if (i < nb) {
        const bool inB = i < a.pitchB;
        const int col = inB ? cb0 + i : co0 + (i - a.pitchB);
        if (col >= 0 && col < a.w) v = (CW)(inB ? base : other)[rowAt + col];
      }
      pre[q] = v;
    }
  };

  const int T0 = Y0 - a.ra, T1 = Y1 - 1 + a.ra;  // rows of codes this block reads: all inside the image
  fetch(T0);
  for (int t = T0; t <= T1; ++t) {
    const int slot = t % a.ring;
#pragma unroll
    for (int q = 0; q < kPreCodes; ++q) {
      const int i = tid + q * a.threads;
      if (i < nb) {
        if (i < a.pitchB) sB[slot * a.pitchB + i] = pre[q];
        else sO[slot * a.pitchO + (i - a.pitchB)] = pre[q];
      }
    }
    __syncthreads();  // row t is staged; the slot it took was last read two iterations ago
    if (t < T1) fetch(t + 1);

    if (a.ra == 0) {  // block-uniform: the cost is the row's own h
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) V[xi][dk] = 0;
    }
    census_row_sums<CW, RIGHT>(sB + slot * a.pitchB + offB, sO + slot * a.pitchO + offO, a.ra, V);
    const int leaving = t - 2 * a.ra - 1;
    if (a.ra != 0 && leaving >= T0) {  // block-uniform
      const int gone = leaving % a.ring;
      uint32_t acc[kXs][kDc];
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) acc[xi][dk] = 0;
      census_row_sums<CW, RIGHT>(sB + gone * a.pitchB + offB, sO + gone * a.pitchO + offO, a.ra, acc);
#pragma unroll
      for (int xi = 0; xi < kXs; ++xi)
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) V[xi][dk] -= acc[xi][dk];
    }
    const int y = t - a.ra;
    if (y < Y0) continue;  // block-uniform: the window is not full yet

    cost_row_out<RIGHT, VOLUME>(a, V, valid, dl, X0 + offB, y, disparity, cost, kwin, volume, clamp);
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

// ---- semi-global matching over the clamped SAD costs
constexpr uint32_t kSgmBig = 0x0FFFFFFFu;  // a padded entry (k >= D) or a missing neighbour: above every L, and + P2 does not wrap
constexpr int kSgmAhead = 8;               // steps whose M and S loads are in flight ahead of the chain

struct SgmArgs {
  int w, h, r, wi, hi;     // wi x hi: the interior
  int D, dmin, nD, nDlog, K8;  // K8 = nD * 8 entries per pixel of either volume
  uint32_t P1, P2;
  int nPaths;
  int subpixel, wantRight;
  const uint16_t* M;
  uint16_t* S;
};

// One DPP move: lane i takes `v` of the lane CTRL names, or `old` where that lane does not exist (bound_ctrl off).
template <int CTRL>
__device__ __forceinline__ uint32_t sgm_dpp(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xF, 0xF, false);
}

// min over the nD lanes of a group (every lane of the wave active).  Quads swap by quad_perm; once a quad agrees, the mirror of
// a half row pairs it with the other quad of its eight, and the mirror of a row pairs the eights; 32 lanes take one shuffle.
__device__ __forceinline__ uint32_t sgm_group_min(uint32_t m, int nD) {
  if (nD >= 2) m = min(m, sgm_dpp<0xB1>(m, m));    // quad_perm [1, 0, 3, 2]
  if (nD >= 4) m = min(m, sgm_dpp<0x4E>(m, m));    // quad_perm [2, 3, 0, 1]
  if (nD >= 8) m = min(m, sgm_dpp<0x141>(m, m));   // row_half_mirror
  if (nD >= 16) m = min(m, sgm_dpp<0x140>(m, m));  // row_mirror
  if (nD >= 32) m = min(m, (uint32_t)__shfl_xor((int)m, 16, 64));
  return m;
}

template <int DX, int DY, bool FIRST>
__global__ __launch_bounds__(64) void k_sgm_path(SgmArgs a) {
  const int tid = (int)(blockIdx.x * 64u + threadIdx.x);
  const int dl = tid & (a.nD - 1);
  const int path = tid >> a.nDlog;
  // the path's first pixel (u, v) in interior coordinates flipped so that the direction is (+1 or 0, +1 or 0), and its length
  int u, v, len;
  if (DY == 0) { u = 0; v = path; len = a.wi; }
  else if (DX == 0) { u = path; v = 0; len = a.hi; }
  else if (path < a.wi) { u = path; v = 0; len = min(a.wi - path, a.hi); }
  else { u = 0; v = path - a.wi + 1; len = min(a.hi - v, a.wi); }
  if (path >= a.nPaths) { u = 0; v = 0; len = 0; }
  const int x = a.r + (DX >= 0 ? u : a.wi - 1 - u);
  const int y = a.r + (DY >= 0 ? v : a.hi - 1 - v);
  const long long stride = ((long long)DY * a.w + DX) * a.K8;  // elements from a pixel to the next one of the path
  const long long at0 = ((long long)y * a.w + x) * a.K8 + dl * kDc;
  int wlen = len;  // the longest path of this wave: the loop is wave-uniform, a finished group idles
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) wlen = max(wlen, __shfl_xor(wlen, s, 64));

  uint32_t inD = 0;  // which of this lane's eight k are below D
#pragma unroll
  for (int dk = 0; dk < kDc; ++dk)
    if (dl * kDc + dk < a.D) inD |= 1u << dk;

  uint4 mq[kSgmAhead], sq[kSgmAhead];
#pragma unroll
  for (int j = 0; j < kSgmAhead; ++j) {
    mq[j] = make_uint4(0, 0, 0, 0);
    sq[j] = make_uint4(0, 0, 0, 0);
    if (j < len) {
      mq[j] = *reinterpret_cast<const uint4*>(a.M + at0 + j * stride);
      if (!FIRST) sq[j] = *reinterpret_cast<const uint4*>(a.S + at0 + j * stride);
    }
  }

  uint32_t L[kDc];
#pragma unroll
  for (int dk = 0; dk < kDc; ++dk) L[dk] = kSgmBig;

  for (int s0 = 0; s0 < wlen; s0 += kSgmAhead) {
#pragma unroll
    for (int j = 0; j < kSgmAhead; ++j) {
      const int s = s0 + j;
      uint32_t Mk[kDc], Sk[kDc];
      unpack8(mq[j], Mk);
      unpack8(sq[j], Sk);
      if (s + kSgmAhead < len) {
        mq[j] = *reinterpret_cast<const uint4*>(a.M + at0 + (s + kSgmAhead) * stride);
        if (!FIRST) sq[j] = *reinterpret_cast<const uint4*>(a.S + at0 + (s + kSgmAhead) * stride);
      }
      if (s == 0) {  // wave-uniform: the predecessor is outside the interior
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) L[dk] = (inD >> dk) & 1u ? Mk[dk] : kSgmBig;
      } else {
        uint32_t m = L[0];
#pragma unroll
        for (int dk = 1; dk < kDc; ++dk) m = min(m, L[dk]);
        m = sgm_group_min(m, a.nD);
        uint32_t below, above;  // L(q, k - 1) of this lane's first k, L(q, k + 1) of its last
        if (a.nD <= 16) {       // wave-uniform: a group lies inside a row of 16 lanes
          below = sgm_dpp<0x111>(kSgmBig, L[kDc - 1]);  // row_shr:1
          above = sgm_dpp<0x101>(kSgmBig, L[0]);        // row_shl:1
        } else {
          below = (uint32_t)__shfl_up((int)L[kDc - 1], 1, 64);
          above = (uint32_t)__shfl_down((int)L[0], 1, 64);
        }
        if (dl == 0) below = kSgmBig;
        if (dl == a.nD - 1) above = kSgmBig;
        const uint32_t jump = m + a.P2;
        uint32_t N[kDc];
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) {
          const uint32_t lo = dk == 0 ? below : L[dk - 1];
          const uint32_t hi = dk == kDc - 1 ? above : L[dk + 1];
          N[dk] = Mk[dk] + min(min(L[dk], jump), min(lo, hi) + a.P1) - m;
        }
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) L[dk] = (inD >> dk) & 1u ? N[dk] : kSgmBig;
      }
      if (s < len) {
        uint32_t o[kDc];
#pragma unroll
        for (int dk = 0; dk < kDc; ++dk) o[dk] = (inD >> dk) & 1u ? (FIRST ? L[dk] : Sk[dk] + L[dk]) : 0u;  // <= 65535 (the host's bound)
        *reinterpret_cast<uint4*>(a.S + at0 + s * stride) = pack8(o);
      }
    }
  }
}

// A block owns one interior row and T neighbouring pixels of it, as left pixels and as right pixels.  It walks the left pixels
// whose entries either view needs, 256 / nD at a time, every lane with the eight S of its pixel from one 16-byte load: a pixel
// of the block's own gets its left winner (the SAD kernel's key, butterfly and edge shuffles), and every entry S(x, k) whose
// right pixel x - d lies in the block goes to that pixel's row of an LDS tile [T][8 nD]; behind one barrier the right winners
// are read off the tile the same way.  The tile is 32 KB at most (T = 16384 / (8 nD), at most 1024).
__global__ __launch_bounds__(256) void k_sgm_winners(SgmArgs a, int T, int strips, float* __restrict__ disparity, uint32_t* __restrict__ cost,
                                                     uint8_t* __restrict__ kL, uint8_t* __restrict__ kR) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(smem);  // [T][K8]: S(x' + d, y, d) of right pixel x0 + t
  const int tid = threadIdx.x;
  const int dl = tid & (a.nD - 1), pl = tid >> a.nDlog;
  const int P = 256 >> a.nDlog;
  const int strip = (int)(blockIdx.x % (unsigned)strips), v = (int)(blockIdx.x / (unsigned)strips);
  const int y = a.r + v, lo = a.r, hi = a.w - 1 - a.r;
  const int x0 = a.r + strip * T, x1 = min(x0 + T - 1, hi);  // the block's own pixels
  int first = x0, last = x1;                                  // the left pixels it walks
  if (a.wantRight) {
    first = max(lo, min(x0, x0 + a.dmin));
    last = min(hi, max(x1, x1 + a.dmin + a.D - 1));
  }
  const size_t rowAt = (size_t)y * a.w;
  for (int xb = first; xb <= last; xb += P) {  // block-uniform
    const int x = xb + pl;
    const bool there = x <= last;
    const size_t p = rowAt + (there ? x : first);
    uint32_t S[kDc];
    unpack8(*reinterpret_cast<const uint4*>(a.S + p * a.K8 + dl * kDc), S);
    bool cand[kDc];
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) {
      const int k = dl * kDc + dk, partner = x - (a.dmin + k);
      cand[dk] = k < a.D && partner >= lo && partner <= hi;
      if (a.wantRight && there && cand[dk] && partner >= x0 && partner <= x1) tile[(partner - x0) * a.K8 + k] = (uint16_t)S[dk];
    }
    const uint32_t best = winner_key(S, cand, dl, a.nD);
    const EdgeCosts edge = edge_costs(S);
    const int k = (int)(best & 0xFFu);
    if (there && x >= x0 && x <= x1 && best != kNoKey && (k >> 3) == dl) {
      kL[p] = (uint8_t)k;
      disparity[p] = winner_disparity(a, S, edge, k, best >> 8, x);
      if (cost) cost[p] = best >> 8;
    }
  }
  if (!a.wantRight) return;  // block-uniform
  __syncthreads();
  for (int t = pl; t < T; t += P) {  // T is a multiple of P: wave-uniform trip count
    const int xr = x0 + t;
    uint32_t S[kDc];
    unpack8(*reinterpret_cast<const uint4*>(tile + t * a.K8 + dl * kDc), S);
    bool cand[kDc];
#pragma unroll
    for (int dk = 0; dk < kDc; ++dk) {  // an entry nobody wrote belongs to no candidate: never looked at
      const int k = dl * kDc + dk, xl = xr + a.dmin + k;
      cand[dk] = k < a.D && xl >= lo && xl <= hi;
    }
    const uint32_t bestR = winner_key(S, cand, dl, a.nD);
    if (dl == 0 && xr <= x1 && bestR != kNoKey) kR[rowAt + xr] = (uint8_t)(bestR & 0xFFu);
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
// The parameter check of every call, in the contract's order: every invalid argument (the image size last), then what is
// valid and unsupported.  `alsoInvalid` / `alsoUnsupported`: what semi-global matching adds to either tier.  `census`: null for
// the SAD calls; else the census radius, which takes radius 0's place in the invalid tier (an aggregation radius of 0 is
// legal) and narrows the supported radii to the footprint the census cost pass is built for.
int params_status(uint32_t w, uint32_t h, const ssrlcv_stereo_params& p, bool alsoInvalid = false, bool alsoUnsupported = false,
                  const uint32_t* census = nullptr) {
  const bool noWindow = census ? *census == 0 : p.radius == 0;
  if (noWindow || p.numDisparities == 0 || p.minDisparity < -32768 || p.minDisparity > 32767 || p.subpixel > 1 || alsoInvalid)
    return SSRLCV_ERR_INVALID_ARG;
  if ((unsigned long long)w * h >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  const bool wideWindow = census ? *census > 3 || p.radius > 7 : p.radius > 15;
  if (wideWindow || p.numDisparities > 256 || alsoUnsupported) return SSRLCV_ERR_UNSUPPORTED;
  return SSRLCV_OK;
}

int stereo_params_status(uint32_t w, uint32_t h, const ssrlcv_stereo_params* p, const uint32_t* census = nullptr) {
  return p ? params_status(w, h, *p, false, false, census) : SSRLCV_ERR_INVALID_ARG;
}

// dense stereo's share of the parameters: the cost limit is off, the winner pass of semi-global matching has none
ssrlcv_stereo_params sgm_as_stereo(const ssrlcv_sgm_params& p) {
  return {p.radius, p.minDisparity, p.numDisparities, 0xFFFFFFFFu, p.lrTolerance, p.subpixel};
}

int sgm_params_status(uint32_t w, uint32_t h, const ssrlcv_sgm_params* p, const uint32_t* census = nullptr) {
  if (!p) return SSRLCV_ERR_INVALID_ARG;
  // M, L and S live in 16 bits: S <= popcount(paths) (costClamp + P2)
  const bool wide = (unsigned long long)__builtin_popcount(p->paths) * ((unsigned long long)p->costClamp + p->P2) > 65535ull;
  return params_status(w, h, sgm_as_stereo(*p), p->P1 > p->P2 || p->paths == 0 || p->paths > 0xFFu, wide, census);
}

// what everything behind a census cost pass sees: the parameters with the footprint radius rho = radius + censusRadius
ssrlcv_stereo_params census_footprint(ssrlcv_stereo_params p, uint32_t censusRadius) {
  p.radius += censusRadius;
  return p;
}

// samples 0, step, 2 step, ... below n: ceil(n / step) without the sum n + step - 1, which wraps for a step near 2^32
uint32_t stereo_grid(uint32_t n, uint32_t step) { return n ? (n - 1) / step + 1 : 0; }

// The workspace of every call, as byte offsets: the winners' k of both views, one byte per pixel each; for semi-global
// matching (numDisparities != 0) the volumes M and S, uint16 [h][w][8 nD] each, 8 nD = numDisparities rounded up to 8, 16, .. 256;
// and for the census calls the code maps of both views behind them, uint64 [h][w] each.
struct StereoLayout { size_t kL, kR, M, S, TL, TR, total; };
StereoLayout stereo_layout(uint32_t w, uint32_t h, uint32_t numDisparities, bool census = false) {
  const size_t map = align256((size_t)w * h);
  size_t k8 = 8;
  while (k8 < numDisparities) k8 <<= 1;
  const size_t volume = numDisparities ? align256((size_t)w * h * k8 * 2) : 0;
  const size_t codes = census ? align256((size_t)w * h * 8) : 0;
  const size_t sad = 2 * map + 2 * volume + 256;
  return {0, map, 2 * map, 2 * map + volume, sad, sad + codes, sad + 2 * codes};
}

StereoArgs stereo_args(uint32_t w, uint32_t h, const ssrlcv_stereo_params& p) {
  StereoArgs a;
  a.w = (int)w;
  a.h = (int)h;
  a.r = (int)p.radius;
  const int W = 2 * a.r + 1;
  a.G = (W + 3) / 4;
  a.remMask = W - 4 * (a.G - 1) == 1 ? 0xFFu : 0xFFFFFFu;  // W is odd: 1 or 3 bytes in the last dword
  a.D = (int)p.numDisparities;
  a.dmin = p.minDisparity;
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
  a.maxCost = p.maxCost;
  a.subpixel = (int)p.subpixel;
  a.ra = 0;
  return a;
}

// The strip of the census cost pass, from stereo_args of the footprint radius: codes of `codeBytes` bytes staged in a ring of
// 2 ra + 3 rows (two slots for ra = 0), the strip as wide as k_stereo_sad's unless the ring would pass 64 KB of LDS, then half
// as wide (7 x 7 codes only, at ra = 7 with nD <= 4 and at ra = 6 with nD = 2 or 4: 128 columns, and 32 threads a block at
// nD = 1).  TY stays stereo_args' on purpose: a halved strip only means more blocks of the same march.  A thread stages at most
// kPreCodes codes a row: (8 NX + 4 ra + 8 nD) / (NX nD) <= 9.2 at nD = 1, NX = 32, ra = 7.
StereoArgs census_tile(StereoArgs a, int ra, int codeBytes) {
  a.ra = ra;
  a.ring = ra ? 2 * ra + 3 : 2;
  int NX = a.nD >= 4 ? 256 / a.nD : 64;
  for (;; NX >>= 1) {
    a.TX = kXs * NX;
    a.pitchB = a.TX + 2 * ra;
    a.pitchO = a.TX + 2 * ra + a.nD * kDc;
    if ((size_t)a.ring * (a.pitchB + a.pitchO) * codeBytes <= 65536) break;
  }
  a.threads = NX * a.nD;
  a.tilesX = (a.w - 2 * a.r + a.TX - 1) / a.TX;
  return a;
}

SgmArgs sgm_args(const StereoArgs& a, const ssrlcv_sgm_params& p, const uint16_t* M, uint16_t* S) {
  SgmArgs g;
  g.w = a.w; g.h = a.h; g.r = a.r;
  g.wi = a.w - 2 * a.r; g.hi = a.h - 2 * a.r;
  g.D = a.D; g.dmin = a.dmin; g.nD = a.nD; g.nDlog = a.nDlog; g.K8 = a.nD * kDc;
  g.P1 = p.P1; g.P2 = p.P2;
  g.nPaths = 0;  // set per direction
  g.subpixel = a.subpixel; g.wantRight = p.lrTolerance >= 0 ? 1 : 0;
  g.M = M; g.S = S;
  return g;
}

template <bool RIGHT, bool VOLUME = false>
void launch_sad(const StereoArgs& a, hipStream_t st, const uint8_t* base, const uint8_t* other, float* disparity, uint32_t* cost, uint8_t* kwin,
                uint16_t* volume = nullptr, uint32_t clamp = 0) {
  const int tilesY = (a.h - 2 * a.r + a.TY - 1) / a.TY;
  const size_t lds = (size_t)a.ring * (a.pitchB + a.pitchO);
  hipLaunchKernelGGL((k_stereo_sad<RIGHT, VOLUME>), dim3((unsigned)(a.tilesX * tilesY)), dim3(a.threads), lds, st, base, other, a, disparity, cost,
                     kwin, volume, clamp);
}

template <int C>
void launch_census_codes(hipStream_t st, const uint8_t* image, uint32_t w, uint32_t h, uint64_t* codes) {
  const size_t n = (size_t)w * h;
  unsigned blocks = (unsigned)((n + 255) / 256);
  if (blocks > 8192u) blocks = 8192u;
  hipLaunchKernelGGL(k_census<C>, dim3(blocks), dim3(256), 0, st, image, (int)w, (int)h, codes);
}
void launch_census_codes(uint32_t censusRadius, hipStream_t st, const uint8_t* image, uint32_t w, uint32_t h, uint64_t* codes) {
  if (censusRadius == 1) launch_census_codes<1>(st, image, w, h, codes);
  else if (censusRadius == 2) launch_census_codes<2>(st, image, w, h, codes);
  else launch_census_codes<3>(st, image, w, h, codes);
}

template <class CW, bool RIGHT, bool VOLUME>
void launch_census_cost(const StereoArgs& sa, int ra, hipStream_t st, const uint64_t* base, const uint64_t* other, float* disparity, uint32_t* cost,
                        uint8_t* kwin, uint16_t* volume, uint32_t clamp) {
  const StereoArgs a = census_tile(sa, ra, (int)sizeof(CW));
  const int tilesY = (a.h - 2 * a.r + a.TY - 1) / a.TY;
  const size_t lds = (size_t)a.ring * (a.pitchB + a.pitchO) * sizeof(CW);
  hipLaunchKernelGGL((k_stereo_census<CW, RIGHT, VOLUME>), dim3((unsigned)(a.tilesX * tilesY)), dim3(a.threads), lds, st, base, other, a, disparity,
                     cost, kwin, volume, clamp);
}
// `a`: stereo_args of the footprint radius; the aggregation radius is what the census window leaves of it
template <bool RIGHT, bool VOLUME = false>
void launch_census_cost(const StereoArgs& a, uint32_t censusRadius, hipStream_t st, const uint64_t* base, const uint64_t* other, float* disparity,
                        uint32_t* cost, uint8_t* kwin, uint16_t* volume = nullptr, uint32_t clamp = 0) {
  const int ra = a.r - (int)censusRadius;
  if (censusRadius == 1) launch_census_cost<uint8_t, RIGHT, VOLUME>(a, ra, st, base, other, disparity, cost, kwin, volume, clamp);
  else if (censusRadius == 2) launch_census_cost<uint32_t, RIGHT, VOLUME>(a, ra, st, base, other, disparity, cost, kwin, volume, clamp);
  else launch_census_cost<uint64_t, RIGHT, VOLUME>(a, ra, st, base, other, disparity, cost, kwin, volume, clamp);
}

// the directions in the order of the `paths` bits, [first selected direction: it stores S][dir]
using SgmPathKernel = void (*)(SgmArgs);
const SgmPathKernel kSgmPath[2][8] = {
    {k_sgm_path<1, 0, false>, k_sgm_path<-1, 0, false>, k_sgm_path<0, 1, false>, k_sgm_path<0, -1, false>,
     k_sgm_path<1, 1, false>, k_sgm_path<-1, 1, false>, k_sgm_path<1, -1, false>, k_sgm_path<-1, -1, false>},
    {k_sgm_path<1, 0, true>, k_sgm_path<-1, 0, true>, k_sgm_path<0, 1, true>, k_sgm_path<0, -1, true>,
     k_sgm_path<1, 1, true>, k_sgm_path<-1, 1, true>, k_sgm_path<1, -1, true>, k_sgm_path<-1, -1, true>}};

// ssrlcv_hip_stereo_sgm_set_pass_events: the events later calls record between their passes (tools/bench_sgm.py)
constexpr uint32_t kSgmMaxEvents = 12;
void* g_sgm_events[kSgmMaxEvents];
uint32_t g_sgm_event_count = 0;

// semi-global matching behind its cost pass: the selected directions' passes over M into S, then the winner pass; `mark()`
// behind each
template <class Mark>
void sgm_passes(const StereoArgs& a, const ssrlcv_sgm_params& p, const uint16_t* M, uint16_t* S, float* disparity, uint32_t* cost, uint8_t* kL,
                uint8_t* kR, hipStream_t st, Mark& mark) {
  SgmArgs g = sgm_args(a, p, M, S);
  bool first = true;
  for (int dir = 0; dir < 8; ++dir) {
    if (!((p.paths >> dir) & 1u)) continue;
    g.nPaths = dir < 2 ? g.hi : dir < 4 ? g.wi : g.wi + g.hi - 1;
    const unsigned blocks = (unsigned)(((size_t)g.nPaths * g.nD + 63) / 64);
    hipLaunchKernelGGL(kSgmPath[first][dir], dim3(blocks), dim3(64), 0, st, g);
    first = false;
    mark();
  }
  int T = 16384 / g.K8;  // pixels of a row per block of the winner pass: a tile of 32 KB, 64 .. 1024 pixels
  if (T > 1024) T = 1024;
  const int strips = (g.wi + T - 1) / T;
  hipLaunchKernelGGL(k_sgm_winners, dim3((unsigned)strips * (unsigned)g.hi), dim3(256), (size_t)T * g.K8 * 2, st, g, T, strips, disparity,
                     cost, kL, kR);
  mark();
}

// What every call does around its passes, once the parameters have passed their check (first: its codes do not depend on the
// buffers).  `sp`: dense stereo's share of the parameters, its radius the footprint's.  `passes(a, kL, kR)` launches what leaves disparity, cost, kL and, when
// the check is asked for, kR; `mark()` is called before the first launch and behind the last one.
template <class Passes, class Mark>
int stereo_call(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params& sp, const StereoLayout& lay,
                void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, hipStream_t st, Passes passes, Mark mark) {
  if (!left || !right || !workspace || !disparity) return SSRLCV_ERR_INVALID_ARG;
  if (workspaceBytes < lay.total) return SSRLCV_ERR_WORKSPACE;
  const size_t n = (size_t)w * h;
  if (n == 0) return SSRLCV_OK;
  unsigned fillBlocks = (unsigned)((n + 255) / 256);
  if (fillBlocks > 2048u) fillBlocks = 2048u;
  mark();
  hipLaunchKernelGGL(k_stereo_fill, dim3(fillBlocks), dim3(256), 0, st, disparity, cost, n);
  const uint32_t side = 2 * sp.radius + 1;
  if (w >= side && h >= side) {  // else: no pixel has a window
    const StereoArgs a = stereo_args(w, h, sp);
    uint8_t* kL = (uint8_t*)workspace + lay.kL;
    uint8_t* kR = (uint8_t*)workspace + lay.kR;
    passes(a, kL, kR);
    if (sp.lrTolerance >= 0)
      hipLaunchKernelGGL(k_stereo_lr, dim3(fillBlocks), dim3(256), 0, st, disparity, cost, kL, kR, (int)w, n, a.dmin, sp.lrTolerance);
    mark();
  }
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

// Block matching, SAD (censusRadius == 0) or census: the parameters have passed their check
int block_matching_call(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params& p, uint32_t censusRadius,
                        void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, hipStream_t st) {
  const StereoLayout lay = stereo_layout(w, h, 0, censusRadius != 0);
  return stereo_call(
      left, right, w, h, census_footprint(p, censusRadius), lay, workspace, workspaceBytes, disparity, cost, st,
      [&](const StereoArgs& a, uint8_t* kL, uint8_t* kR) {
        if (censusRadius == 0) {
          launch_sad<false>(a, st, left, right, disparity, cost, kL);
          if (p.lrTolerance >= 0) launch_sad<true>(a, st, right, left, nullptr, nullptr, kR);
          return;
        }
        uint64_t* TL = (uint64_t*)((uint8_t*)workspace + lay.TL);
        uint64_t* TR = (uint64_t*)((uint8_t*)workspace + lay.TR);
        launch_census_codes(censusRadius, st, left, w, h, TL);
        launch_census_codes(censusRadius, st, right, w, h, TR);
        launch_census_cost<false>(a, censusRadius, st, TL, TR, disparity, cost, kL);
        if (p.lrTolerance >= 0) launch_census_cost<true>(a, censusRadius, st, TR, TL, nullptr, nullptr, kR);
      },
      [] {});
}

// Semi-global matching over the SAD (censusRadius == 0) or the census costs: the parameters have passed their check
int sgm_call(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_sgm_params& p, uint32_t censusRadius, void* workspace,
             size_t workspaceBytes, float* disparity, uint32_t* cost, hipStream_t st) {
  const StereoLayout lay = stereo_layout(w, h, p.numDisparities, censusRadius != 0);
  uint32_t marks = 0;
  auto mark = [&]() {  // the next pass event, if the caller of set_pass_events asked for one
    if (marks < g_sgm_event_count && g_sgm_events[marks]) (void)hipEventRecord((hipEvent_t)g_sgm_events[marks], st);
    ++marks;
  };
  return stereo_call(
      left, right, w, h, census_footprint(sgm_as_stereo(p), censusRadius), lay, workspace, workspaceBytes, disparity, cost, st,
      [&](const StereoArgs& a, uint8_t* kL, uint8_t* kR) {
        uint16_t* M = (uint16_t*)((uint8_t*)workspace + lay.M);
        uint16_t* S = (uint16_t*)((uint8_t*)workspace + lay.S);
        if (censusRadius == 0) {
          launch_sad<false, true>(a, st, left, right, nullptr, nullptr, nullptr, M, p.costClamp);
        } else {
          uint64_t* TL = (uint64_t*)((uint8_t*)workspace + lay.TL);
          uint64_t* TR = (uint64_t*)((uint8_t*)workspace + lay.TR);
          launch_census_codes(censusRadius, st, left, w, h, TL);
          launch_census_codes(censusRadius, st, right, w, h, TR);
          launch_census_cost<false, true>(a, censusRadius, st, TL, TR, nullptr, nullptr, nullptr, M, p.costClamp);
        }
        mark();
        sgm_passes(a, p, M, S, disparity, cost, kL, kR, st, mark);
      },
      mark);
}

}  // namespace

extern "C" {

size_t ssrlcv_hip_stereo_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_stereo_params* params) {
  return stereo_params_status(w, h, params) ? 0 : stereo_layout(w, h, 0).total;
}

int ssrlcv_hip_stereo_sad_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params* params,
                             void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, ssrlcv_stream_t stream) {
  if (const int rc = stereo_params_status(w, h, params)) return rc;
  return block_matching_call(left, right, w, h, *params, 0, workspace, workspaceBytes, disparity, cost, (hipStream_t)stream);
}

size_t ssrlcv_hip_stereo_sgm_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_sgm_params* params) {
  return sgm_params_status(w, h, params) ? 0 : stereo_layout(w, h, params->numDisparities).total;
}

int ssrlcv_hip_stereo_sgm_set_pass_events(void* const* events, uint32_t count) {
  if (count > kSgmMaxEvents || (count && !events)) return SSRLCV_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < count; ++i) g_sgm_events[i] = events[i];
  g_sgm_event_count = count;
  return SSRLCV_OK;
}

int ssrlcv_hip_stereo_sgm_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_sgm_params* params,
                             void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, ssrlcv_stream_t stream) {
  if (const int rc = sgm_params_status(w, h, params)) return rc;
  return sgm_call(left, right, w, h, *params, 0, workspace, workspaceBytes, disparity, cost, (hipStream_t)stream);
}

int ssrlcv_hip_census_u8(const uint8_t* image, uint32_t w, uint32_t h, uint32_t censusRadius, uint64_t* codes, ssrlcv_stream_t stream) {
  if (censusRadius == 0 || (unsigned long long)w * h >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  if (censusRadius > 3) return SSRLCV_ERR_UNSUPPORTED;
  if (!image || !codes) return SSRLCV_ERR_INVALID_ARG;
  if ((size_t)w * h == 0) return SSRLCV_OK;
  launch_census_codes(censusRadius, (hipStream_t)stream, image, w, h, codes);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

size_t ssrlcv_hip_stereo_census_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_stereo_params* params, uint32_t censusRadius) {
  return stereo_params_status(w, h, params, &censusRadius) ? 0 : stereo_layout(w, h, 0, true).total;
}

int ssrlcv_hip_stereo_census_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params* params,
                                uint32_t censusRadius, void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost,
                                ssrlcv_stream_t stream) {
  if (const int rc = stereo_params_status(w, h, params, &censusRadius)) return rc;
  return block_matching_call(left, right, w, h, *params, censusRadius, workspace, workspaceBytes, disparity, cost, (hipStream_t)stream);
}

size_t ssrlcv_hip_stereo_sgm_census_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_sgm_params* params, uint32_t censusRadius) {
  return sgm_params_status(w, h, params, &censusRadius) ? 0 : stereo_layout(w, h, params->numDisparities, true).total;
}

int ssrlcv_hip_stereo_sgm_census_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_sgm_params* params,
                                    uint32_t censusRadius, void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost,
                                    ssrlcv_stream_t stream) {
  if (const int rc = sgm_params_status(w, h, params, &censusRadius)) return rc;
  return sgm_call(left, right, w, h, *params, censusRadius, workspace, workspaceBytes, disparity, cost, (hipStream_t)stream);
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
