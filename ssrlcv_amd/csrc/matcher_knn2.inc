// ssrlcv_amd/csrc/matcher_knn2.inc -- the TWO nearest targets of every query (included by matcher.hip inside its anonymous
// namespace, behind matcher_i8.inc: shares k_pack_i8's rows and tile records, make_key and the constants of the integer
// formulation).  What Lowe's ratio test needs, d1 < ratio^2 d2, is the second-best distance, and that never leaves
// k_match_i8: a lane there keeps one key and its fast-path bound is the best value.  k_match2_i8 is the brute-force
// instantiation of that kernel with
//   * two keys per lane and resident query tile, key1 < key2 (same key: distance, f mod 32, f);
//   * the fast-path bound of the SECOND best: a row is a candidate while v <= the second-best v (<=: the key breaks ties);
//   * the bound the two lane halves of a query share = the smaller of their SECOND-best values.  (The smaller of their best
//     values is not a bound: the half that holds the query's nearest target would then drop the second nearest when that
//     sits in the same half.)  A half that takes over its partner's tighter bound may from then on miss its OWN second
//     best, never one of the query's two: the partner already holds two keys at or below that bound;
//   * no threshold, no prefilter, no permutation: mode 0 at an infinite threshold;
//   * no atomics on the way out: every (target split, lane half) stores its two keys to its own slot of a partial array,
//     and k_knn2_merge takes the two smallest of a query's 2 x splits pairs.  The result is a function of the inputs alone.
// int8 MFMA only (v_mfma_i32_32x32x32_i8); ssrlcv_hip_set_match_arithmetic does not reach it -- both arithmetics are exact.
// The LDS ring (a tile fetched once per block, kStep tiles per barrier) is the one of k_match_i8's brute-force branch.
#ifndef SSRLCV_MATCH2_QT
#define SSRLCV_MATCH2_QT 4
#endif
constexpr int kQT8Knn2 = SSRLCV_MATCH2_QT;            // query tiles per wave
constexpr int kQPerBlock8Knn2 = kWaves * kQT8Knn2 * 32;
static_assert(kQPerBlock8 % kQPerBlock8Knn2 == 0, "make_layout pads the queries to a multiple of kQPerBlock8");

struct Key2 { unsigned long long k1, k2; };  // 16 bytes: one store per lane

template <int QT>
__global__ __launch_bounds__(256, QT >= 4 ? 2 : 4) void k_match2_i8(const uint8_t* __restrict__ packedQ, const uint8_t* __restrict__ packedT,
                                                                    const int* __restrict__ normQ, const int* __restrict__ normT,
                                                                    uint32_t nq_pad, uint32_t nt, uint32_t tilesPerSplit,
                                                                    Key2* __restrict__ partial) {
  static_assert(QT % 2 == 0, "query tiles are processed in pairs");
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned col = lane & 31, kgrp = lane >> 5;
  const uint32_t qbase = (blockIdx.x * kWaves + wave) * (QT * 32);
  const uint32_t numTiles = (nt + 31) / 32;
  const uint32_t tile0 = blockIdx.y * tilesPerSplit;
  uint32_t tile1 = tile0 + tilesPerSplit;
  if (tile1 > numTiles) tile1 = numTiles;

  i32x4 bq[QT][4];
  int na[QT];     // |q'|^2
  // The bound is the second-best v = |t'|^2 - 2 dot so far, shared with the other lane half; it is kept in accumulator
  // space only (v <= bound needs a >= -(bound >> 1)): anything >= thr goes to the slow path, where the keys decide exactly.
  // (A copy in v space, as k_match_i8 keeps, cost 32 bytes of scratch at four query tiles.)
  int thr[QT];
  unsigned long long key1[QT], key2[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const uint32_t q = qbase + qt * 32 + col;  // padded rows exist up to nq_pad
    const i32x4* row = reinterpret_cast<const i32x4*>(packedQ + (size_t)q * kRow8) + kgrp;
#pragma unroll
    for (int s = 0; s < 4; ++s) bq[qt][s] = row[2 * s];
    na[qt] = normQ[q];
    thr[qt] = -(0x7fffffff >> 1);
    key1[qt] = kNoKey;
    key2[qt] = kNoKey;
  }
  // plain max(max()), as in k_match_i8: the back end sees that the operands are MFMA results and inserts the wait states
  auto max3 = [](int a, int b, int c) {
    const int ab = a > b ? a : b;
    return ab > c ? ab : c;
  };
  auto epilogue = [&](uint32_t tt, int qt, const i32x16& acc, const int* nslot) {
    int m0 = max3(acc[0], acc[1], acc[2]);
    int m1 = max3(acc[3], acc[4], acc[5]);
    int m2 = max3(acc[6], acc[7], acc[8]);
    int m3 = max3(acc[9], acc[10], acc[11]);
    int m4 = max3(acc[12], acc[13], acc[14]);
    int m = max3(max3(m0, m1, m2), max3(m3, m4, acc[15]), m0);
    if (__any(m >= thr[qt])) {
      bool improved = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (acc[r] >= thr[qt]) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * (int)kgrp;
          const int v = (nslot[row] & 1) - 2 * acc[r];  // |t'|^2 - 2 dot
          const uint32_t f = tt * 32 + (uint32_t)row;
          if (f < nt) {
            const unsigned long long k = make_key((float)(na[qt] + v), f);  // exact integer < 2^24
            // selects on the values (as branches the compiler merged the two stores into one through a selected
            // address, which put both key arrays on the stack)
            const bool lt1 = k < key1[qt], lt2 = k < key2[qt];  // key1 < key2: lt1 implies lt2
            key2[qt] = lt1 ? key1[qt] : (lt2 ? k : key2[qt]);
            key1[qt] = lt1 ? k : key1[qt];
            improved = improved || lt2;
          }
        }
      }
      if (__any(improved)) {
        // this half's second-best v (none yet: no bound of its own), then the smaller of the two halves'
        const int b = key2[qt] != kNoKey ? (int)(uint32_t)(key2[qt] >> 32) - na[qt] : 0x7fffffff;
        int t = -(b >> 1);
        t = t > thr[qt] ? t : thr[qt];  // (a bound taken over from the partner may be tighter than this half's own)
        const int pt = __shfl_xor(t, 32, 64);
        thr[qt] = pt > t ? pt : t;
      }
    }
  };
  auto chain2 = [&](const i32x4 (&a)[4], int qt, const i32x16& cin, i32x16& accA, i32x16& accB) {
    accA = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0], bq[qt][0], cin, 0, 0, 0);
    accB = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0], bq[qt + 1][0], cin, 0, 0, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      accA = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[qt][s], accA, 0, 0, 0);
      accB = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[qt + 1][s], accB, 0, 0, 0);
    }
  };
  auto process_tile = [&](uint32_t tt, const i32x4 (&a)[4], const i32x16& cin, const int* nslot) {
    i32x16 acc[2][2];
    chain2(a, 0, cin, acc[0][0], acc[0][1]);
#pragma unroll
    for (int qp = 1; qp < QT / 2; ++qp) {
      chain2(a, 2 * qp, cin, acc[qp & 1][0], acc[qp & 1][1]);
      epilogue(tt, 2 * qp - 2, acc[(qp - 1) & 1][0], nslot);
      epilogue(tt, 2 * qp - 1, acc[(qp - 1) & 1][1], nslot);
    }
    epilogue(tt, QT - 2, acc[(QT / 2 - 1) & 1][0], nslot);
    epilogue(tt, QT - 1, acc[(QT / 2 - 1) & 1][1], nslot);
  };
  // the ring of k_match_i8's brute-force branch: every wave loads a quarter of a tile one step ahead into registers, drops
  // it into an LDS slot, all four read their operands back; kStep tiles per barrier, 2 kStep slots
  constexpr int kStep = SSRLCV_MATCH_STEP;
  constexpr int kSlots = 2 * kStep;
  __shared__ i32x4 s_tile[kSlots][8 * 32];
  __shared__ int s_nt[kSlots][32];  // |t'|^2 of the slot's rows (slow path: its parity)
  __shared__ int s_nh[kSlots][32];  // -floor(|t'|^2 / 2): the accumulators' start values
  const unsigned ldChunk = 2 * wave + kgrp;
  auto fetch = [&](uint32_t tt, i32x4& stA, int& stN) {
    const uint32_t t = tt < tile1 ? tt : tile1 - 1;  // past the end: re-read the last tile (never stored)
    stA = *(reinterpret_cast<const i32x4*>(packedT + (size_t)t * kTileRec) + ldChunk * 32 + col);
    if (wave == 0) stN = normT[(size_t)t * 32 + col];
  };
  auto stash = [&](uint32_t slot, const i32x4& stA, int stN) {
    s_tile[slot][ldChunk * 32 + col] = stA;
    if (wave == 0 && kgrp == 0) {
      s_nt[slot][col] = stN;
      s_nh[slot][col] = -(stN >> 1);
    }
  };
  auto operands = [&](uint32_t slot, i32x4 (&a)[4], i32x16& cin) {
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) a[s2] = s_tile[slot][(2 * s2 + kgrp) * 32 + col];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const i32x4 h4 = *reinterpret_cast<const i32x4*>(&s_nh[slot][4 * kgrp + 8 * g4]);
      cin[4 * g4] = h4[0]; cin[4 * g4 + 1] = h4[1]; cin[4 * g4 + 2] = h4[2]; cin[4 * g4 + 3] = h4[3];
    }
  };
  if (tile0 < tile1) {  // (uniform over the block; a split past the last tile only writes its empty pairs)
    i32x4 sa[kStep];
    int sn[kStep];
#pragma unroll
    for (int j = 0; j < kStep; ++j) { sn[j] = 0; fetch(tile0 + j, sa[j], sn[j]); }
#pragma unroll
    for (int j = 0; j < kStep; ++j)
      if (tile0 + j < tile1) stash((uint32_t)j, sa[j], sn[j]);
#pragma unroll
    for (int j = 0; j < kStep; ++j) fetch(tile0 + kStep + j, sa[j], sn[j]);
    __syncthreads();
    uint32_t half = 0;
    for (uint32_t tt = tile0; tt < tile1; tt += kStep) {
      const uint32_t other = kStep - half;
#pragma unroll
      for (int j = 0; j < kStep; ++j)
        if (tt + kStep + j < tile1) stash(other + (uint32_t)j, sa[j], sn[j]);
#pragma unroll
      for (int j = 0; j < kStep; ++j) fetch(tt + 2 * kStep + j, sa[j], sn[j]);
      i32x4 a[2][4];
      i32x16 cin[2];
      operands(half, a[0], cin[0]);
#pragma unroll
      for (int j = 0; j < kStep; ++j) {
        if (tt + j < tile1) {  // uniform
          if (j + 1 < kStep) operands(half + (uint32_t)j + 1, a[(j + 1) & 1], cin[(j + 1) & 1]);
          process_tile(tt + j, a[j & 1], cin[j & 1], s_nt[half + (uint32_t)j]);
        }
      }
      half = other;
      __syncthreads();
    }
  }
  // partial[(split, lane half)][query]: every slot of the array is written by exactly one lane of one block
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const uint32_t q = qbase + qt * 32 + col;
    Key2 o;
    o.k1 = key1[qt];
    o.k2 = key2[qt];
    partial[(size_t)(blockIdx.y * 2 + kgrp) * nq_pad + q] = o;
  }
}

// the two smallest of a query's 2 x splits pairs (the pairs hold disjoint targets: all keys but kNoKey differ)
__global__ __launch_bounds__(256) void k_knn2_merge(const Key2* __restrict__ partial, uint32_t nq, uint32_t nq_pad, uint32_t lists,
                                                    Key2* __restrict__ best) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  unsigned long long k1 = kNoKey, k2 = kNoKey;
  for (uint32_t l = 0; l < lists; ++l) {
    const Key2 p = partial[(size_t)l * nq_pad + q];
    if (p.k1 < k1) {
      k2 = k1 < p.k2 ? k1 : p.k2;
      k1 = p.k1;
    } else if (p.k1 < k2) {
      k2 = p.k1;
    }
  }
  Key2 o;
  o.k1 = k1;
  o.k2 = k2;
  best[q] = o;
}

__device__ __forceinline__ uint32_t key_index(unsigned long long k) {
  const uint32_t lo = (uint32_t)(k & 0xffffffffull);
  return ((lo & 0x07ffffffu) << 5) | (lo >> 27);
}

__global__ __launch_bounds__(256) void k_knn2_out(const Key2* __restrict__ best, uint32_t nq, uint32_t* __restrict__ index_out,
                                                  float* __restrict__ dist_out) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const Key2 b = best[q];
  index_out[2 * (size_t)q] = b.k1 != kNoKey ? key_index(b.k1) : 0xffffffffu;
  index_out[2 * (size_t)q + 1] = b.k2 != kNoKey ? key_index(b.k2) : 0xffffffffu;
  if (dist_out) {
    dist_out[2 * (size_t)q] = b.k1 != kNoKey ? (float)(uint32_t)(b.k1 >> 32) : __builtin_inff();
    dist_out[2 * (size_t)q + 1] = b.k2 != kNoKey ? (float)(uint32_t)(b.k2 >> 32) : __builtin_inff();
  }
}

// ratio test, absolute threshold and mutual check -> the output structs, kept or rejected entries written as k_finalize
// writes them (padding bytes zero).  reverseKey (nullable): the one-nearest keys of the targets among all queries.
__global__ __launch_bounds__(256) void k_finalize_ratio(const Key2* __restrict__ best, uint32_t nq,
                                                        const unsigned long long* __restrict__ reverseKey,
                                                        const ssrlcv_sift_feature* __restrict__ query,
                                                        const ssrlcv_sift_feature* __restrict__ target, uint32_t queryID,
                                                        uint32_t targetID, float ratio, float absThreshold, int outKind,
                                                        void* __restrict__ out) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const Key2 b = best[q];
  const bool found = b.k1 != kNoKey;
  const float d1 = found ? (float)(uint32_t)(b.k1 >> 32) : absThreshold;
  const uint32_t j = found ? key_index(b.k1) : 0u;
  bool keep = found && !(d1 >= absThreshold);
  // (float)d1 < (ratio * ratio) * (float)d2, each product rounded to float32 (the build has -ffp-contract=off)
  if (keep && ratio > 0.0f && b.k2 != kNoKey) keep = d1 < (ratio * ratio) * (float)(uint32_t)(b.k2 >> 32);
  if (keep && reverseKey) {
    const unsigned long long rk = reverseKey[j];
    keep = rk != kNoKey && key_index(rk) == q;
  }
  if (outKind == SSRLCV_OUT_UINT2_PAIR) {
    ssrlcv_uint2_pair m;
    m.a.x = queryID; m.a.y = q;
    m.b.x = keep ? targetID : queryID;
    m.b.y = keep ? j : q;
    reinterpret_cast<ssrlcv_uint2_pair*>(out)[q] = m;
    return;
  }
  static_assert(sizeof(ssrlcv_dmatch) == 48 && sizeof(ssrlcv_match) == 40, "DMatch / Match layout");
  uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // invalid 0 | kp0 {parentId 2, loc 4 5} | kp1 {6, 8 9} | distance 10
  w[0] = keep ? 0u : 1u;
  if (keep) {
    const ssrlcv_float2 lq = query[q].loc, lt = target[j].loc;
    w[2] = queryID; w[4] = __float_as_uint(lq.x); w[5] = __float_as_uint(lq.y);
    w[6] = targetID; w[8] = __float_as_uint(lt.x); w[9] = __float_as_uint(lt.y);
  }
  w[10] = __float_as_uint(d1);
  const int words = outKind == SSRLCV_OUT_DMATCH ? 12 : 10;
  uint32_t* o = reinterpret_cast<uint32_t*>(out) + (size_t)q * words;
  for (int i = 0; i < words; ++i) o[i] = w[i];
}
