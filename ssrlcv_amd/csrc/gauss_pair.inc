// ssrlcv_amd/csrc/gauss_pair.inc -- S4 for the first TWO levels of an octave in one launch (round 6).
// Included by pyramid.hip inside its anonymous namespace (shares block_minmax_commit, kTX).
//
// Levels 0 and 1 of an octave (13 and 17 taps, src/FeatureFactory.cu:63-82 building blur b from blur b - 1 by
// convolveSeparable, src/Image.cu:1197-1239,1526-1546) are the two launches of the scale space that sit at the copy floor:
// level 1 is read-4-write-4 bytes per pixel at 4.6-4.9 TB/s and level 0 of octave 0 (whose input is the 2x upsample of
// the u8 image, S1 + S2) writes 268 MB in the time level 1 moves 536 (profiles/r06_pyramid_floor.json).  Both levels have
// to be written (the DoG / extrema pass and the key-point stage read them), but level 0 need not be READ again: here one
// block forms a tile of level 0, keeps it in LDS, and forms level 1 from it.  Per octave-0 image: 17 + 268 + 268 MB instead
// of 285 + 536, one launch instead of two, and the u8 rows reach the lanes through LDS (one 4-byte load per thread and
// step) instead of sixteen byte loads per lane.
//
// Arithmetic = k_gauss_strip's (and so the reference's `sum += pixel * weight` chains in tap order, horizontal pass
// first): the vector formulation, weights in SGPRs.  What is new is the hand-over between the levels:
//   * a block owns TWB = 240 columns of level b (= level a + 1) and forms level a on the 256 columns those need (8 more on
//     either side; the neighbour strips form them too -- 6.7 % more level-a arithmetic, no extra memory traffic);
//   * both levels march down the image 8 rows per step.  Level a's march starts DA rows early so that its results come
//     out as row tiles aligned to multiples of 8; a finished tile goes to global memory (the columns and rows this block
//     owns) and into one of two LDS buffers, where level b's horizontal pass finds it one step later;
//   * level b reads level a with the reference's mirror (getSymmetrizedCoord): columns outside the image are written into
//     the LDS tile by the thread that owns their mirror image; rows outside are the tile of rows 0..7 (or H - 8..H - 1)
//     read in REVERSE order, one extra step at the top and at the bottom of the image (RB == 8 == the step height makes
//     the mirrored rows exactly one tile);
//   * a step is two phases, H (both levels' horizontal passes) and V (both vertical passes), with one barrier each.
// Results are bit-identical to the two separate launches (tests/test_gpu_sift.py, tools/gauss_pair_lab.hip).
struct PairArgs {
  const float* in;       // level a's input, w x h (UPS: not read)
  const uint8_t* u8;     // UPS: the u8 image (w / 2) x (h / 2) whose 2x bilinear upsample is the input
  float* outA;
  float* outB;
  float* minmaxA;        // nullable: {min, max} of level a / level b
  float* minmaxB;
  uint32_t w, h;
  uint32_t rowsPerBlock; // multiple of 8
  float wgtA[9], wgtB[9];  // taps k = 0..R of each level (bit-symmetric), zero-padded in front to the templated radius
#ifdef SSRLCV_STAMPS
  long long* stamps;       // tools/gauss_pair_lab.hip: s_memtime stamps of one block, [wave][step][8]
#endif
};

#ifndef SSRLCV_PAIR_VGPR_WEIGHTS
#define SSRLCV_PAIR_VGPR_WEIGHTS 1  // (measured: 236 against 263 us per 8192^2 u8-sourced pair with the weights in SGPRs -- the kernel is bound by FMA issue)
#endif

template <int RA, bool UPS>
__global__ __launch_bounds__(256) void k_gauss_pair(PairArgs a) {
  constexpr int RB = 8, RP = 8, NR = 8;
  constexpr int TWA = 256, TWB = TWA - 2 * RB;      // 240 columns of level b per block
  constexpr int SWA = TWA + 2 * RP;                 // staged input columns of level a
  constexpr int WINA = 2 * RA + NR, WINB = 2 * RB + NR;
  constexpr int HQ = (2 * RP + 8) / 4;              // float4 reads of a horizontal pass (both levels stage a halo of 8)
  constexpr int DA = (8 - (2 * RA) % 8) % 8;        // level a's march starts DA rows early: its results then come in aligned tiles
  constexpr int LAG = (2 * RA + DA) / 8;            // steps before level a's first tile (2 for RA = 6 and RA = 8)
  static_assert(RA >= 1 && RA <= RP && LAG == 2 && kTX == TWA && kNR == NR, "geometry");
  constexpr int U8DW = 36, U8ROWB = U8DW * 4;       // UPS: 144 source bytes per staged u8 row, five rows per step
  __shared__ float4 s_inA4[NR][SWA / 4];
  __shared__ float4 s_hA4[NR][TWA / 4];
  __shared__ float4 s_inB4[2][NR][TWA / 4];
  __shared__ float4 s_hB4[NR][TWB / 4];
  __shared__ uint32_t s_u8[UPS ? 5 * U8DW : 1];
  float* s_inA = reinterpret_cast<float*>(&s_inA4[0][0]);
  float* s_hA = reinterpret_cast<float*>(&s_hA4[0][0]);
  float* s_inB = reinterpret_cast<float*>(&s_inB4[0][0][0]);
  float* s_hB = reinterpret_cast<float*>(&s_hB4[0][0]);

  const int W = (int)a.w, H = (int)a.h;
  const int xb0 = blockIdx.x * TWB, xa0 = xb0 - RB;
  const int y0 = blockIdx.y * (int)a.rowsPerBlock;
  int nrows = (int)a.rowsPerBlock;
  if (y0 + nrows > H) nrows = H - y0;               // (H and rowsPerBlock are multiples of 8)
  const int A0 = y0 >= 8 ? y0 - 8 : 0;              // first level-a row this block forms (the image has no row above 0)
  const int Aend = y0 + nrows + 8 < H ? y0 + nrows + 8 : H;
  const int nt = (Aend - A0) / 8;                   // level-a tiles
  const int nq = nrows / 8 + 2;                     // level-b steps: virtual rows y0 - 8 .. y0 + nrows + 7
  const int steps = nt + 2 > nq + 3 ? nt + 2 : nq + 3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hr = tid >> 5, hg = tid & 31, hq = hg * 2;  // horizontal-pass role: row hr, outputs 8 hg .. + 7

  float wa[RA + 1], wb[RB + 1];
#pragma unroll
  for (int k = 0; k <= RA; ++k) {
    wa[k] = a.wgtA[k];
#if SSRLCV_PAIR_VGPR_WEIGHTS
    asm volatile("" : "+v"(wa[k]));
#endif
  }
#pragma unroll
  for (int k = 0; k <= RB; ++k) {
    wb[k] = a.wgtB[k];
#if SSRLCV_PAIR_VGPR_WEIGHTS
    asm volatile("" : "+v"(wb[k]));
#endif
  }
  auto mirror_col = [&](int x) {  // getSymmetrizedCoord for the columns a valid result reads; beyond them: any pixel of the image
    x = x > W - 1 + RP ? W - 1 + RP : x;
    x = x < -2 * RP ? -2 * RP : x;
    x = x < 0 ? -1 - x : x;
    return x > W - 1 ? 2 * W - 1 - x : x;
  };
  auto mirror_row = [&](int y) {  // wave-uniform
    y = y > H - 1 + RP ? H - 1 + RP : y;
    y = y < -2 * RP ? -2 * RP : y;
    y = y < 0 ? -1 - y : y;
    return y > H - 1 ? 2 * H - 1 - y : y;
  };

  // ---- level a's loader
  // float input: a wave stages rows 2 wave, 2 wave + 1 of a step; lane l holds the 16-byte chunk l of the 68 a staged row
  // has (columns xa0 - 8 + 4 l ..), lanes 0..3 also chunk 64 + l.  A chunk that lies inside the image is one 16-byte load,
  // one that crosses its border four mirrored 4-byte loads.
  const int cM = xa0 - RP + 4 * lane, cE = xa0 - RP + 4 * (64 + lane);
  const bool hasE = lane < (SWA / 4 - 64);
  int gxM[4], gxE[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    gxM[e] = mirror_col(cM + e);
    gxE[e] = mirror_col(cE + e);
  }
  float4 preM0 = make_float4(0.f, 0.f, 0.f, 0.f), preM1 = preM0, preE0 = preM0, preE1 = preM0;
  typedef unsigned u32x4p __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, UPS ? 0 : (int)((uint32_t)W * (uint32_t)H * 4u), 0x00020000);
  // (a strip whose staged columns all lie inside the image -- every strip but the first and the last one or two -- loads
  // whole chunks through the buffer descriptor, row offset scalar; the others element by element with mirrored columns.
  // Written as two loaders behind a wave-uniform switch: as one loader with a per-lane choice the compiler merged the two
  // into four 4-byte loads per chunk for everybody)
  const bool innerStrip = xa0 - RP >= 0 && xa0 + TWA + RP <= W;
  auto load_chunk = [&](const float* row, const int (&gx)[4]) { return make_float4(row[gx[0]], row[gx[1]], row[gx[2]], row[gx[3]]); };
  auto load_vec = [&](int y, int c0) {
    const u32x4p v = __builtin_amdgcn_raw_buffer_load_b128(rin, c0 * 4, (int)((unsigned)y * (unsigned)W * 4u), 0);
    const f32x4 t = __builtin_bit_cast(f32x4, v);  // (the whole vector: __builtin_bit_cast of a vector ELEMENT reads element 0, see gauss_rm.inc)
    return make_float4(t[0], t[1], t[2], t[3]);
  };
  // UPS: thread t forms column t of the staged row (and column 256 + t for t < 16) from the u8 rows in LDS.  Its two source
  // columns (xm, xp' of upsample_at, after the convolution's mirror on the upsampled column) are fixed for the whole march.
  const int uw = W >> 1, uh = H >> 1;
  int xsBase = (xa0 - RP) >> 1;
  xsBase = xsBase > uw - U8ROWB ? uw - U8ROWB : xsBase;
  xsBase = xsBase < 0 ? 0 : xsBase;
  xsBase &= ~3;
  int bm0 = 0, bp0 = 0, bm1 = 0, bp1 = 0;
  if (UPS) {
    const int s0 = mirror_col(xa0 - RP + tid), s1 = mirror_col(xa0 - RP + 256 + (tid & 15));
    const int m0 = s0 >> 1, m1 = s1 >> 1;
    bm0 = m0 - xsBase;
    bp0 = ((s0 & 1) ? (m0 + 1 < uw ? m0 + 1 : uw - 1) : m0) - xsBase;
    bm1 = m1 - xsBase;
    bp1 = ((s1 & 1) ? (m1 + 1 < uw ? m1 + 1 : uw - 1) : m1) - xsBase;
  }
  uint32_t preU = 0;
  // the five u8 rows a step's eight upsampled rows are made of: rows rlo .. rlo + 4, and per upsampled row i its two
  // source rows as slots 0..4 (packed 4 bits each: slot of ym in bits 8 i .. 8 i + 3, of yp' in bits 8 i + 4 .. + 7)
  auto u8_rows = [&](int ybase, int& rlo, unsigned long long& slots) {
    int ym[NR], yp[NR];
    rlo = 1 << 30;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int Y = mirror_row(ybase + i);
      ym[i] = Y >> 1;
      yp[i] = (Y & 1) ? (ym[i] + 1 < uh ? ym[i] + 1 : uh - 1) : ym[i];
      rlo = ym[i] < rlo ? ym[i] : rlo;
    }
    rlo = rlo > uh - 5 ? uh - 5 : rlo;
    slots = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) slots |= (unsigned long long)((ym[i] - rlo) | ((yp[i] - rlo) << 4)) << (8 * i);
  };
  const int F0 = A0 - DA - RA;  // first input row level a's march feeds (virtual: mirrored by the loader)
  // the u8 rows of a step away from the image's top and bottom: rows (ybase >> 1) .. + 4 in the fixed slot pattern
  constexpr unsigned long long kRegularSlots = 0x4333322221111000ull;
  auto u8_rows_of = [&](int ybase, int& rlo, unsigned long long& slots) {
    if (ybase >= 0 && ybase + 9 < H) {  // (ybase is even)
      rlo = ybase >> 1;
      slots = kRegularSlots;
    } else {
      u8_rows(ybase, rlo, slots);
    }
  };
  auto fetch = [&](int s) {
    const int ybase = F0 + s * NR;
    if (UPS) {
      int rlo;
      unsigned long long slots;
      u8_rows_of(ybase, rlo, slots);
      if (tid < 5 * U8DW) {
        const int r = tid / U8DW, d = tid - r * U8DW;
        preU = *reinterpret_cast<const uint32_t*>(a.u8 + (size_t)(rlo + r) * uw + xsBase + 4 * d);
      }
      return;
    }
    const int y0r = mirror_row(ybase + 2 * wave), y1r = mirror_row(ybase + 2 * wave + 1);
    if (innerStrip) {
      preM0 = load_vec(y0r, cM);
      preM1 = load_vec(y1r, cM);
      if (hasE) {
        preE0 = load_vec(y0r, cE);
        preE1 = load_vec(y1r, cE);
      }
    } else {
      const float* r0 = a.in + (size_t)y0r * W;
      const float* r1 = a.in + (size_t)y1r * W;
      preM0 = load_chunk(r0, gxM);
      preM1 = load_chunk(r1, gxM);
      if (hasE) {
        preE0 = load_chunk(r0, gxE);
        preE1 = load_chunk(r1, gxE);
      }
    }
  };
  auto stage_u8 = [&]() {
    if (tid < 5 * U8DW) s_u8[tid] = preU;
  };
  // phase A of a step: the staged rows of level a
  auto stage_a = [&](int s) {
    if (!UPS) {
      s_inA4[2 * wave][lane] = preM0;
      s_inA4[2 * wave + 1][lane] = preM1;
      if (hasE) {
        s_inA4[2 * wave][64 + lane] = preE0;
        s_inA4[2 * wave + 1][64 + lane] = preE1;
      }
      return;
    }
    const int ybase = F0 + s * NR;
    int rlo;
    unsigned long long slots;
    u8_rows_of(ybase, rlo, slots);
    const uint8_t* s8 = reinterpret_cast<const uint8_t*>(s_u8);
    // row sums p[r][xm] + p[r][xp'] of the five staged rows, for this thread's column(s); an upsampled pixel is
    // 0.25 * (sum of its two source rows' sums): the exact integer form of upsample_at (see k_upsample2x_u8x4)
    // (named scalars: as arrays, indexed through the selects below, the ten sums were promoted to LDS)
    struct R5 { uint32_t r0, r1, r2, r3, r4; };
    auto sums = [&](int bm, int bp) {
      R5 v;
      v.r0 = (uint32_t)s8[0 * U8ROWB + bm] + (uint32_t)s8[0 * U8ROWB + bp];
      v.r1 = (uint32_t)s8[1 * U8ROWB + bm] + (uint32_t)s8[1 * U8ROWB + bp];
      v.r2 = (uint32_t)s8[2 * U8ROWB + bm] + (uint32_t)s8[2 * U8ROWB + bp];
      v.r3 = (uint32_t)s8[3 * U8ROWB + bm] + (uint32_t)s8[3 * U8ROWB + bp];
      v.r4 = (uint32_t)s8[4 * U8ROWB + bm] + (uint32_t)s8[4 * U8ROWB + bp];
      return v;
    };
    auto pick = [](const R5 rs, unsigned slot) {  // slot is wave-uniform
      uint32_t v = rs.r0;
      v = slot == 1 ? rs.r1 : v;
      v = slot == 2 ? rs.r2 : v;
      v = slot == 3 ? rs.r3 : v;
      return slot == 4 ? rs.r4 : v;
    };
    const bool second = tid < SWA - 256;  // (wave 0, lanes 0..15)
    const R5 a0 = sums(bm0, bp0);
    R5 a1 = a0;
    if (second) a1 = sums(bm1, bp1);
    // away from the top and bottom of the image the slot pattern is fixed (rows 2 m, 2 m + 1 use source rows (m, m), (m, m + 1));
    // at the border the sums are picked by wave-uniform selects
    if (slots == kRegularSlots) {
      const uint32_t e0[NR] = {2 * a0.r0, a0.r0 + a0.r1, 2 * a0.r1, a0.r1 + a0.r2, 2 * a0.r2, a0.r2 + a0.r3, 2 * a0.r3, a0.r3 + a0.r4};
      const uint32_t e1[NR] = {2 * a1.r0, a1.r0 + a1.r1, 2 * a1.r1, a1.r1 + a1.r2, 2 * a1.r2, a1.r2 + a1.r3, 2 * a1.r3, a1.r3 + a1.r4};
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        s_inA[i * SWA + tid] = (float)e0[i] * 0.25f;
        if (second) s_inA[i * SWA + 256 + tid] = (float)e1[i] * 0.25f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const unsigned sm = (unsigned)(slots >> (8 * i)) & 15u, sp = (unsigned)(slots >> (8 * i + 4)) & 15u;
        s_inA[i * SWA + tid] = (float)(pick(a0, sm) + pick(a0, sp)) * 0.25f;
        if (second) s_inA[i * SWA + 256 + tid] = (float)(pick(a1, sm) + pick(a1, sp)) * 0.25f;
      }
    }
  };

  // ---- level b's view of level a at the image border: the thread that owns column x of a tile also writes the slots of the
  // columns whose mirror image x is (x' = -1 - x left of the image, 2 W - 1 - x right of it), when they lie in this strip
  const int xA = xa0 + tid;                      // this thread's column of level a
  const bool colIn = xA >= 0 && xA < W;
  const bool ownCol = colIn && tid >= RB && tid < RB + TWB;  // (columns this block stores; the halo columns are a neighbour's)
  int dup = -1;
  if (colIn && xA < RB) dup = (-1 - xA) - xa0;
  if (colIn && xA >= W - RB) dup = (2 * W - 1 - xA) - xa0;
  if (dup < 0 || dup >= TWA) dup = -1;
  const int xB = xb0 + tid;                      // this thread's column of level b (tid < TWB)
  const bool colB = tid < TWB && xB < W;

  float winA[WINA], winB[WINB];
#pragma unroll
  for (int k = 0; k < WINA; ++k) winA[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < WINB; ++k) winB[k] = 0.0f;
  float mnA = FLT_MAX, mxA = -FLT_MAX, mnB = FLT_MAX, mxB = -FLT_MAX;

  // Every step runs both levels' passes; what a level has no use for yet (level b before its first tile exists, level a
  // behind its last one) is arithmetic on clamped rows whose results are not stored -- cheaper than the branches and the
  // register copies at their joins (the first edition of this loop had 150 v_mov per step for 28 window moves).
  fetch(0);
  if (UPS) {
    stage_u8();
    __syncthreads();
    fetch(1);
  }
  for (int s = 0; s < steps; ++s) {
    const int q = s - 3;                   // level b's step
    // ---- phase A: stage level a's input rows of this step
    stage_a(s);
    if (!UPS) fetch(s + 1);
    __syncthreads();
    // ---- phase H
    if (UPS) {
      stage_u8();                          // the u8 rows of step s + 1 (requested a step ago) ...
      fetch(s + 2);                        // ... and the request for step s + 2
    }
    {
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = 0.0f;
#pragma unroll
      for (int qq = 0; qq < HQ; ++qq) {
        const float4 v4 = s_inA4[hr][hq + qq];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = 4 * qq + j - (RP - RA) - i;
            if (k >= 0 && k <= 2 * RA) o[i] = __builtin_fmaf(v[j], wa[k <= RA ? k : 2 * RA - k], o[i]);
          }
        }
      }
      s_hA4[hr][hq] = make_float4(o[0], o[1], o[2], o[3]);
      s_hA4[hr][hq + 1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    if (hg < TWB / 8) {
      // the tile of level a this step reads: virtual rows v .. v + 7; outside the image it is the border tile backwards
      int v = y0 - 8 + 8 * q;
      v = v < -8 ? -8 : (v > H ? H : v);   // (steps in front of level b's first: any tile)
      const bool rev = v < 0 || v >= H;
      const int tile = v < 0 ? 0 : (v >= H ? (H - 8 - A0) / 8 : (v - A0) / 8);
      const float4* row4 = &s_inB4[tile & 1][rev ? NR - 1 - hr : hr][0];
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = 0.0f;
#pragma unroll
      for (int qq = 0; qq < HQ; ++qq) {
        const float4 v4 = row4[hq + qq];
        const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = 4 * qq + j - i;  // (RP == RB)
            if (k >= 0 && k <= 2 * RB) o[i] = __builtin_fmaf(vv[j], wb[k <= RB ? k : 2 * RB - k], o[i]);
          }
        }
      }
      s_hB4[hr][hq] = make_float4(o[0], o[1], o[2], o[3]);
      s_hB4[hr][hq + 1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    // ---- phase V
    {
#pragma unroll
      for (int i = 0; i < NR; ++i) winA[2 * RA + i] = s_hA[i * TWA + tid];
      float vs[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) vs[i] = 0.0f;
#pragma unroll
      for (int k = 0; k <= 2 * RA; ++k) {
#pragma unroll
        for (int i = 0; i < NR; ++i) vs[i] = __builtin_fmaf(winA[i + k], wa[k <= RA ? k : 2 * RA - k], vs[i]);
      }
      const int tile = s - LAG;                // level a emits tile s - 2 in steps 2 .. nt + 1
      const bool emit = tile >= 0 && tile < nt;
      float* tb = s_inB + (size_t)(tile & 1) * NR * TWA;
      if (emit && colIn) {                     // (a column outside the image: its slot belongs to the thread whose mirror image it is)
#pragma unroll
        for (int i = 0; i < NR; ++i) tb[i * TWA + tid] = vs[i];
      }
      if (emit && dup >= 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) tb[i * TWA + dup] = vs[i];
      }
      const int ar = A0 + 8 * tile;            // the tile's first row; this block stores the rows y0 .. y0 + nrows - 1
      if (emit && ownCol && ar >= y0 && ar < y0 + nrows) {
        float* orow = a.outA + (size_t)ar * W + xA;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          orow[(size_t)i * W] = vs[i];
          mnA = fminf(mnA, vs[i]);
          mxA = fmaxf(mxA, vs[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2 * RA; ++k) winA[k] = winA[k + NR];
    }
    {
      if (tid < TWB) {
#pragma unroll
        for (int i = 0; i < NR; ++i) winB[2 * RB + i] = s_hB[i * TWB + tid];
      }
      float vs[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) vs[i] = 0.0f;
#pragma unroll
      for (int k = 0; k <= 2 * RB; ++k) {
#pragma unroll
        for (int i = 0; i < NR; ++i) vs[i] = __builtin_fmaf(winB[i + k], wb[k <= RB ? k : 2 * RB - k], vs[i]);
      }
      if (q >= 2 && q < nq && colB) {
        float* orow = a.outB + (size_t)(y0 + 8 * (q - 2)) * W + xB;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          orow[(size_t)i * W] = vs[i];
          mnB = fminf(mnB, vs[i]);
          mxB = fmaxf(mxB, vs[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2 * RB; ++k) winB[k] = winB[k + NR];
    }
    // (no barrier here: phase A of the next step writes s_inA, last read in this step's phase H, and reads s_u8, written in
    // this step's phase H, both in front of the barrier above; the H buffers and the level-a tile are protected by the
    // barrier behind phase A)
  }
  if (a.minmaxA) block_minmax_commit(mnA, mxA, a.minmaxA, s_hA);
  if (a.minmaxB) block_minmax_commit(mnB, mxB, a.minmaxB, s_hA);
}

// Whether the pair kernel serves levels 0 + 1 of a w x h octave: 13 + 17 taps, sizes that are multiples of 8 (row tiles, u8
// rows of whole dwords), wide enough that a mirrored column lies in the strip that reads it, 32-bit element offsets.
bool pair_usable(uint32_t w, uint32_t h, int taps0, int taps1, const float* in, const float* outA, const float* outB) {
  const bool off = svdev::sw().noGaussPair || svdev::sw().gaussValu || svdev::sw().gaussMfma;
  return !off && taps0 == 13 && taps1 == 17 && (w & 7) == 0 && (h & 7) == 0 && w >= 512 && h >= 64 &&
         (uint64_t)w * h < ((uint64_t)1 << 31) && (reinterpret_cast<size_t>(in) & 15) == 0 && (reinterpret_cast<size_t>(outA) & 3) == 0 &&
         (reinterpret_cast<size_t>(outB) & 3) == 0;
}

// levels a (13 taps, weights wA) and b (17 taps, wB) of one octave; u8src != nullptr: level a's input is the 2x upsample of it
int launch_pair(const float* in, const uint8_t* u8src, float* outA, float* outB, uint32_t w, uint32_t h, const float* wA, const float* wB,
                float* minmaxA, float* minmaxB, hipStream_t st) {
  PairArgs p;
  p.in = in;
  p.u8 = u8src;
  p.outA = outA;
  p.outB = outB;
  p.minmaxA = minmaxA;
  p.minmaxB = minmaxB;
  p.w = w;
  p.h = h;
  for (int k = 0; k <= 6; ++k) {
    if (wA[k] != wA[12 - k]) return SSRLCV_ERR_UNSUPPORTED;
    p.wgtA[k] = wA[k];
  }
  p.wgtA[7] = p.wgtA[8] = 0.0f;
  for (int k = 0; k <= 8; ++k) {
    if (wB[k] != wB[16 - k]) return SSRLCV_ERR_UNSUPPORTED;
    p.wgtB[k] = wB[k];
  }
#ifdef SSRLCV_STAMPS
  p.stamps = nullptr;
#endif
  // rows per block: ONE round of resident blocks (as many per CU as the occupancy query grants; a grid two blocks larger
  // than that ran twice as long), never below 64 rows (a block spends five steps of eight rows filling its two windows)
  static int cus = 0, perCu[2] = {0, 0};
  if (!cus) {
    int dev = 0;
    SSRLCV_HIP_TRY(hipGetDevice(&dev));
    SSRLCV_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu[0], (const void*)k_gauss_pair<6, false>, 256, 0) != hipSuccess || perCu[0] < 1) perCu[0] = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu[1], (const void*)k_gauss_pair<6, true>, 256, 0) != hipSuccess || perCu[1] < 1) perCu[1] = 1;
  }
  const int rowsForced = svdev::sw().pairRows;
  const uint32_t strips = (w + 239) / 240;
  uint32_t by = (uint32_t)(perCu[u8src ? 1 : 0] * cus) / strips;
  by = by < 1 ? 1 : by;
  uint32_t rows = (h + by - 1) / by;
  rows = rows < 64 ? 64 : rows;
  if (rowsForced > 0) rows = (uint32_t)rowsForced;
  rows = (rows + 7) / 8 * 8;
  p.rowsPerBlock = rows;
  const dim3 grid(strips, (h + rows - 1) / rows);
  if (u8src) hipLaunchKernelGGL((k_gauss_pair<6, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((k_gauss_pair<6, false>), grid, dim3(256), 0, st, p);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}
