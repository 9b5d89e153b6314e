// ssrlcv_amd/csrc/gauss_pair_rm.inc -- levels 0 and 1 of an octave (13 + 17 taps) in ONE launch on the f32 matrix pipe (round 6).
// Included by pyramid.hip behind gauss_rm.inc and gauss_pair.inc (shares PairArgs, the LDS helpers, rm_phys, rm_static_for).
//
// Why: the floor table of round 6 (profiles/r06_pyramid_floor.json) shows levels 1-3 of octave 0 AT the copy floor of the
// bytes they move and level 0 (u8 source, 268 MB written) at twice its floor -- the first 260 us of every image are two
// launches that move 285 + 537 MB where 17 + 268 + 268 have to move.  The vector formulation of the fused pair
// (k_gauss_pair) is bound by its 480 FMAs per thread and step (236-268 us against 235-255 for the two launches); here both
// levels run as register-marching products on v_mfma_f32_4x4x1 (gauss_rm.inc: a chain of them per output is the reference's
// `sum += pixel * weight` chain in tap order), 72 MFMA slots per pixel against 60 vector FMAs at a third of their issue cost.
//
// Structure = two k_gauss_rm engines in one block of four waves, 16 rows per step:
//   engine A (level a, R = 6: K = 16 MFMAs per group of four outputs) on the 256 columns level b's 240 need;
//   engine B (level b, R = 8: K = 20) on the block's 240 columns; both rings have 8 slots, so the step loop is unrolled twice.
//   phase H: horizontal pass of A on the rows this wave staged itself + horizontal pass of B on the level-a tile in LDS
//   phase V: vertical pass of A -- a completed group of four rows goes to global memory (the columns / rows this block
//            owns) and into the level-a tile in LDS, laid out as engine B's row stage -- + vertical pass of B.
// Level a's march starts RA rows above level b's first input row, which makes its K = 16 = one step of warm-up: the
// groups stored during step s are exactly tile s - 1 (virtual rows y0 - 8 + 16 (s - 1) .. + 15), and engine B's horizontal
// pass reads tile s - 2 in step s.  The mirror of level b's reads (getSymmetrizedCoord) is made in the tile: a column
// outside the image is written by the lane that owns its mirror image, and in the tile that straddles the top (bottom) of
// the image the eight real rows at positions p are also written at positions 15 - p -- RB = 8 = half a tile makes the
// mirrored rows the other half of the same tile.  A chunk of four input columns outside the image is the chunk of its
// mirror image loaded whole and reversed in registers (strips start on multiples of 4: a chunk is inside or outside as a
// whole).  Bit-identical to the two launches (tools/gauss_pair_lab.hip, tests/test_gpu_sift.py).
struct PairRm {
  static constexpr int RA = 6, RB = 8, RP = 8, TWA = 256, TWB = 240, STEP = 16;
  static constexpr int KA = 4 + 2 * RA, KB = 4 + 2 * RB, GA = KA / 4, GB = KB / 4, GP = 8, P = GP / 4;
  static constexpr int T = (16 + 2 * RP) / 4;  // 16-byte sample reads per signal and step (both engines stage a halo of 8)
  // row strides (floats): the two row stages in gauss_rm.inc's layout (16-column chunks at a pitch of 20, stride a multiple
  // of 64: conflict-free 16-byte reads), the two H buffers dense (their sixteen 16-byte writes per step take a 4-way
  // conflict; padded like gauss_rm.inc's the block would not fit twice into a CU's 160 KB)
  static constexpr int SROWA = 384, SROWB = 320, HROWA = 256, HROWB = 240;
  static constexpr int U8ROWS = 9, U8DW = 36, U8ROWB = U8DW * 4;
  static constexpr size_t floatBytes = sizeof(float) * (size_t)STEP * (SROWA + HROWA + SROWB + HROWB);
  static constexpr size_t ldsBytes = floatBytes + 1536 /* nine u8 rows */ + 1024 /* stores that go nowhere */;
  static_assert(GP > GA && GP > GB && 2 * ldsBytes <= 163840, "two blocks per CU");
};

#ifndef SSRLCV_PAIR_OPT
#define SSRLCV_PAIR_OPT 1  // bit 0: swizzled H buffers (default: 204 against 212 us); 8: stores / tile rows / min-max of a step in batches; 16: H rows in one batch -- all exact, neither 8 nor 16 faster; a late start of a SIMD's second wave slot and one block per CU were measured too and are gone (profiles/r06_kernel_ab.txt section 5)
#endif
// Engine B's vertical pass with the MFMA's operands exchanged (see gauss_rm.inc, SSRLCV_RM_TRANSPOSED): a lane holds four columns of
// one output row and a completed group leaves in one 16-byte store per lane.  (Engine A keeps rows in its registers: its groups also
// go to the level-a tile, column by column.)  -DSSRLCV_PAIR_B_TRANSPOSED=0: four 4-byte stores per group.
#ifndef SSRLCV_PAIR_B_TRANSPOSED
#define SSRLCV_PAIR_B_TRANSPOSED 1
#endif
#ifdef SSRLCV_TIMING_VARIANT  // tools/ lab builds only (dev_switch.h): bits leave work out to time what remains -- results invalid
#define PAIR_TV(bit) ((SSRLCV_TIMING_VARIANT & (bit)) != 0)
#else
#define PAIR_TV(bit) false
#endif
template <bool UPS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_gauss_pair_rm(PairArgs a) {
  using C = PairRm;
  constexpr int RA = C::RA, RB = C::RB, RP = C::RP, TWA = C::TWA, TWB = C::TWB, STEP = C::STEP;
  constexpr int KA = C::KA, KB = C::KB, GA = C::GA, GB = C::GB, GP = C::GP, P = C::P, T = C::T;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int W = (int)a.w, H = (int)a.h;
  const int xb0 = blockIdx.x * TWB, xa0 = xb0 - RB;
  const int y0 = blockIdx.y * (int)a.rowsPerBlock;
  int nrows = (int)a.rowsPerBlock;
  if (y0 + nrows > H) nrows = H - y0;                 // (H and rowsPerBlock are multiples of 16)
  const int T0 = y0 - RB;                             // level b's first input row = first row of level-a tile 0
  const int nb = nrows / STEP;
  const bool top = y0 == 0, bottom = y0 + nrows >= H;
  const int steps = (nb + 4 + P - 1) / P * P;         // B's last group is stored in step nb + 3
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  float Aa[KA], Ab[KB];
#pragma unroll
  for (int m = 0; m < KA; ++m) {
    const int t = m - (lane & 3), ti = t <= RA ? t : 2 * RA - t;
    Aa[m] = (t >= 0 && t <= 2 * RA) ? a.wgtA[ti < 0 ? 0 : ti] : 0.0f;
  }
#pragma unroll
  for (int m = 0; m < KB; ++m) {
    const int t = m - (lane & 3), ti = t <= RB ? t : 2 * RB - t;
    Ab[m] = (t >= 0 && t <= 2 * RB) ? a.wgtB[ti < 0 ? 0 : ti] : 0.0f;
  }
#pragma unroll
  for (int m = 0; m < KA; ++m) asm volatile("" : "+v"(Aa[m]));
#pragma unroll
  for (int m = 0; m < KB; ++m) asm volatile("" : "+v"(Ab[m]));

  // ---- LDS byte addresses (per-lane constants)
  const unsigned stageA = lds_addr(s_mem), hbufA = stageA + (unsigned)(STEP * C::SROWA) * 4u;
  const unsigned stageB = hbufA + (unsigned)(STEP * C::HROWA) * 4u, hbufB = stageB + (unsigned)(STEP * C::SROWB) * 4u;
  const unsigned u8st = hbufB + (unsigned)(STEP * C::HROWB) * 4u, nowhere = u8st + 1536u;
  const int hrow = 4 * wave + (lane >> 4), hseg = lane & 15;
  const unsigned sWM = stageA + (unsigned)((4 * wave) * C::SROWA + rm_phys(4 * lane)) * 4u;              // chunk `lane` of rows 4 wave ..
  const unsigned sWE = stageA + (unsigned)((4 * wave + ((lane >> 2) & 3)) * C::SROWA + rm_phys(256 + 4 * (lane & 3))) * 4u;  // lanes 0..15: chunk 64 + (lane & 3) of row lane >> 2
  const unsigned hRA = stageA + (unsigned)(hrow * C::SROWA + 20 * hseg) * 4u;
  // H buffers: dense rows; the four 16-byte chunks of a 16-column segment are stored at chunk g ^ ((segment >> 1) & 3), which
  // spreads the eight lanes of a 16-byte store over eight different 16-byte slots of a 128-byte bank window (dense and
  // unswizzled they met in two: a 4-way conflict on every store, 24 us of the kernel's 213: profiles/r06_kernel_ab.txt)
  const unsigned swz = (SSRLCV_PAIR_OPT & 1) ? (unsigned)((hseg >> 1) & 3) : 0u;
  const unsigned hWA = hbufA + (unsigned)(hrow * C::HROWA + 16 * hseg) * 4u;
  unsigned hWAg[4], hWBg[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) hWAg[g] = hWA + 16u * ((unsigned)g ^ swz);
  auto hcol = [](int c) { return (SSRLCV_PAIR_OPT & 1) ? (c & ~15) + 4 * (((c >> 2) & 3) ^ ((c >> 5) & 3)) + (c & 3) : c; };  // column -> its place in a swizzled H row
  const unsigned vRA = hbufA + (unsigned)hcol(64 * wave + lane) * 4u;
  const unsigned hRB = stageB + (unsigned)(hrow * C::SROWB + 20 * hseg) * 4u;
  const unsigned hWB = hbufB + (unsigned)(hrow * C::HROWB + 16 * hseg) * 4u;
#pragma unroll
  for (int g = 0; g < 4; ++g) hWBg[g] = hseg < TWB / 16 ? hWB + 16u * ((unsigned)g ^ swz) : nowhere + 64u * (unsigned)(lane >> 4) + 16u * (unsigned)g;  // (segment 15 lies beyond level b's strip)
  const unsigned vRB = hbufB + (unsigned)hcol(64 * wave + lane) * 4u;
  // the level-a tile: this lane's column (the padding floats of the stage, never read, take what must not be written)
  const int ca = 64 * wave + lane, xA = xa0 + ca;
  const bool colIn = xA >= 0 && xA < W;
  const unsigned pad = stageB + (unsigned)(20 * (lane & 15) + 16 + (lane >> 4)) * 4u;
  const unsigned tW = colIn ? stageB + (unsigned)rm_phys(ca) * 4u : pad;
  int dupc = -1;
  if (colIn && xA < RB) dupc = (-1 - xA) - xa0;
  if (colIn && xA >= W - RB) dupc = (2 * W - 1 - xA) - xa0;
  if (dupc < 0 || dupc >= TWA) dupc = -1;
  const unsigned tD = dupc >= 0 ? stageB + (unsigned)rm_phys(dupc) * 4u : pad;
  const bool anyDup = __any(dupc >= 0);               // (wave-uniform: only waves at the image's left / right border)
  const bool ownA = colIn && ca >= RB && ca < RB + TWB;
  const int xB = xb0 + ca;
  const bool colB = ca < TWB && xB < W;
  const __amdgpu_buffer_rsrc_t routA = __builtin_amdgcn_make_buffer_rsrc((void*)a.outA, 0, (int)((uint32_t)W * (uint32_t)H * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t routB = __builtin_amdgcn_make_buffer_rsrc((void*)a.outB, 0, (int)((uint32_t)W * (uint32_t)H * 4u), 0x00020000);
  constexpr bool TRB = SSRLCV_PAIR_B_TRANSPOSED != 0;
  // (transposed engine B: this lane's results are row (lane & 3) of a group, columns 64 wave + 4 (lane >> 2) .. + 3 of the strip --
  // inside or outside level b's strip and the image as a whole: TWB, xb0 and W are multiples of four)
  const int cb4 = 64 * wave + 4 * (lane >> 2);
  const bool colB4 = cb4 < TWB && xb0 + cb4 < W;
  const bool ownB = TRB ? colB4 : colB;
  const int vOutA = ownA ? xA * 4 : 0x7ffffff0;
  const int vOutB = TRB ? (colB4 ? ((xb0 + cb4) + (lane & 3) * W) * 4 : 0x7ffffff0) : (colB ? xB * 4 : 0x7ffffff0);

  // ---- engine A's loader.  This wave stages rows 4 wave .. + 3 of every step: every lane chunk `lane` (columns xa0 - 8 + 4 lane ..)
  // of the four rows, and lanes 0..15 one of the sixteen chunks 64..67 (row lane >> 2, chunk 64 + (lane & 3)): five requests /
  // conversions per lane and step, not eight.  A chunk outside the image is its mirror image's chunk, reversed (only the
  // waves that have such a chunk run the selects: anyRev).
  auto chunk_src = [&](int x0c, bool& rev) {
    rev = x0c < 0 || x0c >= W;
    int c = x0c < 0 ? -x0c - 4 : (x0c >= W ? 2 * W - x0c - 4 : x0c);
    c = c < 0 ? 0 : (c > W - 4 ? W - 4 : c);
    return c;
  };
  bool revM, revE;
  const int csM = chunk_src(xa0 - RP + 4 * lane, revM), csE = chunk_src(xa0 - RP + 4 * (64 + (lane & 3)), revE);
  const bool hasE = lane < 16;
  const int rowE = (lane >> 2) & 3;                   // the row (of the wave's four) of this lane's extra chunk
  const bool anyRev = __any(revM || (hasE && revE));
  const int F0 = T0 - RA;                             // first input row engine A feeds
  auto mirror_row = [&](int y) {                      // wave-uniform
    y = y > H - 1 + RP ? H - 1 + RP : y;
    y = y < -2 * RP ? -2 * RP : y;
    y = y < 0 ? -1 - y : y;
    return y > H - 1 ? 2 * H - 1 - y : y;
  };
  // float source
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, UPS ? 0 : (int)((uint32_t)W * (uint32_t)H * 4u), 0x00020000);
  u32x4 preI[4], preE;
  auto fetch = [&](int s) __attribute__((always_inline)) {
    const int ybase = F0 + s * STEP + 4 * wave;
    unsigned soff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) soff[k] = (unsigned)mirror_row(ybase + k) * (unsigned)W * 4u;
#pragma unroll
    for (int k = 0; k < 4; ++k) preI[k] = __builtin_amdgcn_raw_buffer_load_b128(rin, csM * 4, (int)soff[k], 0);
    if (hasE) {  // (per-lane row: the row offset goes into the vector offset)
      const unsigned so = rowE == 0 ? soff[0] : rowE == 1 ? soff[1] : rowE == 2 ? soff[2] : soff[3];
      preE = __builtin_amdgcn_raw_buffer_load_b128(rin, (int)(so + (unsigned)csE * 4u), 0, 0);
    }
  };
  auto put_chunk = [&](unsigned addr, f32x4 v, bool rev) __attribute__((always_inline)) {
    if (anyRev) {  // (wave-uniform)
      const f32x4 r = f32x4{v[3], v[2], v[1], v[0]};
      v = rev ? r : v;
    }
    lds_st4(addr, v);
  };
  auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) put_chunk(sWM + (unsigned)(k * C::SROWA) * 4u, __builtin_bit_cast(f32x4, preI[k]), revM);
    if (hasE) put_chunk(sWE, __builtin_bit_cast(f32x4, preE), revE);
  };
  // u8 source (S1 + S2 in the loader): the nine u8 rows a step's sixteen upsampled rows are made of go through LDS (one or two
  // 4-byte loads per thread and step); a chunk of four upsampled pixels is made of source bytes 2c, 2c + 1, 2c + 2 of two rows:
  // 0.25 * {2 a0, a0 + a1, 2 a1, a1 + a2}, a_j = the two rows' sum of byte j -- the exact integer form of upsample_at
  // (k_upsample2x_u8x4); byte 2c + 2 of the image's last chunk is its byte 2c + 1 (upsample_at clamps xp).
  const int uw = W >> 1, uh = H >> 1;
  int xsBase = (xa0 - RP) >> 1;
  xsBase = xsBase > uw - C::U8ROWB ? uw - C::U8ROWB : xsBase;
  xsBase = xsBase < 0 ? 0 : xsBase;
  xsBase &= ~3;
  const unsigned bM = u8st + (unsigned)((csM >> 1) - xsBase), bE = u8st + (unsigned)((csE >> 1) - xsBase);
  const bool lastM = csM == W - 4, lastE = csE == W - 4;
  uint32_t preU0 = 0, preU1 = 0;
  constexpr unsigned long long kRegLo = 0x4333322221111000ull, kRegHi = 0x8777766665555444ull;  // slots of rows 0-7 / 8-15 away from the border
  auto u8_rows = [&](int ybase, int& rlo, unsigned long long& lo, unsigned long long& hi) __attribute__((always_inline)) {
    if (ybase >= 0 && ybase + 17 < H) {  // (ybase is even)
      rlo = ybase >> 1;
      lo = kRegLo;
      hi = kRegHi;
      return;
    }
    int ym[STEP], yp[STEP];
    rlo = 1 << 30;
#pragma unroll
    for (int i = 0; i < STEP; ++i) {
      const int Y = mirror_row(ybase + i);
      ym[i] = Y >> 1;
      yp[i] = (Y & 1) ? (ym[i] + 1 < uh ? ym[i] + 1 : uh - 1) : ym[i];
      rlo = ym[i] < rlo ? ym[i] : rlo;
    }
    rlo = rlo > uh - C::U8ROWS ? uh - C::U8ROWS : rlo;
    lo = hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      lo |= (unsigned long long)((ym[i] - rlo) | ((yp[i] - rlo) << 4)) << (8 * i);
      hi |= (unsigned long long)((ym[i + 8] - rlo) | ((yp[i + 8] - rlo) << 4)) << (8 * i);
    }
  };
  auto u8_fetch = [&](int s) __attribute__((always_inline)) {
    int rlo;
    unsigned long long lo, hi;
    u8_rows(F0 + s * STEP, rlo, lo, hi);
    {
      const int r = tid / C::U8DW, d = tid - r * C::U8DW;
      preU0 = *reinterpret_cast<const uint32_t*>(a.u8 + (size_t)(rlo + r) * uw + xsBase + 4 * d);
    }
    if (tid < C::U8ROWS * C::U8DW - 256) {
      const int t2 = tid + 256, r = t2 / C::U8DW, d = t2 - r * C::U8DW;
      preU1 = *reinterpret_cast<const uint32_t*>(a.u8 + (size_t)(rlo + r) * uw + xsBase + 4 * d);
    }
  };
  auto u8_write = [&]() __attribute__((always_inline)) {
    *(__attribute__((address_space(3))) uint32_t*)(size_t)(u8st + 4u * (unsigned)tid) = preU0;
    if (tid < C::U8ROWS * C::U8DW - 256) *(__attribute__((address_space(3))) uint32_t*)(size_t)(u8st + 4u * (unsigned)(tid + 256)) = preU1;
  };
  auto ld_u16 = [](unsigned addr) { return (uint32_t)*(const __attribute__((address_space(3))) uint16_t*)(size_t)addr; };
  auto ld_u8 = [](unsigned addr) { return (uint32_t)*(const __attribute__((address_space(3))) uint8_t*)(size_t)addr; };
  auto up_chunk = [&](uint32_t pm, uint32_t qm, uint32_t pp, uint32_t qp, bool last) __attribute__((always_inline)) {
    const uint32_t a0 = (pm & 255u) + (pp & 255u), a1 = (pm >> 8) + (pp >> 8);
    const uint32_t a2 = last ? a1 : qm + qp;
    return f32x4{(float)(2 * a0) * 0.25f, (float)(a0 + a1) * 0.25f, (float)(2 * a1) * 0.25f, (float)(a1 + a2) * 0.25f};
  };
  // the rows 4 wave .. + 3 of step s from the u8 rows in LDS
  auto u8_convert = [&](int s) __attribute__((always_inline)) {
    int rlo;
    unsigned long long lo, hi;
    u8_rows(F0 + s * STEP, rlo, lo, hi);
    const unsigned long long word = (wave & 2) ? hi : lo;
    const unsigned sl = (unsigned)(word >> (32 * (wave & 1)));  // rows 4 wave .. + 3: a byte each, slot of ym | slot of yp' << 4
    if (lo == kRegLo && hi == kRegHi) {
      // regular: rows 4w + {0, 1, 2, 3} use the source slots (2w, 2w), (2w, 2w + 1), (2w + 1, 2w + 1), (2w + 1, 2w + 2)
      const unsigned b0 = (unsigned)(2 * wave) * (unsigned)C::U8ROWB;
      uint32_t p[3], q[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        p[j] = ld_u16(bM + b0 + (unsigned)(j * C::U8ROWB));
        q[j] = ld_u8(bM + b0 + (unsigned)(j * C::U8ROWB) + 2u);
      }
      put_chunk(sWM, up_chunk(p[0], q[0], p[0], q[0], lastM), revM);
      put_chunk(sWM + (unsigned)(1 * C::SROWA) * 4u, up_chunk(p[0], q[0], p[1], q[1], lastM), revM);
      put_chunk(sWM + (unsigned)(2 * C::SROWA) * 4u, up_chunk(p[1], q[1], p[1], q[1], lastM), revM);
      put_chunk(sWM + (unsigned)(3 * C::SROWA) * 4u, up_chunk(p[1], q[1], p[2], q[2], lastM), revM);
      if (hasE) {  // this lane's one extra chunk: row 4 wave + rowE uses the slots 2 wave + (rowE >> 1) and + (rowE & 1) more
        const unsigned bs = bE + b0 + (unsigned)(rowE >> 1) * (unsigned)C::U8ROWB, bp = bs + (unsigned)(rowE & 1) * (unsigned)C::U8ROWB;
        put_chunk(sWE, up_chunk(ld_u16(bs), ld_u8(bs + 2u), ld_u16(bp), ld_u8(bp + 2u), lastE), revE);
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // a step at the top or bottom of the image: slots by wave-uniform offsets
      const unsigned om = ((sl >> (8 * k)) & 15u) * (unsigned)C::U8ROWB, op = ((sl >> (8 * k + 4)) & 15u) * (unsigned)C::U8ROWB;
      put_chunk(sWM + (unsigned)(k * C::SROWA) * 4u, up_chunk(ld_u16(bM + om), ld_u8(bM + om + 2u), ld_u16(bM + op), ld_u8(bM + op + 2u), lastM), revM);
    }
    if (hasE) {
      const unsigned byteE = (sl >> (8 * rowE)) & 255u;  // (per-lane row: a vector shift)
      const unsigned om = (byteE & 15u) * (unsigned)C::U8ROWB, op = (byteE >> 4) * (unsigned)C::U8ROWB;
      put_chunk(sWE, up_chunk(ld_u16(bE + om), ld_u8(bE + om + 2u), ld_u16(bE + op), ld_u8(bE + op + 2u), lastE), revE);
    }
  };

  // ---- state of the two vertical passes
  f32x4 accA[GP], accB[GP];
#pragma unroll
  for (int g = 0; g < GP; ++g) accA[g] = accB[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float mnA = FLT_MAX, mxA = -FLT_MAX, mnB = FLT_MAX, mxB = -FLT_MAX;
  auto minmax4 = [](float& mn, float& mx, const f32x4& v) __attribute__((always_inline)) {
    mn = __builtin_fminf(__builtin_fminf(mn, v[0]), v[1]);
    mn = __builtin_fminf(__builtin_fminf(mn, v[2]), v[3]);
    mx = __builtin_fmaxf(__builtin_fmaxf(mx, v[0]), v[1]);
    mx = __builtin_fmaxf(__builtin_fmaxf(mx, v[2]), v[3]);
  };
  auto rdoff = [](int t) { return (unsigned)(4 * t + (t & ~3)) * 4u; };

  // ---- prologue: the staged rows of step 0, the request for step 1
  if (UPS) {
    u8_fetch(0);
    u8_write();
    __syncthreads();
    u8_convert(0);
    u8_fetch(1);
  } else {
    fetch(0);
    stage_write();
    fetch(1);
  }
  __syncthreads();

  auto step = [&](int s, auto pc) __attribute__((always_inline)) {
    constexpr int PH = decltype(pc)::value;  // s mod P
    const int it = s;
    (void)it;
    SV_STAMP(0);
    if (UPS && !PAIR_TV(16)) {  // the u8 rows of step s + 1 (requested a step ago; the rows of step s were converted in front of the last barrier) ...
      u8_write();
      u8_fetch(s + 2);  // ... and the request for step s + 2
    }
    // ---- phase H, engine A: rows 4 wave .. + 3 of step s (4 groups per signal, KA MFMAs each)
    {
      f32x4 hacc[4], rd[3];
      rd[0] = lds_ld4(hRA + rdoff(0));
      rd[1] = lds_ld4(hRA + rdoff(1));
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (t + 2 < T) rd[(t + 2) % 3] = lds_ld4(hRA + rdoff(t + 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int u = 4 * t + e - (RP - RA);
          if (u >= 0 && u < 16 + 2 * RA) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int m = u - 4 * g;
              if (m == 0) hacc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(Aa[0], rd[t % 3][e], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
              else if (m > 0 && m < KA) hacc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(Aa[m], rd[t % 3][e], hacc[g], 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
              if (!(SSRLCV_PAIR_OPT & 16) && (u - 4 * g == KA + 3 || (u == 16 + 2 * RA - 1 && u - 4 * g >= KA - 1 && u - 4 * g < KA + 3))) { if (!PAIR_TV(4)) lds_st4(hWAg[g], hacc[g]); else asm volatile("" :: "v"(hacc[g])); }
          }
        }
      }
      if (SSRLCV_PAIR_OPT & 16) {  // the four groups of the pass in one batch behind its MFMAs
#pragma unroll
        for (int g = 0; g < 4; ++g) lds_st4(hWAg[g], hacc[g]);
      }
    }
    SV_STAMP(1);
    // ---- phase H, engine B: rows 4 wave .. + 3 of level-a tile s - 2 (written by the vertical pass of step s - 1)
    {
      f32x4 hacc[4], rd[3];
      rd[0] = lds_ld4(hRB + rdoff(0));
      rd[1] = lds_ld4(hRB + rdoff(1));
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (t + 2 < T) rd[(t + 2) % 3] = lds_ld4(hRB + rdoff(t + 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int u = 4 * t + e;  // (RP == RB)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int m = u - 4 * g;
            if (m == 0) hacc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(Ab[0], rd[t % 3][e], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
            else if (m > 0 && m < KB) hacc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(Ab[m], rd[t % 3][e], hacc[g], 0, 0, 0);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (!(SSRLCV_PAIR_OPT & 16) && (u - 4 * g == KB + 3 || (u == 16 + 2 * RB - 1 && u - 4 * g >= KB - 1 && u - 4 * g < KB + 3))) { if (!PAIR_TV(4)) lds_st4(hWBg[g], hacc[g]); else asm volatile("" :: "v"(hacc[g])); }
        }
      }
      if (SSRLCV_PAIR_OPT & 16) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lds_st4(hWBg[g], hacc[g]);
      }
    }
    SV_STAMP(2);
    if (!PAIR_TV(64)) __syncthreads();  // both H buffers complete; the level-a tile and the row stage are free
    SV_STAMP(3);
    // ---- phase V
    float bvA[16], bvB[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bvA[r] = lds_ld(vRA + (unsigned)(r * C::HROWA) * 4u);
#pragma unroll
    for (int r = 0; r < 16; ++r) bvB[r] = lds_ld(vRB + (unsigned)(r * C::HROWB) * 4u);
    if (!PAIR_TV(16)) {
      if (UPS) {
        u8_convert(s + 1);
      } else {
        stage_write();
        fetch(s + 2);
      }
    }
    SV_STAMP(4);
    // Both engines: the group a quantum completes leaves one quantum later at the earliest -- its MFMAs have retired by then.
    // Where its rows go out (global store, level-a tile, min / max) is a schedule:
    //   default: the global store of row rho behind MFMA row rho of the following quantum (gauss_rm.inc's order), tile rows and
    //            min / max as a batch behind that quantum;
    //   SSRLCV_PAIR_OPT & 8: all of a step's groups in batches behind the MFMA quanta (engine A: one batch behind its four
    //            quanta; engine B, whose ring re-starts a slot three quanta after the group in it completed, two batches).
    // A vector instruction (and an LDS store, which reads its data like one) among MFMAs waits for a gap in BOTH waves'
    // MFMA streams on the SIMD: single ones between MFMA rows cost up to ~85 cycles each (SSRLCV_PAIR_OPT & 2 / 4:
    // profiles/r06_kernel_ab.txt), so everything that reads vector registers is batched.
    const bool dupRows = (top && s == 1) || (bottom && s == nb + 1);  // the tile that straddles the image's top / bottom edge
    auto quantumA = [&](auto qc, bool storeRows) __attribute__((always_inline)) {
      constexpr int qi = decltype(qc)::value;
      constexpr int PHI = 4 * PH + qi;
      constexpr int done = (PHI - GA + GP) % GP;
      const int v0 = T0 + STEP * (s - 1) + 4 * qi;   // the stored group's first row (uniform); a real row of the image?
      const bool mine = s >= 1 && v0 >= 0 && v0 < H && v0 >= y0 && v0 < y0 + nrows;
      const int voff = mine ? vOutA : 0x7ffffff0;
      const unsigned rowOff = mine ? (unsigned)v0 * (unsigned)W * 4u : 0u;
      rm_static_for<4>([&](auto rc) __attribute__((always_inline)) {
        constexpr int rho = decltype(rc)::value;
#pragma unroll
        for (int age = 0; age < GA; ++age) {
          const int slot = (PHI - age + GP) % GP;
          const int m = 4 * age + rho;
          if (m == 0) accA[slot] = __builtin_amdgcn_mfma_f32_4x4x1f32(Aa[0], bvA[4 * qi], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
          else accA[slot] = __builtin_amdgcn_mfma_f32_4x4x1f32(Aa[m], bvA[4 * qi + rho], accA[slot], 0, 0, 0);
        }
        if (storeRows && !PAIR_TV(1))
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)accA[done][rho]), routA, voff, (int)(rowOff + (unsigned)rho * (unsigned)W * 4u), 0);
      });
    };
    auto leaveA = [&](auto qc, bool storeRows) __attribute__((always_inline)) {  // rows of the group stored "during" quantum qi
      constexpr int qi = decltype(qc)::value;
      constexpr int PHI = 4 * PH + qi;
      constexpr int done = (PHI - GA + GP) % GP;
      constexpr int pos = 4 * qi;
      const int v0 = T0 + STEP * (s - 1) + 4 * qi;
      const bool real = s >= 1 && v0 >= 0 && v0 < H;
      const bool mine = real && v0 >= y0 && v0 < y0 + nrows;
      if (storeRows && !PAIR_TV(1)) {
        const int voff = mine ? vOutA : 0x7ffffff0;
        const unsigned rowOff = mine ? (unsigned)v0 * (unsigned)W * 4u : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)accA[done][i]), routA, voff, (int)(rowOff + (unsigned)i * (unsigned)W * 4u), 0);
      }
      if (real && !PAIR_TV(8)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_st(tW + (unsigned)((pos + i) * C::SROWB) * 4u, accA[done][i]);
        if (anyDup) {
#pragma unroll
          for (int i = 0; i < 4; ++i) lds_st(tD + (unsigned)((pos + i) * C::SROWB) * 4u, accA[done][i]);
        }
        if (dupRows) {
#pragma unroll
          for (int i = 0; i < 4; ++i) lds_st(tW + (unsigned)((15 - pos - i) * C::SROWB) * 4u, accA[done][i]);
          if (anyDup) {
#pragma unroll
            for (int i = 0; i < 4; ++i) lds_st(tD + (unsigned)((15 - pos - i) * C::SROWB) * 4u, accA[done][i]);
          }
        }
      }
      if (real) minmax4(mnA, mxA, accA[done]);
    };
    auto quantumB = [&](auto qc, bool storeRows) __attribute__((always_inline)) {
      constexpr int qi = decltype(qc)::value;
      constexpr int PHI = 4 * PH + qi;
      constexpr int done = (PHI - GB + GP) % GP;
      const int jrel = 4 * (4 * (s - 2) + qi - 1) - 2 * RB;
      const bool ok = jrel >= 0 && jrel < nrows;
      const int voff = ok ? vOutB : 0x7ffffff0;
      const unsigned rowOff = ok ? (unsigned)(y0 + jrel) * (unsigned)W * 4u : 0u;
      rm_static_for<4>([&](auto rc) __attribute__((always_inline)) {
        constexpr int rho = decltype(rc)::value;
#pragma unroll
        for (int age = 0; age < GB; ++age) {
          const int slot = (PHI - age + GP) % GP;
          const int m = 4 * age + rho;
          if (m == 0) accB[slot] = TRB ? __builtin_amdgcn_mfma_f32_4x4x1f32(bvB[4 * qi], Ab[0], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0)
                                       : __builtin_amdgcn_mfma_f32_4x4x1f32(Ab[0], bvB[4 * qi], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
          else accB[slot] = TRB ? __builtin_amdgcn_mfma_f32_4x4x1f32(bvB[4 * qi + rho], Ab[m], accB[slot], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_4x4x1f32(Ab[m], bvB[4 * qi + rho], accB[slot], 0, 0, 0);
        }
        if (storeRows && !PAIR_TV(2)) {
          if (TRB) {
            if (rho == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, accB[done]), routB, voff, (int)rowOff, 0);
          } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)accB[done][rho]), routB, voff, (int)(rowOff + (unsigned)rho * (unsigned)W * 4u), 0);
          }
        }
      });
    };
    auto leaveB = [&](auto qc, bool storeRows) __attribute__((always_inline)) {
      constexpr int qi = decltype(qc)::value;
      constexpr int PHI = 4 * PH + qi;
      constexpr int done = (PHI - GB + GP) % GP;
      const int jrel = 4 * (4 * (s - 2) + qi - 1) - 2 * RB;
      const bool ok = jrel >= 0 && jrel < nrows;
      if (storeRows && !PAIR_TV(2)) {
        const int voff = ok ? vOutB : 0x7ffffff0;
        const unsigned rowOff = ok ? (unsigned)(y0 + jrel) * (unsigned)W * 4u : 0u;
        if (TRB) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, accB[done]), routB, voff, (int)rowOff, 0);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)accB[done][i]), routB, voff, (int)(rowOff + (unsigned)i * (unsigned)W * 4u), 0);
        }
      }
      if (ok) minmax4(mnB, mxB, accB[done]);
    };
    constexpr bool kBatched = (SSRLCV_PAIR_OPT & 8) != 0;
    if (kBatched) {
      rm_static_for<4>([&](auto qc) __attribute__((always_inline)) { quantumA(qc, false); });
      rm_static_for<4>([&](auto qc) __attribute__((always_inline)) { leaveA(qc, true); });
      SV_STAMP(5);
      quantumB(std::integral_constant<int, 0>{}, false);
      quantumB(std::integral_constant<int, 1>{}, false);
      leaveB(std::integral_constant<int, 0>{}, true);
      leaveB(std::integral_constant<int, 1>{}, true);
      quantumB(std::integral_constant<int, 2>{}, false);
      quantumB(std::integral_constant<int, 3>{}, false);
      leaveB(std::integral_constant<int, 2>{}, true);
      leaveB(std::integral_constant<int, 3>{}, true);
    } else {
      rm_static_for<4>([&](auto qc) __attribute__((always_inline)) {
        quantumA(qc, true);
        leaveA(qc, false);
      });
      SV_STAMP(5);
      rm_static_for<4>([&](auto qc) __attribute__((always_inline)) {
        quantumB(qc, true);
        leaveB(qc, false);
      });
    }
    SV_STAMP(6);
    if (!PAIR_TV(64)) __syncthreads();  // H buffers free; the level-a tile, the next row stage (and the u8 rows' readers) complete
    SV_STAMP(7);
  };
  for (int s = 0; s < steps; s += P) {
    rm_static_for<P>([&](auto pc) __attribute__((always_inline)) { step(s + decltype(pc)::value, pc); });
  }
  // a lane outside the image (level a) or outside the strip (level b) has reduced values nobody stored
  if (!ownA) { mnA = FLT_MAX; mxA = -FLT_MAX; }
  if (!ownB) { mnB = FLT_MAX; mxB = -FLT_MAX; }
  if (a.minmaxA) block_minmax_commit(mnA, mxA, a.minmaxA, s_mem);
  if (a.minmaxB) block_minmax_commit(mnB, mxB, a.minmaxB, s_mem);
}

bool pair_rm_usable(uint32_t w, uint32_t h) {
  return !svdev::sw().noGaussPairRm && (w & 15) == 0 && (h & 15) == 0 && w >= 512 && h >= 64;
}

// the matrix-pipe form of launch_pair (same arguments, same results); the caller has checked pair_usable and pair_rm_usable
int launch_pair_rm(const float* in, const uint8_t* u8src, float* outA, float* outB, uint32_t w, uint32_t h, const float* wA, const float* wB,
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
  p.stamps = g_lab_stamps;
#endif
  static int cus = 0, perCu[2] = {0, 0};
  constexpr size_t ldsBytes = PairRm::ldsBytes;
  if (!cus) {
    SSRLCV_HIP_TRY(hipFuncSetAttribute((const void*)k_gauss_pair_rm<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
    SSRLCV_HIP_TRY(hipFuncSetAttribute((const void*)k_gauss_pair_rm<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
    int dev = 0;
    SSRLCV_HIP_TRY(hipGetDevice(&dev));
    SSRLCV_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu[0], (const void*)k_gauss_pair_rm<false>, 256, ldsBytes) != hipSuccess || perCu[0] < 1) perCu[0] = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu[1], (const void*)k_gauss_pair_rm<true>, 256, ldsBytes) != hipSuccess || perCu[1] < 1) perCu[1] = 1;
  }
  const int rowsForced = svdev::sw().pairRows;
  const uint32_t strips = (w + 239) / 240;
  uint32_t by = (uint32_t)(perCu[u8src ? 1 : 0] * cus) / strips;  // one round of resident blocks
  by = by < 1 ? 1 : by;
  uint32_t rows = (h + by - 1) / by;
  rows = rows < 64 ? 64 : rows;
  if (rowsForced > 0) rows = (uint32_t)rowsForced;
  rows = (rows + 15) / 16 * 16;
  p.rowsPerBlock = rows;
  const dim3 grid(strips, (h + rows - 1) / rows);
  if (u8src) hipLaunchKernelGGL((k_gauss_pair_rm<true>), grid, dim3(256), ldsBytes, st, p);
  else hipLaunchKernelGGL((k_gauss_pair_rm<false>), grid, dim3(256), ldsBytes, st, p);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}
