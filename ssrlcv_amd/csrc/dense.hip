// ssrlcv_amd/csrc/dense.hip -- dense SIFT: SIFT_FeatureFactory::generateFeatures(image, dense = true, ..) for gfx950.
//
// Key points on a regular grid, all at one scale, on the image itself (no scale space).  The result is DEFINED as what the
// per-kernel exports of keypoints.hip / pyramid.hip give when they are chained over that grid (include/ssrlcv_hip.h states
// the chain; tests/dense_ref.py runs it) and the kernels here are held to it bit for bit.  They are not that chain:
//
//   k_dense_minmax   min / max of the u8 image (the level's normalisation constants; float(u8) is monotone and exact)
//   k_dense_polar    ONE pass over the image: normalised level L, and per pixel the gradient's magnitude, raw sv_atan2f
//                    and orientation-histogram bin.  No later kernel evaluates atan2f or sqrtf: on a stride-1 grid a pixel is
//                    sampled by (2 wo + 1)^2 orientation windows and about (2 wd + 1)^2 descriptor windows.
//   k_dense_weights  the (2 wo + 1)^2 Gaussian weights of the orientation window: they depend on the integer offset alone
//   k_dense_orient   a block owns a tile of grid points and stages the tile's pixels + halo wo (magnitude, bin) in LDS
//                    once; one lane per grid point walks its window in raster order -- the single fmaf chain per bin of
//                    the reference kernel -- into a histogram column in LDS (no 36-way select chain), picks its peaks
//                    (svf::pick_orientations) and writes the survivors slot-compacted with their count
//   (scan)           exclusive scan of the counts (scan_lookback.h): where each grid point's features start
//   k_dense_desc     a block owns the same kind of tile with halo wd (magnitude, angle) in LDS; one wave per oriented key
//                    point gathers its rotated window from LDS; records leave through LDS as 16-byte stores
//
// Every result-defining expression -- gradient stencil, polar form, bin, window widths, weights, peak picking, votes, norms,
// bytes -- is the one function of sift_sampling.h that k_x_gradients / k_x_thetas / k_x_descriptors call as well.  What the
// reformulation keeps besides (keypoints.hip, k_x_thetas): a histogram bin is one fmaf(mag, wgt, hist[bin]) chain over the
// window, y outer, x inner; a sample whose bin comes out as 36 votes nowhere.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "device_math.h"
#include "scan_lookback.h"
#include "sift_sampling.h"

namespace {

constexpr uint32_t kMaxHalo = 32;          // wo, wd <= 32: the largest tile of one grid point is 65 x 65 pixels
constexpr size_t kLdsBudget = 60 * 1024;   // dynamic LDS of one block (64 KB with the static arrays)
constexpr uint32_t kNoBin = 36;            // svf::orientation_bin == 36: votes nowhere

struct DenseGeom {
  uint32_t w, h, stride, margin, nx, ny, wo, wd;
};
struct DenseLayout {
  size_t mm, level, polar, bin, wtab, thetas, cnt, off, scan, total;
};
struct TileShape {
  uint32_t px, py;  // grid points per block, x and y
};

inline bool finite_pos(float v) { return v > 0.0f && v <= FLT_MAX; }

// the window widths are the chain's (sift_sampling.h; pixelWidth = 1)
int dense_geom(uint32_t w, uint32_t h, const ssrlcv_dense_params* p, DenseGeom* g) {
  if (!p) return SSRLCV_ERR_INVALID_ARG;
  if (p->stride == 0 || !finite_pos(p->sigma) || !finite_pos(p->orientationContribWidth) || !finite_pos(p->descriptorContribWidth) ||
      p->maxOrientations < 1 || p->maxOrientations > 8)
    return SSRLCV_ERR_INVALID_ARG;
  const float wo = svf::orientation_window(p->sigma, p->orientationContribWidth, 1.0f);
  const float wd = svf::descriptor_window(p->sigma, p->descriptorContribWidth, 1.0f);
  if (!(wo <= (float)kMaxHalo) || !(wd <= (float)kMaxHalo)) return SSRLCV_ERR_UNSUPPORTED;
  g->w = w;
  g->h = h;
  g->stride = p->stride;
  g->wo = (uint32_t)wo;
  g->wd = (uint32_t)wd;
  g->margin = g->wo > g->wd ? g->wo : g->wd;
  // x = margin + i stride <= w - 2 - margin
  const int64_t spanX = (int64_t)w - 2 - 2 * (int64_t)g->margin, spanY = (int64_t)h - 2 - 2 * (int64_t)g->margin;
  g->nx = spanX < 0 ? 0u : (uint32_t)(spanX / p->stride) + 1u;
  g->ny = spanY < 0 ? 0u : (uint32_t)(spanY / p->stride) + 1u;
  if (g->nx == 0 || g->ny == 0) g->nx = g->ny = 0;
  if ((uint64_t)g->nx * g->ny * p->maxOrientations >= (1ull << 31)) return SSRLCV_ERR_INVALID_ARG;
  return SSRLCV_OK;
}


// workspace: {min, max} | L float[w h] | polar float2[w h] | bin u8[w h] | weights float[(2 wo + 1)^2] |
//            thetas float[n maxO] | counts u32[n + 1] | offsets u32[n + 1] | scan descriptors        (n = nx ny)
DenseLayout dense_layout(const DenseGeom& g, uint32_t maxO) {
  DenseLayout L;
  const size_t px = (size_t)g.w * g.h, n = (size_t)g.nx * g.ny, side = 2 * g.wo + 1;
  size_t at = 0;
  L.mm = at;      at += 256;
  L.level = at;   at += align256(px * 4);
  L.polar = at;   at += align256(px * 8);
  L.bin = at;     at += align256(px);
  L.wtab = at;    at += align256(side * side * 4);
  L.thetas = at;  at += align256(n * maxO * 4);
  L.cnt = at;     at += align256((n + 1) * 4);
  L.off = at;     at += align256((n + 1) * 4);
  L.scan = at;    at += svs::workspace_bytes<1>(svs::scan_tiles<8>((uint32_t)(n + 1)));
  L.total = at;
  return L;
}

// pixels a tile of `points` grid points spans.  In 64 bits: (points - 1) stride passes 2^32 for the strides near it, and a
// wrapped extent would size a tile smaller than one window.  Capped at 2^20, far above what fits LDS, so that the products
// of two extents below stay exact as well.
inline size_t tile_extent(uint32_t points, uint32_t stride, uint32_t halo) {
  const uint64_t e = (uint64_t)(points - 1) * stride + 2 * halo + 1;
  return (size_t)(e < (1ull << 20) ? e : (1ull << 20));
}
inline size_t orient_lds(TileShape t, uint32_t stride, uint32_t wo) {
  const size_t tw = tile_extent(t.px, stride, wo), th = tile_extent(t.py, stride, wo), side = 2 * wo + 1;
  return tw * th * 4 + side * side * 4 + (size_t)36 * t.px * t.py * 4 + (tw * th + 3) / 4 * 4;
}
inline size_t desc_lds(TileShape t, uint32_t stride, uint32_t wd) {
  return tile_extent(t.px, stride, wd) * tile_extent(t.py, stride, wd) * 8;
}
// the largest tile of grid points whose LDS fits; one point always does (halo <= 32).  A stride too long for two points
// to share a tile leaves a block with one window: that is then all the sharing there is.
template <typename F>
TileShape pick_tile(F bytes) {
  static const TileShape cand[] = {{16, 16}, {16, 8}, {8, 8}, {8, 4}, {4, 4}, {4, 2}, {2, 2}, {2, 1}, {1, 1}};
  for (const TileShape& t : cand)
    if (bytes(t) <= kLdsBudget) return t;
  return TileShape{1, 1};
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_minmax(const uint8_t* __restrict__ px, size_t n, uint32_t* __restrict__ mm) {
  uint32_t mn = 255u, mx = 0u;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const uint32_t v = px[i];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&mm[0], mn);
    atomicMax(&mm[1], mx);
  }
}

// L = (float(u8) - min) / (max - min) as k_normalize computes it; the gradient is k_x_gradients' stencil on L
__global__ __launch_bounds__(256) void k_dense_polar(const uint8_t* __restrict__ px, int W, int H, const uint32_t* __restrict__ mm,
                                                     float* __restrict__ level, float2* __restrict__ polar, uint8_t* __restrict__ bins) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)W * H) return;
  const int x = (int)(id % W), y = (int)(id / W);
  const float mn = (float)mm[0], mx = (float)mm[1];
  const sv::Divisor range = sv::make_divisor(mx - mn);
  level[id] = sv::div_by((float)px[id] - mn, range);
  const float2 r = svf::polar_of(svf::gradient_taps(x, y, W, H, [&](size_t a) { return sv::div_by((float)px[a] - mn, range); }));
  const int bin = svf::orientation_bin(r.y);
  polar[id] = r;
  bins[id] = (uint8_t)((unsigned)bin < kNoBin ? bin : (int)kNoBin);
}

__global__ __launch_bounds__(256) void k_dense_weights(float* __restrict__ wtab, int wo, float sigma, float lambda) {
  const int side = 2 * wo + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= side * side) return;
  wtab[i] = svf::orientation_weight((float)(i % side - wo), (float)(i / side - wo), svf::orientation_weight_denom(sigma, lambda));
}

struct TileArgs {
  int W, H;
  uint32_t stride, margin, nx, ny, halo, px, py, tilesX;
};

__global__ __launch_bounds__(256) void k_dense_orient(TileArgs a, const float2* __restrict__ polar, const uint8_t* __restrict__ bins,
                                                      const float* __restrict__ wtab, uint32_t maxO, float orientationThreshold,
                                                      float* __restrict__ thetas, uint32_t* __restrict__ counts) {
  extern __shared__ float s_dyn[];
  const int wo = (int)a.halo, side = 2 * wo + 1;
  const int tw = (int)((a.px - 1) * a.stride) + side, th = (int)((a.py - 1) * a.stride) + side;
  const int nPts = (int)(a.px * a.py);
  float* s_mag = s_dyn;
  float* s_wt = s_mag + tw * th;
  float* s_hist = s_wt + side * side;
  uint8_t* s_bin = reinterpret_cast<uint8_t*>(s_hist + 36 * nPts);
  const int t = threadIdx.x, nT = blockDim.x;
  const uint32_t tileX = blockIdx.x % a.tilesX, tileY = blockIdx.x / a.tilesX;
  const int x0 = (int)(a.margin + tileX * a.px * a.stride) - wo, y0 = (int)(a.margin + tileY * a.py * a.stride) - wo;  // >= 0
  for (int i = t; i < tw * th; i += nT) {
    const int x = x0 + i % tw, y = y0 + i / tw;
    float m = 0.0f;
    uint8_t b = (uint8_t)kNoBin;
    if (x < a.W && y < a.H) {  // (past the image only in tiles the grid does not fill; those pixels are never sampled)
      m = polar[(size_t)y * a.W + x].x;
      b = bins[(size_t)y * a.W + x];
    }
    s_mag[i] = m;
    s_bin[i] = b;
  }
  for (int i = t; i < side * side; i += nT) s_wt[i] = wtab[i];
  for (int i = t; i < 36 * nPts; i += nT) s_hist[i] = 0.0f;
  __syncthreads();
  if (t >= nPts) return;
  const uint32_t lx = (uint32_t)t % a.px, ly = (uint32_t)t / a.px;
  const uint32_t gx = tileX * a.px + lx, gy = tileY * a.py + ly;
  if (gx >= a.nx || gy >= a.ny) return;
  // the window in raster order: hist[bin] = fmaf(mag, wgt, hist[bin]), one chain per bin (column t of s_hist)
  float* hist = s_hist + t;
  const int cx = (int)(lx * a.stride), cy = (int)(ly * a.stride);  // the window's top-left corner inside the tile
  for (int dy = 0; dy < side; ++dy) {
    const float* mrow = s_mag + (cy + dy) * tw + cx;
    const uint8_t* brow = s_bin + (cy + dy) * tw + cx;
    const float* wrow = s_wt + dy * side;
    for (int dx = 0; dx < side; ++dx) {
      const uint32_t bin = brow[dx];
      if (bin < kNoBin) hist[bin * nPts] = __builtin_fmaf(mrow[dx], wrow[dx], hist[bin * nPts]);
    }
  }
  const int regNumOrient = (int)(maxO > 8u ? 8u : maxO);
  float bx[8], by[8];
  svf::pick_orientations([&](int b) { return hist[b * nPts]; }, regNumOrient, orientationThreshold, bx, by);
  // what compact_thetas / compact_addresses leave of this key point's slots, in slot order
  const size_t g = (size_t)gy * a.nx + gx;
  uint32_t kept = 0;
  for (int i = 0; i < regNumOrient; ++i)
    if (bx[i] != 0.0f) thetas[g * maxO + kept++] = by[i];
  counts[g] = kept;
}

// wave-level hand-over through LDS: a wave's LDS operations complete in issue order; the fences keep the compiler from
// moving them across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_dense_desc(TileArgs a, const float2* __restrict__ polar, const float* __restrict__ thetas,
                                                    const uint32_t* __restrict__ offsets, uint32_t maxO, float sigma, float lambda,
                                                    ssrlcv_sift_feature* __restrict__ features, uint32_t capacity) {
  extern __shared__ float s_dyn[];
  __shared__ unsigned s_bins[4][128];
  __shared__ __attribute__((aligned(16))) uint32_t s_rec[4][40];  // one record at byte 0 or 8: 16-byte chunks line up with memory
  float2* s_pol = reinterpret_cast<float2*>(s_dyn);
  const int wd = (int)a.halo, sideT = 2 * wd + 1;
  const int tw = (int)((a.px - 1) * a.stride) + sideT, th = (int)((a.py - 1) * a.stride) + sideT;
  const int nPts = (int)(a.px * a.py);
  const uint32_t tileX = blockIdx.x % a.tilesX, tileY = blockIdx.x / a.tilesX;
  const int x0 = (int)(a.margin + tileX * a.px * a.stride) - wd, y0 = (int)(a.margin + tileY * a.py * a.stride) - wd;  // >= 0
  for (int i = threadIdx.x; i < tw * th; i += 256) {
    const int x = x0 + i % tw, y = y0 + i / tw;
    float2 p = make_float2(0.0f, 0.0f);
    if (x < a.W && y < a.H) p = polar[(size_t)y * a.W + x];
    s_pol[i] = p;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* bins = s_bins[wave];
  const float pixelWidth = 1.0f;
  for (int pt = wave; pt < nPts; pt += 4) {
    const uint32_t gx = tileX * a.px + (uint32_t)pt % a.px, gy = tileY * a.py + (uint32_t)pt / a.px;
    if (gx >= a.nx || gy >= a.ny) continue;
    const size_t g = (size_t)gy * a.nx + gx;
    const uint32_t first = offsets[g], cnt = offsets[g + 1] - first;
    const float kx = (float)(a.margin + gx * a.stride), ky = (float)(a.margin + gy * a.stride);
    for (uint32_t slot = 0; slot < cnt; ++slot) {
      const uint32_t fi = first + slot;
      if (fi >= capacity) break;
      const float theta = thetas[g * maxO + slot];
      bins[lane] = 0u;
      bins[lane + 64] = 0u;
      wave_sync();
      // ---- k_x_descriptors' body from sift_sampling.h; the gradient's magnitude and direction come from the tile
      const svf::DescriptorFrame fr = svf::descriptor_frame(sigma, theta, lambda, pixelWidth);
      const int iw = (int)fr.windowWidth, side = 2 * iw + 1;
      for (int sIdx = lane; sIdx < side * side; sIdx += 64) {
        float cx, cy;
        if (!svf::rotate_sample(fr, (float)(sIdx % side - iw), (float)(sIdx / side - iw), cx, cy)) continue;
        const int sx = (int)llroundf(cx + kx) - x0, sy = (int)llroundf(cy + ky) - y0;
        float2 p = make_float2(0.0f, 0.0f);
        if (sx >= 0 && sx < tw && sy >= 0 && sy < th) p = s_pol[sy * tw + sx];  // (always: |cx|, |cy| <= wd)
        const float mag = p.x * svf::sample_weight(fr, cx, cy);
        const float ang = svf::relative_angle(p.y, theta);
        // k_x_descriptors walks the sixteen cells and, inside a cell it votes in, the eight directions -- a wave then runs
        // every cell and direction ANY of its lanes votes in.  Here a lane first collects the cells (at most nine) and
        // directions (at most two) that pass the same tests, then walks its own; the votes are the same functions, and
        // their integer sums do not depend on the order.
        unsigned cells = 0u, dirs = 0u;
        float hx, hy, angle;
#pragma unroll
        for (int cell = 0; cell < 16; ++cell)
          if (svf::cell_offsets(fr, cell >> 2, cell & 3, cx, cy, hx, hy)) cells |= 1u << cell;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (svf::direction_offset(ang, k, angle)) dirs |= 1u << k;
        while (cells != 0u) {
          const int cell = __ffs(cells) - 1;
          cells &= cells - 1u;
          (void)svf::cell_offsets(fr, cell >> 2, cell & 3, cx, cy, hx, hy);
          for (unsigned left = dirs; left != 0u; left &= left - 1u) {
            const int k = __ffs(left) - 1;
            (void)svf::direction_offset(ang, k, angle);
            atomicAdd(&bins[cell * 8 + k], svf::vote_fixed(hx, hy, angle, mag, fr.voteScale));
          }
        }
      }
      wave_sync();
      float v0 = (float)bins[lane], v1 = (float)bins[lane + 64];  // elements lane and lane + 64 of the bins in [nx][ny][k] order
      const float sq = svf::normalise_pair(v0, v1);
      char* out = reinterpret_cast<char*>(features + fi);
      const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 8u);  // records are 8-byte aligned, 152 bytes long
      uint8_t* rec = reinterpret_cast<uint8_t*>(s_rec[wave]) + shift;
      rec[24 + svf::descriptor_slot(lane)] = svf::descriptor_byte(v0, sq);
      rec[24 + svf::descriptor_slot(lane + 64)] = svf::descriptor_byte(v1, sq);
      if (lane == 0) {
        uint32_t* r32 = reinterpret_cast<uint32_t*>(rec);
        r32[0] = 0xffffffffu;  // parent = -1, as the sparse path writes it
        r32[1] = 0u;           // the padding before the 8-aligned loc
        r32[2] = __float_as_uint(kx * pixelWidth);
        r32[3] = __float_as_uint(ky * pixelWidth);
        r32[4] = __float_as_uint(sigma);
        r32[5] = __float_as_uint(theta);
      }
      wave_sync();
      // ten 16-byte chunks of s_rec cover the record; the first (shift 8) or the last (shift 0) is half a chunk
      if (lane < 10) {
        const uint4 v = *reinterpret_cast<const uint4*>(&s_rec[wave][lane * 4]);
        char* dst = out - shift + lane * 16;
        if (shift != 0u && lane == 0) *reinterpret_cast<uint2*>(dst + 8) = make_uint2(v.z, v.w);
        else if (shift == 0u && lane == 9) *reinterpret_cast<uint2*>(dst) = make_uint2(v.x, v.y);
        else *reinterpret_cast<uint4*>(dst) = v;
      }
      wave_sync();
    }
  }
}

}  // namespace

extern "C" {

int ssrlcv_sift_dense_grid(uint32_t w, uint32_t h, const ssrlcv_dense_params* params, uint32_t* margin, uint32_t* nx, uint32_t* ny) {
  DenseGeom g;
  const int rc = dense_geom(w, h, params, &g);
  if (rc) return rc;
  if (margin) *margin = g.margin;
  if (nx) *nx = g.nx;
  if (ny) *ny = g.ny;
  return SSRLCV_OK;
}

uint32_t ssrlcv_sift_dense_max_features(uint32_t w, uint32_t h, const ssrlcv_dense_params* params) {
  DenseGeom g;
  if (dense_geom(w, h, params, &g)) return 0;
  return g.nx * g.ny * params->maxOrientations;
}

size_t ssrlcv_hip_sift_dense_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_dense_params* params) {
  DenseGeom g;
  if (dense_geom(w, h, params, &g)) return 0;
  return dense_layout(g, params->maxOrientations).total;
}

int ssrlcv_hip_sift_dense_u8(const uint8_t* pixels, uint32_t w, uint32_t h, const ssrlcv_dense_params* params, void* workspace,
                             size_t workspaceBytes, ssrlcv_sift_feature* features, uint32_t capacity, uint32_t* numFeatures,
                             ssrlcv_stream_t stream) {
  DenseGeom g;
  const int rc = dense_geom(w, h, params, &g);  // the parameters first: their codes do not depend on the buffers
  if (rc) return rc;
  if (!pixels || !workspace || !numFeatures || (!features && capacity != 0)) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t maxO = params->maxOrientations;
  const DenseLayout L = dense_layout(g, maxO);
  if (workspaceBytes < L.total) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t n = g.nx * g.ny;
  if (n == 0) {
    SSRLCV_HIP_TRY(hipMemsetAsync(numFeatures, 0, 4, st));
    return SSRLCV_OK;
  }
  char* ws = (char*)workspace;
  uint32_t* mm = (uint32_t*)(ws + L.mm);
  float* level = (float*)(ws + L.level);
  float2* polar = (float2*)(ws + L.polar);
  uint8_t* bins = (uint8_t*)(ws + L.bin);
  float* wtab = (float*)(ws + L.wtab);
  float* thetas = (float*)(ws + L.thetas);
  uint32_t* cnt = (uint32_t*)(ws + L.cnt);
  uint32_t* off = (uint32_t*)(ws + L.off);
  const size_t px = (size_t)w * h;

  SSRLCV_HIP_TRY(hipMemsetAsync(mm, 0xff, 4, st));
  SSRLCV_HIP_TRY(hipMemsetAsync(mm + 1, 0, 4, st));
  SSRLCV_HIP_TRY(hipMemsetAsync(cnt + n, 0, 4, st));
  size_t mmBlocks = (px + 256 * 16 - 1) / (256 * 16);
  if (mmBlocks > 2048) mmBlocks = 2048;
  hipLaunchKernelGGL(k_dense_minmax, dim3((unsigned)mmBlocks), dim3(256), 0, st, pixels, px, mm);
  hipLaunchKernelGGL(k_dense_polar, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, pixels, (int)w, (int)h, mm, level, polar, bins);
  const uint32_t side = 2 * g.wo + 1;
  hipLaunchKernelGGL(k_dense_weights, dim3((side * side + 255) / 256), dim3(256), 0, st, wtab, (int)g.wo, params->sigma,
                     params->orientationContribWidth);

  TileArgs a;
  a.W = (int)w;
  a.H = (int)h;
  a.stride = g.stride;
  a.margin = g.margin;
  a.nx = g.nx;
  a.ny = g.ny;
  {
    const TileShape t = pick_tile([&](TileShape s) { return orient_lds(s, g.stride, g.wo); });
    a.halo = g.wo;
    a.px = t.px;
    a.py = t.py;
    a.tilesX = (g.nx + t.px - 1) / t.px;
    const uint32_t tilesY = (g.ny + t.py - 1) / t.py, threads = t.px * t.py < 64 ? 64 : t.px * t.py;
    hipLaunchKernelGGL(k_dense_orient, dim3(a.tilesX * tilesY), dim3(threads), orient_lds(t, g.stride, g.wo), st, a, polar, bins, wtab, maxO,
                       params->orientationThreshold, thetas, cnt);
  }
  SSRLCV_HIP_TRY(svs::exclusive_scan<8>(cnt, off, n + 1, ws + L.scan, st));
  SSRLCV_HIP_TRY(hipMemcpyAsync(numFeatures, off + n, 4, hipMemcpyDeviceToDevice, st));
  if (capacity != 0) {
    const TileShape t = pick_tile([&](TileShape s) { return desc_lds(s, g.stride, g.wd); });
    a.halo = g.wd;
    a.px = t.px;
    a.py = t.py;
    a.tilesX = (g.nx + t.px - 1) / t.px;
    const uint32_t tilesY = (g.ny + t.py - 1) / t.py;
    hipLaunchKernelGGL(k_dense_desc, dim3(a.tilesX * tilesY), dim3(256), desc_lds(t, g.stride, g.wd), st, a, polar, thetas, off, maxO, params->sigma,
                       params->descriptorContribWidth, features, capacity);
  }
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
