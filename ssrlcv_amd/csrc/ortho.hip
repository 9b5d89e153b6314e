// ssrlcv_amd/csrc/ortho.hip -- the ortho-image of a height map for gfx950: every valid cell's world point projected into up to 8
// views, tested for occlusion by a march over the height map towards each camera, sampled bilinearly and chosen among the views
// that see it.  The contract is include/ssrlcv_hip.h "ortho-image"; tests/ortho_ref.py restates it.
//
//   k_ortho_top   the greatest height that is not a NaN, as an unsigned order key, through an integer atomicMax: one a wave
//   k_ortho       a thread per cell, a loop over the views, a height a step of the march.  64 neighbouring cells march side by
//                 side, so a wave's loads of one step are 64 neighbouring heights.  The march also stops, visible, once zr + bias
//                 has reached the greatest height: zr never decreases with the step (sz >= 0, and a rounded product and a
//                 rounded sum are monotone), so no later height can exceed it.  On a 4096^2 map under eight views this took 0.02
//                 (flat) to 0.08 (towers) of the time of the march without it at maxSteps 256 (profiles/ortho_bench.txt); with
//                 maxSteps 0 nothing marches and the pass over the map is not run.  A step forms its stop condition, loads --
//                 the lane's own cell where the step stops -- and tests behind the load; the same march with its exits in front
//                 of the load took 1.03 to 1.4 x as long.
// The march without the early stop, the plain form, is built aside with -DSSRLCV_ORTHO_PLAIN for tools/bench_ortho.py --form.  A
// third form was measured and is gone: the steps in batches of 4 whose loads are issued together and judged in order afterwards
// (which height a step reads depends on its number alone) gave the same bytes between 0.02 faster and 0.4 slower than one step
// at a time behind the early stop, which ends most marches inside the first batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ssrlcv_hip.h"
#include "align256.h"
#include "bilinear_u8.h"
#include "camera_host.h"
#include "device_math.h"
#include "dsm_frame.h"
#include "order_key.h"

namespace {

using dsm::finite_bits;
using dsm::finite_host;

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kMaxViews = 8;
constexpr float kFltMax = 3.4028234663852886e38f;
#ifdef SSRLCV_ORTHO_PLAIN
constexpr bool kEarly = false;
#else
constexpr bool kEarly = true;
#endif

struct Views {
  ssrlcv_ortho_view v[kMaxViews];
};

// the order key as an unsigned word: 0 lies below every value that is not a NaN
__device__ __forceinline__ uint32_t top_key(uint32_t bits) { return (uint32_t)order_key(bits) ^ 0x80000000u; }

__global__ __launch_bounds__(256) void k_ortho_top(const uint32_t* __restrict__ height, uint32_t cells, uint32_t* __restrict__ top) {
  uint32_t best = 0u;
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t c0 = blockIdx.x * 256u + threadIdx.x; c0 < cells; c0 += 4u * stride) {  // four loads in flight a lane
    uint32_t bits[4];
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) {
      const unsigned long long c = (unsigned long long)c0 + (unsigned long long)t * stride;
      bits[t] = c < cells ? height[c] : kNaN;
    }
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t)
      if ((bits[t] & 0x7FFFFFFFu) <= 0x7F800000u) best = max(best, top_key(bits[t]));  // an infinity counts: +inf occludes
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor(best, o, 64));
  if ((threadIdx.x & 63u) == 0u && best != 0u) atomicMax(top, best);
}

// "ortho-image", visibility: true if nothing between the cell and the camera stands above the line of sight
__device__ __forceinline__ bool visible(const uint32_t* __restrict__ height, uint32_t w, float fw, float fh, uint32_t c, float ci, float cj, float z,
                                        const float (&eye)[3], uint32_t maxSteps, float bias, float top) {
  const float du = eye[0] - ci, dv = eye[1] - cj, dz = eye[2] - z;
  if (!(dz > 0.0f)) return false;
  const float L = fmaxf(fabsf(du), fabsf(dv));
  if (L < 1.0f || maxSteps == 0u) return true;
  const float su = __fdiv_rn(du, L), sv = __fdiv_rn(dv, L), sz = __fdiv_rn(dz, L);
  for (uint32_t s = 1u;; ++s) {  // the dominant axis moves a whole cell a step: the march leaves the grid
    const float fs = (float)s;
    const float u = ci + fs * su, v = cj + fs * sv, zr = z + fs * sz;
    const float fi = floorf(u), fj = floorf(v);
    const float lim = zr + bias;
    // out of steps, past the camera, or outside the grid (compared on floats, as in rasterize): visible
    bool stop = s - 1u >= maxSteps || fs > L || !(fi >= 0.0f && fi < fw && fj >= 0.0f && fj < fh);
    if (kEarly) stop = stop || lim >= top;
    uint32_t at = c;  // a step that stops loads the lane's own cell: the one exit test of a step stands behind the load
    if (!stop) at = (uint32_t)fj * w + (uint32_t)fi;
    const uint32_t hb = height[at];
    if (stop) return true;
    if (hb != kNaN && __uint_as_float(hb) > lim) return false;  // +inf occludes, another NaN never does
  }
}

__global__ __launch_bounds__(256) void k_ortho(const uint32_t* __restrict__ height, ssrlcv_dsm_frame f, Views views, uint32_t m, uint32_t maxSteps,
                                               float bias, uint32_t rule, const uint32_t* __restrict__ topKey, uint8_t* __restrict__ ortho,
                                               uint8_t* __restrict__ seen, uint8_t* __restrict__ which) {
  const uint32_t cells = f.w * f.h;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= cells) return;
  const uint32_t zb = height[c];
  uint32_t mask = 0u, byte = 0u, from = 0xFFu;
  if (zb != kNaN && finite_bits(zb)) {
    float top = 0.0f;
    if (kEarly && maxSteps != 0u) {
      const uint32_t key = *topKey;  // not 0: this cell's own height is in it
      top = __uint_as_float((uint32_t)order_key(key ^ 0x80000000u));
    }
    const uint32_t j = c / f.w, i = c - j * f.w;
    const float z = __uint_as_float(zb);
    const float ci = (float)i + 0.5f, cj = (float)j + 0.5f;
    const float a = ci * f.cell, b = cj * f.cell;
    float P[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = ((f.origin[k] + (a * f.ex[k])) + (b * f.ey[k])) + (z * f.ez[k]);  // dsm_points' vertex
    const float fw = (float)f.w, fh = (float)f.h;
    unsigned long long bytes = 0ull;
    for (uint32_t k = 0; k < m; ++k) {
      const ssrlcv_ortho_view& v = views.v[k];
      const float dx = P[0] - v.pos[0], dy = P[1] - v.pos[1], dz = P[2] - v.pos[2];
      const float X = (v.M[0] * dx + v.M[1] * dy) + v.M[2] * dz;
      const float Y = (v.M[3] * dx + v.M[4] * dy) + v.M[5] * dz;
      const float W = (v.M[6] * dx + v.M[7] * dy) + v.M[8] * dz;
      const float sx = __fdiv_rn(X, W), sy = __fdiv_rn(Y, W);
      // MAPPED and INSIDE of "rectification": a NaN fails every comparison
      bool sees = W > 0.0f && fabsf(sx) <= kFltMax && fabsf(sy) <= kFltMax && sx >= 0.0f && sx <= (float)(v.w - 1u) && sy >= 0.0f &&
                  sy <= (float)(v.h - 1u);
      if (sees) sees = visible(height, f.w, fw, fh, c, ci, cj, z, v.eye, maxSteps, bias, top);
      if (sees) {
        mask |= 1u << k;
        bytes |= (unsigned long long)bilinear_u8(v.image, (int)v.w, (int)v.h, sx, sy) << (8u * k);
      }
    }
    if (mask != 0u) {
      if (rule == 0u) {  // FIRST
        from = (uint32_t)__ffs((int)mask) - 1u;
        byte = (uint32_t)(bytes >> (8u * from)) & 0xFFu;
      } else {  // the lower MEDIAN of the seeing views' bytes
        int32_t key[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) key[k] = (mask >> k) & 1u ? (int32_t)((bytes >> (8 * k)) & 0xFFull) : INT32_MAX;
        sort_network<8>(key);
        const int want = (__popc(mask) - 1) / 2;
        int32_t chosen = key[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) chosen = want == k ? key[k] : chosen;
        byte = (uint32_t)chosen;
#pragma unroll
        for (int k = 7; k >= 0; --k)
          if (((mask >> k) & 1u) && (uint32_t)((bytes >> (8 * k)) & 0xFFull) == byte) from = (uint32_t)k;  // the smallest such k
      }
    }
  }
  ortho[c] = (uint8_t)byte;
  if (seen) seen[c] = (uint8_t)mask;
  if (which) which[c] = (uint8_t)from;
}

// ---- host side
size_t top_bytes() { return align256(4); }

unsigned top_blocks(uint32_t cells) {
  const unsigned b = (unsigned)((cells + 255u) / 256u);
  return b > 2048u ? 2048u : b;
}

bool view_ok(const ssrlcv_ortho_view& v) {
  if (v.w == 0 || v.h == 0 || dsm::too_long_a_side(v.w, v.h) || dsm::too_many_cells(v.w, v.h)) return false;
  for (int k = 0; k < 9; ++k)
    if (!finite_host(v.M[k])) return false;
  for (int k = 0; k < 3; ++k)
    if (!finite_host(v.pos[k]) || !finite_host(v.eye[k])) return false;
  return true;
}

}  // namespace

extern "C" {

int ssrlcv_dsm_ortho_view_host(const ssrlcv_camera* cam, const ssrlcv_dsm_frame* frame, ssrlcv_ortho_view* out) {
  using namespace camera_host;
  if (!cam || !out || !dsm::frame_ok(frame)) return SSRLCV_ERR_INVALID_ARG;
  if (cam->size.x == 0 || cam->size.y == 0 || !finite_positive((double)cam->foc) || !finite_positive((double)cam->fov.x)) return SSRLCV_ERR_INVALID_ARG;
  const double fpx = focal_pixels((double)cam->foc, (double)cam->fov.x, (double)cam->size.x);
  if (!finite_positive(fpx)) return SSRLCV_ERR_INVALID_ARG;  // a field of view at a pole of tan
  const M3 R = euler_matrix((double)cam->cam_rot.x, (double)cam->cam_rot.y, (double)cam->cam_rot.z);
  const M3 K = {{{fpx, 0.0, (double)cam->size.x / 2.0}, {0.0, fpx, (double)cam->size.y / 2.0}, {0.0, 0.0, 1.0}}};
  const M3 M = mul(K, transpose(R));
  const double pos[3] = {(double)cam->cam_pos.x, (double)cam->cam_pos.y, (double)cam->cam_pos.z};
  double q[3];
  for (int k = 0; k < 3; ++k) q[k] = pos[k] - (double)frame->origin[k];
  const float* axes[3] = {frame->ex, frame->ey, frame->ez};
  double eye[3];
  for (int a = 0; a < 3; ++a) eye[a] = (q[0] * (double)axes[a][0] + q[1] * (double)axes[a][1]) + q[2] * (double)axes[a][2];
  eye[0] /= (double)frame->cell;
  eye[1] /= (double)frame->cell;
  ssrlcv_ortho_view o = *out;  // image is left as it was
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.M[3 * i + j] = (float)M.m[i][j];
  for (int k = 0; k < 3; ++k) {
    o.pos[k] = (float)pos[k];
    o.eye[k] = (float)eye[k];
  }
  o.w = cam->size.x;
  o.h = cam->size.y;
  *out = o;
  return SSRLCV_OK;
}

size_t ssrlcv_hip_dsm_ortho_workspace_bytes(uint32_t w, uint32_t h, uint32_t m) {
  if (dsm::too_many_cells(w, h) || dsm::too_long_a_side(w, h) || m == 0 || m > kMaxViews) return 0;
  return top_bytes();
}

int ssrlcv_hip_dsm_ortho(const float* height, const ssrlcv_dsm_frame* frame, const ssrlcv_ortho_view* views_host, uint32_t m,
                         const ssrlcv_ortho_params* params, uint8_t* ortho, uint8_t* seen, uint8_t* which, void* workspace, size_t workspaceBytes,
                         ssrlcv_stream_t stream) {
  if (!dsm::frame_ok(frame) || !params || !views_host) return SSRLCV_ERR_INVALID_ARG;
  if (m == 0 || m > kMaxViews || params->rule > 1u || !(params->bias >= 0.0f)) return SSRLCV_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < m; ++k)
    if (!view_ok(views_host[k])) return SSRLCV_ERR_INVALID_ARG;
  const uint32_t w = frame->w, h = frame->h;
  if (dsm::too_many_cells(w, h)) return SSRLCV_ERR_INVALID_ARG;
  if (dsm::too_long_a_side(w, h)) return SSRLCV_ERR_UNSUPPORTED;
  const uint32_t cells = w * h;
  if (cells == 0) return SSRLCV_OK;  // an empty grid: no output has an entry
  if (!height || !ortho || !workspace) return SSRLCV_ERR_INVALID_ARG;
  Views dev;
  memset(&dev, 0, sizeof dev);
  for (uint32_t k = 0; k < m; ++k) {
    if (!views_host[k].image) return SSRLCV_ERR_INVALID_ARG;
    dev.v[k] = views_host[k];
  }
  if (workspaceBytes < top_bytes()) return SSRLCV_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* top = (uint32_t*)workspace;
  if (kEarly && params->maxSteps != 0u) {  // without a march nothing reads it
    SSRLCV_HIP_TRY(hipMemsetAsync(top, 0, 4, st));
    hipLaunchKernelGGL(k_ortho_top, dim3(top_blocks(cells)), dim3(256), 0, st, (const uint32_t*)height, cells, top);
    SSRLCV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_ortho, dim3((cells + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)height, *frame, dev, m, params->maxSteps, params->bias,
                     params->rule, top, ortho, seen, which);
  SSRLCV_LAUNCH_CHECK();
  return SSRLCV_OK;
}

}  // extern "C"
