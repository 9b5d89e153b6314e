// tools/simplify_lab.hip -- A/B of the error pass of the surface simplification (include/ssrlcv_hip.h "surface simplification"
// item 1): a fused form -- the levels k < 2 of a 64 x 64 tile and its halo in LDS (k_fine_errors, below), then the strided lattice --
// against the shipped form, one launch a half-level from k = 0.  Includes csrc/simplify.hip itself, so the shipped form and the levels
// above the tile are the library's code.  The fused form is bit-equal and lost on every map (profiles/simplify_bench.txt), so it
// stays here.  Also times a device copy of the pass's 8 bytes a node.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I ssrlcv_amd/csrc tools/simplify_lab.hip -o tools/_build/simplify_lab
//   simplify_lab <w> <h> <height raw float32 | plane | noise | holes> [repeats]
// prints one line: "<map> <w> x <h>: fused <ms> (min .. max), level-by-level <ms> (min .. max), copy <ms>, equal <0|1>"
#define SSRLCV_SIMPLIFY_LAB
#include "../ssrlcv_amd/csrc/simplify.hip"

namespace svsimp {

constexpr int kFineLevels = 2;        // the levels k_fine_errors computes in LDS
constexpr int kCore = 64;             // the nodes a block of k_fine_errors owns, a side
constexpr int kHalo = 8;              // >= 5, the reach of the two finest levels, and a multiple of 4
constexpr int kRegion = kCore + 2 * kHalo;  // cells a side; 81 x 81 nodes of heights and of errors: 52 KB of LDS, three blocks a CU
constexpr int kPitch = kRegion + 1;   // odd: rows and columns are both conflict-free

// ---- the two finest levels of a tile in LDS.  E(m) is the maximum of e over m's descendants, and they do not stop at a tile's
// border: a D-node of level k reaches 3 2^k nodes away (its A-children stand 2^k away and an A-node reaches 2 2^k), so a tile
// that owns the levels k < 2 of its nodes needs the E of nodes up to 4 away and the heights up to 5 away.  The block loads its
// 64 x 64 nodes and a halo of 8 (a multiple of 4: the region's lattices are the domain's), computes both levels over the
// whole region -- near the region's rim from missing inputs, which no owned node reaches -- and stores the owned nodes: one
// writer an entry, no atomics.  The halo is 56 % more nodes to load and compute than are stored; levels k >= 2 would need a
// halo of 11 and more, so they stay with k_level.  (A tile WITHOUT a halo whose seam nodes are merged by an atomicMax, the
// first form tried, is wrong: an interior D-node reads the seam A-node's partial maximum before the neighbour has added its own.)
__global__ __launch_bounds__(256) void k_fine_errors(const float* __restrict__ height, Dom d, int levels, uint32_t tilesX,
                                                     uint32_t* __restrict__ error) {
  __shared__ uint32_t s_h[kPitch * kPitch];
  __shared__ uint32_t s_e[kPitch * kPitch];
  const uint32_t tileY = blockIdx.x / tilesX;  // a one-dimensional grid: a thin map has more tile rows than a grid has in y
  const int tx0 = (int)(blockIdx.x - tileY * tilesX) * kCore, ty0 = (int)tileY * kCore;
  const int rx0 = tx0 - kHalo, ry0 = ty0 - kHalo;
  for (int i = threadIdx.x; i < kPitch * kPitch; i += 256) {
    const int ly = i / kPitch, lx = i - ly * kPitch;
    const int gx = rx0 + lx, gy = ry0 + ly;
    s_h[i] = d.in_grid(gx, gy) ? __float_as_uint(height[d.at(gx, gy)]) : kNaN;
    s_e[i] = kInf;  // a node outside the grid; every other node of a level is written before it is read
  }
  __syncthreads();
  auto in_region = [=](int x, int y) { return (uint32_t)(x - rx0) <= (uint32_t)kRegion && (uint32_t)(y - ry0) <= (uint32_t)kRegion; };
  auto hbits = [&](int x, int y) -> uint32_t { return in_region(x, y) ? s_h[(y - ry0) * kPitch + (x - rx0)] : kNaN; };
  auto ebits = [&](int x, int y) -> uint32_t { return in_region(x, y) ? s_e[(y - ry0) * kPitch + (x - rx0)] : 0u; };
  for (int k = 0; k < levels; ++k) {
    const int n1 = (kRegion >> k) + 1;
    for (int phase = 0; phase < 2; ++phase) {  // A-nodes read the D-nodes of k - 1, D-nodes the A-nodes of k
      for (int i = threadIdx.x; i < n1 * n1; i += 256) {
        const int iy = i / n1, ix = i - iy * n1;
        const bool ox = ix & 1, oy = iy & 1;  // rx0 and ry0 are multiples of 8: the parities are the domain's
        if (phase == 0 ? (ox == oy) : !(ox && oy)) continue;
        const int gx = rx0 + (ix << k), gy = ry0 + (iy << k);
        if (!d.in_domain(gx, gy)) continue;
        const Split s = split_of(gx, gy, k);
        const uint32_t e = node_e(d, gx, gy, k, s, hbits);
        s_e[(iy << k) * kPitch + (ix << k)] = umax(e, children_max(d, gx, gy, k, s.dnode, ebits));
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < kCore * kCore; i += 256) {
    const int ly = i / kCore, lx = i - ly * kCore;
    const int gx = tx0 + lx, gy = ty0 + ly;
    if (!d.in_grid(gx, gy) || node_k((uint32_t)gx, (uint32_t)gy) >= levels) continue;  // a node of a level above: k_level's
    error[d.at(gx, gy)] = s_e[(ly + kHalo) * kPitch + (lx + kHalo)];
  }
}

// the fused form: the fine kernel, then the library's launches from level 2
inline hipError_t errors_fused(const float* height, Dom d, uint32_t* error, hipStream_t st) {
  const int levels = d.L < kFineLevels ? d.L : kFineLevels;
  if (levels > 0) {
    const uint32_t tilesX = (d.w - 1) / kCore + 1, tilesY = (d.h - 1) / kCore + 1;  // they cover the nodes
    hipLaunchKernelGGL(k_fine_errors, dim3(tilesX * tilesY), dim3(256), 0, st, height, d, levels, tilesX, error);
  }
  return errors_launch(height, d, error, st, levels);
}

}  // namespace svsimp

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define LAB_TRY(expr)                                                                                       \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return 1; } \
  } while (0)

struct Times { float med, lo, hi; };
static Times summary(std::vector<float> t) {
  std::sort(t.begin(), t.end());
  return Times{t[t.size() / 2], t.front(), t.back()};
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s <w> <h> <height raw float32 | plane | noise | holes> [repeats]\n", argv[0]);
    return 2;
  }
  const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]);
  const std::string what = argv[3];
  const int repeats = argc > 4 ? std::max(3, std::atoi(argv[4])) : 9;
  if (w == 0 || h == 0 || (unsigned long long)w * h > (1ull << 29)) { std::fprintf(stderr, "1 <= w h <= 2^29\n"); return 2; }
  const size_t n = (size_t)w * h;
  std::vector<float> host(n);
  if (what == "plane" || what == "noise" || what == "holes") {
    uint32_t s = 12345u;
    for (size_t i = 0; i < n; ++i) {
      s = s * 1664525u + 1013904223u;
      const float r = (float)(s >> 8) * (1.0f / 16777216.0f);
      const float x = (float)(i % w), y = (float)(i / w);
      host[i] = what == "plane" ? 0.5f * x - 0.25f * y : what == "noise" ? r : sinf(x * 0.01f) * cosf(y * 0.013f) * 20.0f;
      if (what == "holes" && r < 0.05f) { const uint32_t nan = 0x7FC00000u; std::memcpy(&host[i], &nan, 4); }
    }
  } else {
    std::FILE* f = std::fopen(what.c_str(), "rb");
    if (!f || std::fread(host.data(), 4, n, f) != n) { std::fprintf(stderr, "cannot read %zu floats from %s\n", n, what.c_str()); return 2; }
    std::fclose(f);
  }
  float* height = nullptr;
  uint32_t *fused = nullptr, *naive = nullptr;
  LAB_TRY(hipMalloc(&height, n * 4));
  LAB_TRY(hipMalloc(&fused, n * 4));
  LAB_TRY(hipMalloc(&naive, n * 4));
  LAB_TRY(hipMemcpy(height, host.data(), n * 4, hipMemcpyHostToDevice));
  const svsimp::Dom d = svsimp::make_dom(w, h);
  hipEvent_t e0, e1;
  LAB_TRY(hipEventCreate(&e0));
  LAB_TRY(hipEventCreate(&e1));
  Times t[3];
  for (int form = 0; form < 3; ++form) {  // 0 fused, 1 one launch a half-level, 2 the copy
    std::vector<float> ms;
    for (int r = 0; r <= repeats; ++r) {
      LAB_TRY(hipEventRecord(e0, nullptr));
      if (form == 2) LAB_TRY(hipMemcpyAsync(naive, height, n * 4, hipMemcpyDeviceToDevice, nullptr));
      else if (form == 0) LAB_TRY(svsimp::errors_fused(height, d, fused, nullptr));
      else LAB_TRY(svsimp::errors_launch(height, d, naive, nullptr));
      LAB_TRY(hipEventRecord(e1, nullptr));
      LAB_TRY(hipEventSynchronize(e1));
      float v = 0;
      LAB_TRY(hipEventElapsedTime(&v, e0, e1));
      if (r) ms.push_back(v);  // the first run warms up
    }
    t[form] = summary(ms);
    if (form == 1) {  // before the copy overwrites it
      std::vector<uint32_t> a(n), b(n);
      LAB_TRY(hipMemcpy(a.data(), fused, n * 4, hipMemcpyDeviceToHost));
      LAB_TRY(hipMemcpy(b.data(), naive, n * 4, hipMemcpyDeviceToHost));
      host[0] = std::memcmp(a.data(), b.data(), n * 4) == 0 ? 1.0f : 0.0f;
    }
  }
  std::printf("%s %u x %u: fused %.4f ms (%.4f .. %.4f), level-by-level %.4f ms (%.4f .. %.4f), copy %.4f ms, equal %d\n", what.c_str(), w, h,
              t[0].med, t[0].lo, t[0].hi, t[1].med, t[1].lo, t[1].hi, t[2].med, (int)host[0]);
  (void)hipFree(height), (void)hipFree(fused), (void)hipFree(naive);
  return host[0] == 1.0f ? 0 : 1;
}
