// tools/terrain_lab.hip -- the A/B of the two forms of the terrain filter's erosion (include/ssrlcv_hip.h "terrain filter"), both
// from csrc/terrain.hip, which this file includes: the running minima (van Herk / Gil-Werman, a row pass and a column pass,
// erode_launch) against the direct form (k_direct: a 64 x 16 tile and its halo of r cells in LDS, the 2r + 1 taps of a row, then
// of a column, in one launch) at every radius the direct form is built for.  Selection in one total order: the two are bit-equal
// by construction, and the lab checks it.  The library takes the direct form up to kDirectMaxRadius;
// profiles/terrain_bench.txt holds the measured rows.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I ssrlcv_amd/csrc tools/terrain_lab.hip -o tools/_build/terrain_lab
//   terrain_lab <w> <h> <height raw float32 | noise | constant | holes> [repeats]
#define SSRLCV_TERRAIN_LAB
#include "../ssrlcv_amd/csrc/terrain.hip"

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
    std::fprintf(stderr, "usage: %s <w> <h> <height raw float32 | noise | constant | holes> [repeats]\n", argv[0]);
    return 2;
  }
  const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]);
  const std::string what = argv[3];
  const int repeats = argc > 4 ? std::max(3, std::atoi(argv[4])) : 7;
  if (w == 0 || h == 0 || (unsigned long long)w * h > (1ull << 29)) { std::fprintf(stderr, "1 <= w h <= 2^29\n"); return 2; }
  const size_t n = (size_t)w * h;
  std::vector<float> host(n);
  if (what == "noise" || what == "constant" || what == "holes") {
    uint32_t s = 12345u;
    for (size_t i = 0; i < n; ++i) {
      s = s * 1664525u + 1013904223u;
      const float r = (float)(s >> 8) * (1.0f / 16777216.0f);
      host[i] = what == "constant" ? 1.25f : r;
      s = s * 1664525u + 1013904223u;
      if (what == "holes" && (s >> 8) < 838861u) { const uint32_t nan = 0x7FC00000u; std::memcpy(&host[i], &nan, 4); }  // 5 %
    }
  } else {
    std::FILE* f = std::fopen(what.c_str(), "rb");
    if (!f || std::fread(host.data(), 4, n, f) != n) { std::fprintf(stderr, "cannot read %zu floats from %s\n", n, what.c_str()); return 2; }
    std::fclose(f);
  }
  uint32_t *in = nullptr, *shipped = nullptr, *direct = nullptr;
  int32_t *rows = nullptr, *scratch = nullptr;
  LAB_TRY(hipMalloc(&in, n * 4));
  LAB_TRY(hipMalloc(&shipped, n * 4));
  LAB_TRY(hipMalloc(&direct, n * 4));
  LAB_TRY(hipMalloc(&rows, n * 4));
  LAB_TRY(hipMalloc(&scratch, n * 4));
  LAB_TRY(hipMemcpy(in, host.data(), n * 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  LAB_TRY(hipEventCreate(&e0));
  LAB_TRY(hipEventCreate(&e1));
  bool allEqual = true;
  for (uint32_t r = 1; r <= svterrain::kDirectMaxRadius; ++r) {
    if (r > std::max(w, h) - 1u) break;
    Times t[3];
    for (int form = 0; form < 3; ++form) {  // 0 the direct form, 1 the shipped running minima, 2 a copy of the map
      std::vector<float> ms;
      for (int k = 0; k <= repeats; ++k) {
        LAB_TRY(hipEventRecord(e0, nullptr));
        if (form == 0) LAB_TRY((svterrain::direct_launch<false>(in, w, h, r, svterrain::Plain{direct}, nullptr)));
        else if (form == 1) LAB_TRY((svterrain::erode_launch<false>(in, rows, scratch, w, h, r, svterrain::Plain{shipped}, nullptr)));
        else LAB_TRY(hipMemcpyAsync(rows, in, n * 4, hipMemcpyDeviceToDevice, nullptr));
        LAB_TRY(hipEventRecord(e1, nullptr));
        LAB_TRY(hipEventSynchronize(e1));
        float v = 0;
        LAB_TRY(hipEventElapsedTime(&v, e0, e1));
        if (k) ms.push_back(v);  // the first run warms up
      }
      t[form] = summary(ms);
    }
    bool equal = true;
    for (int largest = 0; largest < 2; ++largest) {  // the erosions timed above, then the dilations
      if (largest) {
        LAB_TRY((svterrain::direct_launch<true>(in, w, h, r, svterrain::Plain{direct}, nullptr)));
        LAB_TRY((svterrain::erode_launch<true>(in, rows, scratch, w, h, r, svterrain::Plain{shipped}, nullptr)));
      }
      std::vector<uint32_t> a(n), b(n);
      LAB_TRY(hipMemcpy(a.data(), direct, n * 4, hipMemcpyDeviceToHost));
      LAB_TRY(hipMemcpy(b.data(), shipped, n * 4, hipMemcpyDeviceToHost));
      equal = equal && std::memcmp(a.data(), b.data(), n * 4) == 0;
    }
    allEqual = allEqual && equal;
    std::printf("%s %u x %u erode r %u: direct %.4f ms (%.4f .. %.4f), running minima %.4f ms (%.4f .. %.4f), copy %.4f ms, equal %d\n", what.c_str(), w,
                h, r, t[0].med, t[0].lo, t[0].hi, t[1].med, t[1].lo, t[1].hi, t[2].med, (int)equal);
  }
  (void)hipFree(in), (void)hipFree(shipped), (void)hipFree(direct), (void)hipFree(rows), (void)hipFree(scratch);
  return allEqual ? 0 : 1;
}
