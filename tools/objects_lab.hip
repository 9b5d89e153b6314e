// tools/objects_lab.hip -- the A/B of the per-object reduction of "surface objects" (include/ssrlcv_hip.h), on csrc/objects.hip, which
// this file includes: the shipped k_obj_reduce (cells merge over runs of a wave, then per tile-local root in LDS, and each (tile,
// object, field) is flushed once) against the naive form k_obj_naive below (a thread a cell, one global atomic per cell and field).
// Both add into records in the same representation, so the lab compares their bytes and the ids.  It also times the labelling
// alone and a device copy of the bytes the call must move at least (the map once, plus ids).  profiles/objects_bench.txt holds the
// measured rows.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I ssrlcv_amd/csrc tools/objects_lab.hip \
//         ssrlcv_amd/csrc/disparity_filter.hip -o tools/_build/objects_lab
//   objects_lab <w> <h> <objects raw float32 | whole | checker | none | blobs> <min height> [repeats]
#define SSRLCV_OBJECTS_LAB
#include "../ssrlcv_amd/csrc/objects.hip"

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

namespace svobj {

__device__ __forceinline__ uint32_t final_label(const uint32_t* labels, uint32_t q) {
  const uint32_t l = labels[q];
  return l == kNone ? kNone : labels[l];
}

// the naive form: every member cell adds every field of its object's record itself
__global__ __launch_bounds__(256) void k_obj_naive(const uint32_t* __restrict__ in, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ number, uint32_t w, uint32_t h, float minHeight, float scale, uint32_t minCells,
                                                   uint32_t* __restrict__ ids, ssrlcv_object_record* __restrict__ records, uint32_t capacity) {
  const uint32_t n = w * h;
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < n; c += gridDim.x * 256u) {
    const uint32_t bits = in[c];
    uint32_t num = kNone, root = kNone;
    if (is_member(bits, minHeight)) {
      root = labels[labels[c]];
      if (counts[root] >= minCells) num = number[root];
    }
    if (ids) ids[c] = num;
    if (num >= capacity) continue;
    const uint32_t y = c / w, x = c - y * w;
    uint32_t sides = 0;
    sides += x == 0u || final_label(labels, c - 1u) != root;
    sides += x + 1u == w || final_label(labels, c + 1u) != root;
    sides += y == 0u || final_label(labels, c - w) != root;
    sides += y + 1u == h || final_label(labels, c + w) != root;
    ssrlcv_object_record* r = records + num;
    atomicMin(&r->minX, x);
    atomicMin(&r->minY, y);
    atomicMax(&r->maxX, x);
    atomicMax(&r->maxY, y);
    if (sides) atomicAdd(&r->perimeter, sides);
    atomicMax(reinterpret_cast<unsigned long long*>(&r->peakIndex), ((unsigned long long)ukey(bits) << 32) | (unsigned long long)(kNone - c));
    atomicMin(reinterpret_cast<uint32_t*>(&r->low), ukey(bits));
    const unsigned long long X = x, Y = y;
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumX), X);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumY), Y);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumXX), X * X);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumXY), X * Y);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumYY), Y * Y);
    const float t = __uint_as_float(bits) * scale;
    if (fabsf(t) <= 65536.0f) {
      const long long q = (long long)(int32_t)rintf(t);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumQ), (unsigned long long)q);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sumQQ), (unsigned long long)(q * q));
    } else {
      atomicAdd(&r->clipped, 1u);
    }
  }
}

}  // namespace svobj

struct Times { float med, lo, hi; };
static Times summary(std::vector<float> t) {
  std::sort(t.begin(), t.end());
  return Times{t[t.size() / 2], t.front(), t.back()};
}

int main(int argc, char** argv) {
  using namespace svobj;
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s <w> <h> <objects raw float32 | whole | checker | none | blobs> <min height> [repeats]\n", argv[0]);
    return 2;
  }
  const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]);
  const std::string what = argv[3];
  const int repeats = argc > 5 ? std::max(3, std::atoi(argv[5])) : 7;
  if (w == 0 || h == 0 || bad_size(w, h)) { std::fprintf(stderr, "1 <= w, h <= 65536 and w h <= 2^30\n"); return 2; }
  const ssrlcv_object_params params = {(float)std::atof(argv[4]), INFINITY, 256.0f, 1u};
  const uint32_t n = w * h;
  std::vector<float> host(n);
  if (what == "whole" || what == "checker" || what == "none" || what == "blobs") {
    uint32_t s = 12345u;
    for (uint32_t i = 0; i < n; ++i) {
      s = s * 1664525u + 1013904223u;
      const float r = (float)(s >> 8) * (1.0f / 16777216.0f);
      const uint32_t x = i % w, y = i / w;
      host[i] = what == "whole" ? params.minHeight + 1.0f + r : what == "none" ? params.minHeight - 1.0f - r
              : what == "checker" ? ((x + y) & 1u ? params.minHeight - 1.0f : params.minHeight + 1.0f + r)
              : (((x / 24u) + (y / 24u)) % 3u == 0u && x % 24u < 17u && y % 24u < 13u ? params.minHeight + 1.0f + r : params.minHeight - 0.5f * r - 0.1f);
    }
  } else {
    std::FILE* f = std::fopen(what.c_str(), "rb");
    if (!f || std::fread(host.data(), 4, n, f) != n) { std::fprintf(stderr, "cannot read %u floats from %s\n", n, what.c_str()); return 2; }
    std::fclose(f);
  }
  float* in = nullptr;
  void* workspace = nullptr;
  uint32_t *idsA = nullptr, *idsB = nullptr, *copyTo = nullptr, *countDev = nullptr;
  const size_t wsb = 3 * map_bytes(n) + compaction_bytes(n);
  LAB_TRY(hipMalloc(&in, (size_t)n * 4));
  LAB_TRY(hipMalloc(&workspace, wsb));
  LAB_TRY(hipMalloc(&idsA, (size_t)n * 4));
  LAB_TRY(hipMalloc(&idsB, (size_t)n * 4));
  LAB_TRY(hipMalloc(&copyTo, (size_t)n * 4));
  LAB_TRY(hipMalloc(&countDev, 4));
  LAB_TRY(hipMemcpy(in, host.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  const Plan plan(workspace, n);
  hipEvent_t e0, e1;
  LAB_TRY(hipEventCreate(&e0));
  LAB_TRY(hipEventCreate(&e1));
  auto elapsed = [&](float& ms) {
    hipError_t e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    return e;
  };

  // the passes before the reduction, once with every record counted and then with all of them written; the labelling is timed alone
  std::vector<float> labelMs;
  for (int k = 0; k <= repeats; ++k) {
    LAB_TRY(launch_mask(in, n, params.minHeight, plan, nullptr));
    LAB_TRY(hipEventRecord(e0, nullptr));
    svcc::label_components((const float*)plan.number, w, h, params.maxDiff, plan.labels, plan.counts, nullptr);
    float ms = 0;
    LAB_TRY(elapsed(ms));
    if (k) labelMs.push_back(ms);
  }
  const ObjKeep keep{plan.labels, plan.counts, 1u};
  uint32_t* totals = nullptr;
  LAB_TRY((svc::partition<1, kPerThread>(n, keep, ObjEmit{plan.counts, plan.number, nullptr, 0u}, plan.tables, &totals, nullptr)));
  uint32_t count = 0;
  LAB_TRY(hipMemcpy(&count, totals + 1, 4, hipMemcpyDeviceToHost));
  const size_t recordBytes = (size_t)std::max(count, 1u) * sizeof(ssrlcv_object_record);
  ssrlcv_object_record *fresh = nullptr, *recA = nullptr, *recB = nullptr;
  LAB_TRY(hipMalloc(&fresh, recordBytes));
  LAB_TRY(hipMalloc(&recA, recordBytes));
  LAB_TRY(hipMalloc(&recB, recordBytes));
  LAB_TRY((svc::partition<1, kPerThread>(n, keep, ObjEmit{plan.counts, plan.number, fresh, count}, plan.tables, &totals, nullptr)));
  LAB_TRY(hipDeviceSynchronize());

  Times t[3];
  for (int form = 0; form < 3; ++form) {  // 0 the shipped reduction, 1 the naive one, 2 a copy that moves the call's least bytes
    std::vector<float> ms;
    for (int k = 0; k <= repeats; ++k) {
      if (form < 2) LAB_TRY(hipMemcpyAsync(form ? recB : recA, fresh, recordBytes, hipMemcpyDeviceToDevice, nullptr));  // initialised records, not timed
      LAB_TRY(hipEventRecord(e0, nullptr));
      if (form == 0) {
        LAB_TRY(launch_reduce(in, w, h, params, plan, idsA, recA, count, nullptr));
      } else if (form == 1) {
        hipLaunchKernelGGL(k_obj_naive, dim3(capped((n + 255u) / 256u, kMaskGridCap)), dim3(256), 0, nullptr, (const uint32_t*)in, plan.labels, plan.counts,
                           plan.number, w, h, params.minHeight, params.scale, 1u, idsB, recB, count);
        LAB_TRY(hipGetLastError());
      } else {
        LAB_TRY(hipMemcpyAsync(copyTo, in, (size_t)n * 4, hipMemcpyDeviceToDevice, nullptr));  // the map read once, a map of the ids' size written
      }
      float v = 0;
      LAB_TRY(elapsed(v));
      if (k) ms.push_back(v);  // the first run warms up
    }
    t[form] = summary(ms);
  }
  std::vector<char> a(recordBytes), b(recordBytes);
  std::vector<uint32_t> ia(n), ib(n);
  LAB_TRY(hipMemcpy(a.data(), recA, recordBytes, hipMemcpyDeviceToHost));
  LAB_TRY(hipMemcpy(b.data(), recB, recordBytes, hipMemcpyDeviceToHost));
  LAB_TRY(hipMemcpy(ia.data(), idsA, (size_t)n * 4, hipMemcpyDeviceToHost));
  LAB_TRY(hipMemcpy(ib.data(), idsB, (size_t)n * 4, hipMemcpyDeviceToHost));
  const bool equal = std::memcmp(a.data(), b.data(), (size_t)count * sizeof(ssrlcv_object_record)) == 0 && ia == ib;
  const Times l = summary(labelMs);
  std::printf("%s %u x %u: %u objects; reduction %.4f ms (%.4f .. %.4f), naive %.4f ms (%.4f .. %.4f), labelling %.4f ms (%.4f .. %.4f), copy of 8 B a cell %.4f ms, "
              "equal %d\n", what.c_str(), w, h, count, t[0].med, t[0].lo, t[0].hi, t[1].med, t[1].lo, t[1].hi, l.med, l.lo, l.hi, t[2].med, (int)equal);
  (void)hipFree(in), (void)hipFree(workspace), (void)hipFree(idsA), (void)hipFree(idsB), (void)hipFree(copyTo), (void)hipFree(countDev);
  (void)hipFree(fresh), (void)hipFree(recA), (void)hipFree(recB);
  return equal ? 0 : 1;
}
