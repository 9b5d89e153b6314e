// tests/cpp/accuracy_test.cpp -- surface accuracy through the class API: MeshFactory::setReferenceSurface, then
// calculatePerPointDifference, calculateAverageDifference and accuracyReport of a cloud against it.
//   accuracy_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <reference height raw float32 x w h> <cloud raw float32 x 3> <maxJump> <out prefix>
//     the cloud starts in host memory and must come back there.  A plane normal that is not the frame's ez must be refused.
//     Writes <prefix>.diff (float32 a point) and <prefix>.report (12 float64: n, coverage, bias, nmad, mean, rms, le68, le90, le95,
//     min, max, calculateAverageDifference); prints the report, then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(ssrlcv_diff_stats) == 72 && sizeof(ssrlcv_diff_stats_params) == 44, "the records of surface accuracy");

template <typename T>
static ptr::value<Unity<T>> load(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return ptr::value<Unity<T>>();
  std::fseek(f, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(f) / sizeof(T);
  std::fseek(f, 0, SEEK_SET);
  if (n == 0) { std::fclose(f); return ptr::value<Unity<T>>(); }
  ptr::host<T> values((long)n, true);
  const size_t got = std::fread(values.get(), sizeof(T), n, f);
  std::fclose(f);
  if (got != n) return ptr::value<Unity<T>>();
  return ptr::value<Unity<T>>(values, (unsigned long)n, cpu, true);
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <frame raw> <reference height raw> <cloud raw> <maxJump> <out prefix>\n", argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  auto height = load<float>(argv[2]);
  auto cloud = load<float3>(argv[3]);
  if (height == nullptr || cloud == nullptr) { std::fprintf(stderr, "cannot read the map or the cloud\n"); return 2; }
  const float maxJump = (float)std::atof(argv[4]);
  const std::string prefix = argv[5];

  MeshFactory factory;
  CHECK(factory.calculatePerPointDifference(cloud, {frame.ez[0], frame.ez[1], frame.ez[2]}) == nullptr);  // no reference yet
  factory.setReferenceSurface(height, frame, maxJump);
  CHECK(factory.hasReference && height->getMemoryState() == cpu);
  const float3 ez = {frame.ez[0], frame.ez[1], frame.ez[2]};
  CHECK(factory.calculatePerPointDifference(cloud, {frame.ex[0], frame.ex[1], frame.ex[2]}) == nullptr);   // another direction is refused
  CHECK(factory.calculatePerPointDifference(cloud, {-ez.x, -ez.y, -ez.z}) == nullptr);
  CHECK(factory.calculatePerPointDifference(cloud, {0.0f, 0.0f, 0.0f}) == nullptr);
  auto scaled = factory.calculatePerPointDifference(cloud, {3.0f * ez.x, 3.0f * ez.y, 3.0f * ez.z});      // the direction counts, not the length
  CHECK(scaled != nullptr && scaled->size() == cloud->size() && scaled->getMemoryState() == gpu && cloud->getMemoryState() == cpu);

  ptr::value<Unity<float>> diff;
  const MeshFactory::AccuracyReport r = factory.accuracyReport(cloud, &diff);
  CHECK(diff != nullptr && diff->size() == cloud->size() && r.n == cloud->size() && cloud->getMemoryState() == cpu);
  const double average = factory.calculateAverageDifference(cloud, ez);
  std::printf("n %lu coverage %.6f bias %.6f nmad %.6f mean %.6f rms %.6f le68 %.6f le90 %.6f le95 %.6f min %.6f max %.6f average %.6f\n", r.n,
              r.coverage, r.bias, r.nmad, r.mean, r.rms, r.le68, r.le90, r.le95, r.min, r.max, average);
  diff->setMemoryState(cpu);
  scaled->setMemoryState(cpu);
  for (unsigned long k = 0; k < diff->size(); ++k) {
    uint32_t a, b;
    std::memcpy(&a, diff->host.get() + k, 4);
    std::memcpy(&b, scaled->host.get() + k, 4);
    CHECK(a == b);
  }
  f = std::fopen((prefix + ".diff").c_str(), "wb");
  CHECK(f && std::fwrite(diff->host.get(), sizeof(float), diff->size(), f) == diff->size());
  std::fclose(f);
  const double fields[12] = {(double)r.n, r.coverage, r.bias, r.nmad, r.mean, r.rms, r.le68, r.le90, r.le95, r.min, r.max, average};
  f = std::fopen((prefix + ".report").c_str(), "wb");
  CHECK(f && std::fwrite(fields, sizeof(double), 12, f) == 12);
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
