// tests/cpp/register_test.cpp -- surface registration through the class API: MeshFactory::setReferenceSurface, then
// registerToReference of a cloud against it, and PointCloudFactory::transformPointCloud with the pose it found.
//   register_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <reference height raw float32 x w h> <cloud raw float32 x 3> <maxJump>
//                 <dofMask> <iterations> <gateFactor, 0 = no gate> <out prefix>
//     the cloud starts in host memory and must come back there.  Writes <prefix>.pose (the 60 bytes of ssrlcv_register_pose),
//     <prefix>.history (12 float64 an iteration: used, inside, rms, center, gate, delta[7]; NaN deltas for a refused step) and
//     <prefix>.points (the cloud under the pose, float32 x 3); prints the history, then "ok".
//     The host wrappers scalePointCloud, translatePointCloud and rotatePointCloud are checked on three points on the way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(ssrlcv_register_pose) == 60 && sizeof(ssrlcv_register_params) == 8 && sizeof(ssrlcv_register_terms) == 304,
              "the records of surface registration");

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

static bool near(float3 a, float x, float y, float z) { return std::fabs(a.x - x) < 1e-5f && std::fabs(a.y - y) < 1e-5f && std::fabs(a.z - z) < 1e-5f; }

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s <frame raw> <reference height raw> <cloud raw> <maxJump> <dofMask> <iterations> <gateFactor> <out prefix>\n", argv[0]);
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
  const uint32_t dofMask = (uint32_t)std::atoi(argv[5]);
  const unsigned iterations = (unsigned)std::atoi(argv[6]);
  const float gateFactor = (float)std::atof(argv[7]);
  const std::string prefix = argv[8];

  PointCloudFactory clouds;
  {  // the host wrappers: x east turned about z by a quarter goes north; a "no result" point stays one
    ptr::host<float3> three(3);
    three.get()[0] = {1.0f, 0.0f, 0.0f}, three.get()[1] = {0.0f, 0.0f, 0.0f}, three.get()[2] = {1.0f, 2.0f, 3.0f};
    ptr::value<Unity<float3>> small(three, 3, cpu);
    clouds.rotatePointCloud({0.0f, 0.0f, 1.57079632679f}, small);
    CHECK(small->getMemoryState() == cpu && near(small->host.get()[0], 0, 1, 0) && near(small->host.get()[2], -2, 1, 3));
    clouds.scalePointCloud(2.0f, small);
    clouds.translatePointCloud({1.0f, 1.0f, 1.0f}, small);
    CHECK(near(small->host.get()[0], 1, 3, 1) && near(small->host.get()[2], -3, 3, 7) && near(small->host.get()[1], 0, 0, 0));
  }

  MeshFactory factory;
  CHECK(factory.registerToReference(cloud).history.empty());  // no reference yet
  factory.setReferenceSurface(height, frame, maxJump);
  CHECK(factory.hasReference);
  const MeshFactory::Registration reg = factory.registerToReference(cloud, dofMask, iterations, gateFactor);
  CHECK(cloud->getMemoryState() == cpu && !reg.history.empty() && reg.history.size() <= iterations);
  std::vector<double> rows;
  for (const MeshFactory::RegistrationStep& s : reg.history) {
    std::printf("used %u inside %u rms %.6f center %.6f gate %.6f%s\n", s.used, s.inside, s.rms, s.center, s.gate, s.stepped ? "" : " (refused)");
    rows.push_back(s.used), rows.push_back(s.inside), rows.push_back(s.rms), rows.push_back(s.center), rows.push_back(s.gate);
    for (int k = 0; k < 7; ++k) rows.push_back(s.stepped ? s.delta[k] : std::numeric_limits<double>::quiet_NaN());
  }
  clouds.transformPointCloud(cloud, reg.pose);
  CHECK(cloud->getMemoryState() == cpu);
  f = std::fopen((prefix + ".pose").c_str(), "wb");
  CHECK(f && std::fwrite(&reg.pose, sizeof reg.pose, 1, f) == 1);
  std::fclose(f);
  f = std::fopen((prefix + ".history").c_str(), "wb");
  CHECK(f && std::fwrite(rows.data(), sizeof(double), rows.size(), f) == rows.size());
  std::fclose(f);
  f = std::fopen((prefix + ".points").c_str(), "wb");
  CHECK(f && std::fwrite(cloud->host.get(), sizeof(float3), cloud->size(), f) == cloud->size());
  std::fclose(f);
  std::printf("converged %d\nok\n", reg.converged ? 1 : 0);
  return 0;
}
