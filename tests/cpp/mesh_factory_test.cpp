// tests/cpp/mesh_factory_test.cpp -- MeshFactory through the reference's class API.
//   mesh_factory_test ply <dir>                      (no GPU) writePLY with normals of three fixed points -> <dir>/tri.ply
//   mesh_factory_test run <cloud.bin> <dir> <k> <sigma> <vx> <vy> <vz>
//       (GPU) cloud.bin: uint64 n, n float3.  setPoints -> filterByNeighborDistance(k, sigma) -> computeNormals(k, v)
//       -> savePoints("cloud", dir).  Prints "stats <mu> <std> <t>", "kept <count>", then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(float3) == sizeof(ssrlcv_float3), "float3 layout");

int main(int argc, char** argv) {
  if (argc >= 3 && std::string(argv[1]) == "ply") {
    ptr::value<Unity<float3>> p(nullptr, 3ul, cpu), n(nullptr, 3ul, cpu);
    const float3 pv[3] = {{6371.00049f, -0.1f, 1e-7f}, {1.0f / 3.0f, 2.5f, -3.25e5f}, {0.0f, -0.0f, 123456.789f}};
    const float3 nv[3] = {{0.0f, 0.0f, 1.0f}, {0.577350269f, -0.577350269f, 0.577350269f}, {0.0f, 0.0f, 0.0f}};
    for (int i = 0; i < 3; ++i) p->host.get()[i] = pv[i], n->host.get()[i] = nv[i];
    writePLY("tri", p, n, std::string(argv[2]) + "/");
    CHECK(p->getMemoryState() == cpu && n->getMemoryState() == cpu);
    std::printf("ok\n");
    return 0;
  }
  if (argc < 9 || std::string(argv[1]) != "run") {
    std::fprintf(stderr, "usage: %s ply <dir> | run <cloud.bin> <dir> <k> <sigma> <vx> <vy> <vz>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  uint64_t n = 0;
  CHECK(std::fread(&n, sizeof n, 1, f) == 1);
  ptr::value<Unity<float3>> points(nullptr, (unsigned long)n, cpu);
  CHECK(std::fread(points->host.get(), sizeof(float3), n, f) == n);
  std::fclose(f);
  const int k = std::atoi(argv[4]);
  const float sigma = (float)std::atof(argv[5]);
  const float3 v = {(float)std::atof(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8])};
  MeshFactory mesh;
  mesh.setPoints(points);
  ptr::value<Unity<float>> mean = mesh.calculateAverageDistancesToNeighbors(k);
  CHECK(mean != nullptr && mean->size() == n && mean->getMemoryState() == cpu && points->getMemoryState() == cpu);
  mesh.filterByNeighborDistance(k, sigma);
  CHECK(mesh.points != nullptr && mesh.points->getMemoryState() == cpu);
  std::printf("stats %.17g %.17g %.17g\n", mesh.filterStats[0], mesh.filterStats[1], mesh.filterStats[2]);
  std::printf("kept %lu\n", mesh.points->size());
  mesh.computeNormals(k, v);
  CHECK(mesh.normals != nullptr && mesh.normals->size() == mesh.points->size() && mesh.normals->getMemoryState() == cpu);
  mesh.savePoints("cloud", std::string(argv[3]) + "/");
  std::printf("ok\n");
  return 0;
}
