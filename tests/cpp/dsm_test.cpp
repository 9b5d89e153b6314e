// tests/cpp/dsm_test.cpp -- the surface model through the class API: MeshFactory::generateHeightMap per cloud, fuseHeightMaps,
// setPointsFromHeightMap and setSurface(DisparityFactory::generateMesh(height, 1, maxJump)), then the surface normals and faces.
//   dsm_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <minViews> <maxSpread> <maxJump> <out prefix> <cloud raw float32 x 3>...
//     the clouds start in host memory and must come back there.  Rule MAX per cloud, the lower MEDIAN across the maps.  Writes
//     <prefix>.map<k>, .fused, .views, .points, .faces, .normals as raw bytes; prints "vertices <n> faces <t>", then "ok".
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

static_assert(sizeof(ssrlcv_dsm_frame) == 60, "the frame is 60 bytes");

template <typename T>
static bool dump(const std::string& path, ptr::value<Unity<T>> u) {
  MemoryState origin = u->getMemoryState();
  if (origin != cpu) u->setMemoryState(cpu);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(u->host.get(), sizeof(T), u->size(), f) == u->size();
  std::fclose(f);
  if (origin != cpu) u->setMemoryState(origin);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 7 || argc > 6 + 8) {
    std::fprintf(stderr, "usage: %s <frame raw> <minViews> <maxSpread> <maxJump> <out prefix> <cloud raw>... (1 to 8)\n", argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  const unsigned minViews = (unsigned)std::atoi(argv[2]);
  const float maxSpread = (float)std::atof(argv[3]), maxJump = (float)std::atof(argv[4]);
  const std::string prefix = argv[5];

  std::vector<ptr::value<Unity<float>>> maps;
  for (int k = 6; k < argc; ++k) {
    f = std::fopen(argv[k], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / sizeof(float3);
    std::fseek(f, 0, SEEK_SET);
    ptr::host<float3> values((long)n, true);
    const size_t got = std::fread(values.get(), sizeof(float3), n, f);
    std::fclose(f);
    if (got != n || n == 0) { std::fprintf(stderr, "short read of %s\n", argv[k]); return 2; }
    ptr::value<Unity<float3>> cloud(values, (unsigned long)n, cpu, true);
    MeshFactory one(cloud);
    auto height = one.generateHeightMap(frame, 0u);
    CHECK(height != nullptr && height->size() == (unsigned long)frame.w * frame.h && height->getMemoryState() == gpu);
    CHECK(cloud->getMemoryState() == cpu);
    CHECK(dump(prefix + ".map" + std::to_string(k - 6), height));
    maps.push_back(height);
  }

  ptr::value<Unity<unsigned char>> views;
  auto fused = MeshFactory::fuseHeightMaps(maps, frame.w, frame.h, minViews, maxSpread, 1u, &views);
  CHECK(fused != nullptr && views != nullptr && fused->getMemoryState() == gpu);
  CHECK(dump(prefix + ".fused", fused) && dump(prefix + ".views", views));

  MeshFactory mesh;
  mesh.setPointsFromHeightMap(fused, frame);
  CHECK(mesh.points != nullptr);
  DisparityFactory factory(2u);
  factory.setMapSize(frame.w, frame.h);
  mesh.setSurface(factory.generateMesh(fused, 1u, maxJump));
  CHECK(mesh.hasSurface && mesh.surface.vertexCount == mesh.points->size());
  mesh.computeSurfaceNormals();
  auto faces = mesh.faces();
  CHECK(mesh.normals != nullptr && faces != nullptr);
  std::printf("vertices %lu faces %lu\n", mesh.points->size(), faces->size());
  CHECK(dump(prefix + ".points", mesh.points) && dump(prefix + ".normals", mesh.normals) && dump(prefix + ".faces", faces));
  std::printf("ok\n");
  return 0;
}
