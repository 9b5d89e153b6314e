// tests/cpp/ortho_test.cpp -- the ortho-image through the class API: MeshFactory::generateOrthoImage on a height map, then
// setPointsFromHeightMap, setSurface(DisparityFactory::generateMesh(height, 1, inf)), setVertexColors and saveMesh.
//   ortho_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <height raw float32> <cameras raw (Image::Camera, 80 bytes each)> <maxSteps>
//              <bias> <rule> <out prefix> <image raw uint8>...
//     the map and the images start in host memory and must come back there.  Writes <prefix>.ortho, .seen, .which as raw bytes and
//     <prefix>.ply; prints "vertices <n>", then "ok".
#include <cmath>
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

static_assert(sizeof(ssrlcv_dsm_frame) == 60 && sizeof(ssrlcv_ortho_view) == 80 && sizeof(ssrlcv_ortho_params) == 12, "the ABI's sizes");

template <typename T>
static ptr::value<Unity<T>> load(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return ptr::value<Unity<T>>();
  std::fseek(f, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(f) / sizeof(T);
  std::fseek(f, 0, SEEK_SET);
  ptr::host<T> values((long)n, true);
  const size_t got = std::fread(values.get(), sizeof(T), n, f);
  std::fclose(f);
  if (got != n || n == 0) return ptr::value<Unity<T>>();
  return ptr::value<Unity<T>>(values, (unsigned long)n, cpu, true);
}

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
  if (argc < 9 || argc > 8 + 8) {
    std::fprintf(stderr, "usage: %s <frame raw> <height raw> <cameras raw> <maxSteps> <bias> <rule> <out prefix> <image raw>... (1 to 8)\n", argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  auto height = load<float>(argv[2]);
  CHECK(height != nullptr && height->size() == (unsigned long)frame.w * frame.h);
  const int m = argc - 8;
  std::vector<ssrlcv_camera> cameras((size_t)m);
  f = std::fopen(argv[3], "rb");
  if (!f || std::fread(cameras.data(), sizeof(ssrlcv_camera), (size_t)m, f) != (size_t)m) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  std::fclose(f);
  ssrlcv_ortho_params params;
  params.maxSteps = (uint32_t)std::atoi(argv[4]);
  params.bias = (float)std::atof(argv[5]);
  params.rule = (uint32_t)std::atoi(argv[6]);
  const std::string prefix = argv[7];
  std::vector<ptr::value<Unity<unsigned char>>> images;
  for (int k = 8; k < argc; ++k) {
    images.push_back(load<unsigned char>(argv[k]));
    CHECK(images.back() != nullptr);
  }

  ptr::value<Unity<unsigned char>> seen, which;
  auto ortho = MeshFactory::generateOrthoImage(height, frame, images, cameras, params, &seen, &which);
  CHECK(ortho != nullptr && seen != nullptr && which != nullptr && ortho->getMemoryState() == gpu);
  CHECK(height->getMemoryState() == cpu);
  for (auto& image : images) CHECK(image->getMemoryState() == cpu);
  CHECK(dump(prefix + ".ortho", ortho) && dump(prefix + ".seen", seen) && dump(prefix + ".which", which));
  // a wrong image size and a ninth view are refused
  std::vector<ptr::value<Unity<unsigned char>>> one(1, load<unsigned char>(argv[3]));  // the cameras' bytes: not the view's size
  CHECK(MeshFactory::generateOrthoImage(height, frame, one, std::vector<ssrlcv_camera>(1, cameras[0]), params) == nullptr);
  CHECK(MeshFactory::generateOrthoImage(height, frame, std::vector<ptr::value<Unity<unsigned char>>>(9, images[0]),
                                        std::vector<ssrlcv_camera>(9, cameras[0]), params) == nullptr);

  MeshFactory mesh;
  mesh.setPointsFromHeightMap(height, frame);
  CHECK(mesh.points != nullptr && mesh.colors == nullptr);
  DisparityFactory factory(2u);
  factory.setMapSize(frame.w, frame.h);
  mesh.setSurface(factory.generateMesh(height, 1u, INFINITY));
  CHECK(mesh.hasSurface);
  mesh.setVertexColors(ortho, height);
  CHECK(mesh.colors != nullptr && mesh.colors->size() == mesh.points->size() && ortho->getMemoryState() == gpu);
  std::printf("vertices %lu\n", mesh.points->size());
  const size_t slash = prefix.find_last_of('/');
  mesh.saveMesh(prefix.substr(slash + 1), prefix.substr(0, slash + 1));
  std::printf("ok\n");
  return 0;
}
