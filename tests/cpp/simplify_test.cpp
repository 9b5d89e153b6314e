// tests/cpp/simplify_test.cpp -- the surface simplification through the class API: MeshFactory::setPointsFromHeightMap, the full
// surface and its normals (setSurface, computeSurfaceNormals), then simplifySurface(tolerance) and saveMesh.
//   simplify_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <height raw float32, frame.w x frame.h> <tolerance> <out dir> <name>
//     the map starts in host memory and must come back there.  Writes <out dir><name>.ply and <out dir><name>.faces (raw uint32 x 3);
//     prints "full <n> <t>", "vertices <m> faces <t>", then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(ssrlcv_dsm_frame) == 60, "the frame is 60 bytes");

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <frame raw> <height raw> <tolerance> <out dir> <name>\n", argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  const size_t cells = (size_t)frame.w * frame.h;
  ptr::host<float> values((long)cells, true);
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(values.get(), sizeof(float), cells, f) != cells) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  std::fclose(f);
  const float tolerance = (float)std::atof(argv[3]);
  const std::string dir = argv[4], name = argv[5];
  ptr::value<Unity<float>> height(values, (unsigned long)cells, cpu, true);

  MeshFactory mesh;
  CHECK(mesh.simplifySurface(tolerance) == 0);  // nothing to simplify yet
  mesh.setPointsFromHeightMap(height, frame);
  CHECK(mesh.points != nullptr && height->getMemoryState() == cpu);
  DisparityFactory factory(2u);
  factory.setMapSize(frame.w, frame.h);
  mesh.setSurface(factory.generateMesh(height, 1u, std::numeric_limits<float>::infinity()));
  CHECK(mesh.hasSurface);
  mesh.computeSurfaceNormals();
  auto full = mesh.faces();
  CHECK(mesh.normals != nullptr && full != nullptr);
  const unsigned long n = mesh.points->size();
  std::printf("full %lu %lu\n", n, full->size());

  const unsigned long t = mesh.simplifySurface(tolerance);
  CHECK(t > 0 && mesh.hasSimplified && !mesh.hasSurface);
  auto faces = mesh.faces();
  CHECK(faces != nullptr && faces->size() == t && mesh.points->size() <= n);
  CHECK(mesh.normals != nullptr && mesh.normals->size() == mesh.points->size());  // the full-resolution normals, gathered
  // a triangle list is no grid mesh: these leave everything as it is
  auto before = mesh.normals;
  mesh.computeSurfaceNormals();
  CHECK(mesh.normals == before);
  Image::Camera camera = {};
  CHECK(mesh.renderView(camera, frame).depth == nullptr);
  CHECK(mesh.simplifySurface(tolerance) == 0 && mesh.faces()->size() == t);
  std::printf("vertices %lu faces %lu\n", mesh.points->size(), t);

  mesh.saveMesh(name, dir);
  faces->setMemoryState(cpu);
  f = std::fopen((dir + name + ".faces").c_str(), "wb");
  CHECK(f && std::fwrite(faces->host.get(), sizeof(uint3), faces->size(), f) == faces->size());
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
