// tests/cpp/render_test.cpp -- mesh render through the class API: MeshFactory::setPointsFromHeightMap, setSurface of
// DisparityFactory::generateMesh(height, 1, maxJump), setVertexColors of an ortho-image, then renderView into a camera and
// photoConsistency against that camera's picture.
//   render_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <height raw float32 x w h> <ortho raw uint8 x w h> <image raw uint8>
//               <camera raw (Image::Camera, 80 bytes)> <maxJump> <maxExtent> <out prefix>
//     the maps and the image start in host memory and must come back there.  Writes <prefix>.depth, .triangle, .shade and
//     .residual as raw maps and <prefix>.figures (7 float64: coverage, median, nmad, rms, drawn, too large, unusable); prints the
//     figures, then "ok".
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

static_assert(sizeof(ssrlcv_render_params) == 4 && sizeof(ssrlcv_ortho_view) == 80 && sizeof(Image::Camera) == 80, "the ABI's sizes");

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
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s <frame raw> <height raw> <ortho raw> <image raw> <camera raw> <maxJump> <maxExtent> <out prefix>\n", argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  auto height = load<float>(argv[2]);
  auto ortho = load<unsigned char>(argv[3]);
  auto image = load<unsigned char>(argv[4]);
  CHECK(height != nullptr && ortho != nullptr && image != nullptr && height->size() == (unsigned long)frame.w * frame.h && ortho->size() == height->size());
  Image::Camera camera;
  f = std::fopen(argv[5], "rb");
  if (!f || std::fread(&camera, sizeof camera, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
  std::fclose(f);
  const float maxJump = (float)std::atof(argv[6]);
  const uint32_t maxExtent = (uint32_t)std::atoi(argv[7]);
  const std::string prefix = argv[8];

  MeshFactory mesh;
  CHECK(mesh.renderView(camera, frame).depth == nullptr);  // no points, no surface
  mesh.setPointsFromHeightMap(height, frame);
  CHECK(mesh.points != nullptr && mesh.renderView(camera, frame).depth == nullptr);  // no surface yet
  DisparityFactory factory(2u);
  factory.setMapSize(frame.w, frame.h);
  mesh.setSurface(factory.generateMesh(height, 1u, maxJump));
  CHECK(mesh.hasSurface);
  CHECK(mesh.renderView(camera, frame, 0).depth == nullptr && mesh.renderView(camera, frame, 65).depth == nullptr);  // refused, not fatal
  const MeshFactory::RenderedView plain = mesh.renderView(camera, frame, maxExtent);  // without colours: the greys count as 0
  CHECK(plain.depth != nullptr && plain.drawn > 0);
  mesh.setVertexColors(ortho, height);
  CHECK(mesh.colors != nullptr && mesh.colors->getMemoryState() == cpu);
  const MeshFactory::PhotoConsistency p = mesh.photoConsistency(image, camera, frame, maxExtent);
  CHECK(p.residual != nullptr && p.view.depth != nullptr && p.view.w == camera.size.x && p.view.h == camera.size.y);
  CHECK(image->getMemoryState() == cpu && height->getMemoryState() == cpu && mesh.colors->getMemoryState() == cpu);
  CHECK(p.view.drawn == plain.drawn && p.view.tooLarge == plain.tooLarge && p.view.unusable == plain.unusable);
  CHECK(mesh.photoConsistency(ortho, camera, frame, maxExtent).residual == nullptr || ortho->size() == image->size());  // a wrong image size
  CHECK(dump(prefix + ".depth", p.view.depth) && dump(prefix + ".triangle", p.view.triangle) && dump(prefix + ".shade", p.view.shade) &&
        dump(prefix + ".residual", p.residual));
  const double figures[7] = {p.coverage, p.median, p.nmad, p.rms, (double)p.view.drawn, (double)p.view.tooLarge, (double)p.view.unusable};
  f = std::fopen((prefix + ".figures").c_str(), "wb");
  CHECK(f && std::fwrite(figures, sizeof(double), 7, f) == 7);
  std::fclose(f);
  std::printf("coverage %.6f median %.1f nmad %.4f rms %.4f drawn %u too large %u unusable %u\nok\n", p.coverage, p.median, p.nmad, p.rms, p.view.drawn,
              p.view.tooLarge, p.view.unusable);
  return 0;
}
