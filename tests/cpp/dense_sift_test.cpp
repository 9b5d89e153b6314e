// tests/cpp/dense_sift_test.cpp -- SIFT_FeatureFactory::generateFeatures(image, dense = true, ..) through the class API.
//   dense_sift_test <raw u8 file> <W> <H> <stride> <out file>     (GPU)
// Pixels start in host memory; writes the feature records of generateFeatures(image, true, 2) with setDenseStride(stride)
// to <out file>, prints their count, then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s <raw u8 file> <W> <H> <stride> <out file>\n", argv[0]); return 2; }
  const unsigned W = (unsigned)std::atoi(argv[2]), H = (unsigned)std::atoi(argv[3]), stride = (unsigned)std::atoi(argv[4]);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  ptr::host<unsigned char> px((long)W * H, true);
  const size_t got = std::fread(px.get(), 1, (size_t)W * H, f);
  std::fclose(f);
  CHECK(got == (size_t)W * H);
  ptr::value<Unity<unsigned char>> pixels(px, (unsigned long)W * H, cpu, true);
  ptr::value<Image> image(uint2{W, H}, 1u, pixels);
  image->id = 0;
  SIFT_FeatureFactory factory(1.5f, 6.0f);
  factory.setDenseStride(stride);
  auto feats = factory.generateFeatures(image, true, 2);
  CHECK(image->pixels->getMemoryState() == cpu);  // origin state restored
  CHECK(feats->getMemoryState() == gpu);
  feats->transferMemoryTo(cpu);
  std::FILE* o = std::fopen(argv[5], "wb");
  CHECK(o != nullptr);
  const size_t n = feats->size();
  const bool ok = std::fwrite(feats->host.get(), sizeof(Feature<SIFT_Descriptor>), n, o) == n;
  std::fclose(o);
  CHECK(ok);
  std::printf("count %lu\n", (unsigned long)n);
  std::printf("ok\n");
  return 0;
}
