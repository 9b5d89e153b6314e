// tests/cpp/sift_rerun_test.cpp -- the capacity re-run loop of SIFT_FeatureFactory::generateFeatures through the class API.
//   sift_rerun_test <perOctave> <W> <H> <raw u8 file> <out file> [<raw u8 file> <out file> ...]     (GPU)
// ONE factory with setMaxKeyPointsPerOctave(perOctave) runs every image (all W x H, pixels in host memory) in turn through
// generateFeatures(image, false, 2) and writes each image's feature records to its <out file>.  Prints "image <k> count <n>" per
// image, then "ok".  With SSRLCV_LOG set the factory logs one "[warn] key-point capacity exceeded" line per re-run to
// stderr, between the "[info] Generating SIFT features for image <k>" lines (tests/test_gpu_overflow.py counts them).
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
  if (argc < 6 || (argc - 4) % 2 != 0) {
    std::fprintf(stderr, "usage: %s <perOctave> <W> <H> <raw u8 file> <out file> [<raw u8 file> <out file> ...]\n", argv[0]);
    return 2;
  }
  const unsigned perOctave = (unsigned)std::atoi(argv[1]), W = (unsigned)std::atoi(argv[2]), H = (unsigned)std::atoi(argv[3]);
  SIFT_FeatureFactory factory(1.5f, 6.0f);
  factory.setMaxKeyPointsPerOctave(perOctave);
  for (int k = 0; 4 + 2 * k + 1 < argc; ++k) {
    std::FILE* f = std::fopen(argv[4 + 2 * k], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[4 + 2 * k]); return 2; }
    ptr::host<unsigned char> px((long)W * H, true);
    const size_t got = std::fread(px.get(), 1, (size_t)W * H, f);
    std::fclose(f);
    CHECK(got == (size_t)W * H);
    ptr::value<Unity<unsigned char>> pixels(px, (unsigned long)W * H, cpu, true);
    ptr::value<Image> image(uint2{W, H}, 1u, pixels);
    image->id = k;
    auto feats = factory.generateFeatures(image, false, 2);
    CHECK(image->pixels->getMemoryState() == cpu);  // origin state restored
    CHECK(feats->getMemoryState() == gpu);
    feats->transferMemoryTo(cpu);
    std::FILE* o = std::fopen(argv[4 + 2 * k + 1], "wb");
    CHECK(o != nullptr);
    const size_t n = feats->size();
    const bool ok = std::fwrite(feats->host.get(), sizeof(Feature<SIFT_Descriptor>), n, o) == n;
    std::fclose(o);
    CHECK(ok);
    std::printf("image %d count %lu\n", k, (unsigned long)n);
  }
  std::printf("ok\n");
  return 0;
}
