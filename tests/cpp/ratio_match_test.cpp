// tests/cpp/ratio_match_test.cpp -- MatchFactory's ratio / mutual matchers through the class API.
//   ratio_match_test <pair.bin> <ratio> <mutual 0|1> <absolute threshold> <out prefix>     (GPU)
// pair.bin: uint64 nq, uint64 nt, nq + nt ssrlcv_sift_feature.  Writes the validated arrays of generateMatchesRatio,
// generateDistanceMatchesRatio and generateMatchesRatioIndexOnly to <prefix>.match / .dmatch / .pairs, prints their
// three counts, then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <typename OUT>
static int dump(const std::string& path, ptr::value<Unity<OUT>> m) {
  m->transferMemoryTo(cpu);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t n = m->size();
  const bool ok = std::fwrite(m->host.get(), sizeof(OUT), n, f) == n;
  std::fclose(f);
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s <pair.bin> <ratio> <mutual> <absolute> <out prefix>\n", argv[0]); return 2; }
  const float ratio = (float)std::atof(argv[2]);
  const bool mutual = std::atoi(argv[3]) != 0;
  const float absolute = (float)std::atof(argv[4]);
  const std::string prefix = argv[5];
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint64_t n[2] = {0, 0};
  CHECK(std::fread(n, sizeof n, 1, f) == 1);
  ptr::value<Unity<Feature<SIFT_Descriptor>>> feats[2];
  ptr::value<Image> images[2];
  for (int i = 0; i < 2; ++i) {
    feats[i] = ptr::value<Unity<Feature<SIFT_Descriptor>>>(nullptr, (unsigned long)n[i], cpu);
    CHECK(std::fread(feats[i]->host.get(), sizeof(Feature<SIFT_Descriptor>), n[i], f) == n[i]);
    images[i].construct();
    images[i]->id = 3 + 2 * i;  // (ids 3 and 5: not the indices)
  }
  std::fclose(f);
  MatchFactory<SIFT_Descriptor> factory(0.6f, absolute);
  auto m = factory.generateMatchesRatio(images[0], feats[0], images[1], feats[1], ratio, mutual);
  auto d = factory.generateDistanceMatchesRatio(images[0], feats[0], images[1], feats[1], ratio, mutual);
  auto p = factory.generateMatchesRatioIndexOnly(images[0], feats[0], images[1], feats[1], ratio, mutual);
  CHECK(feats[0]->getMemoryState() == cpu && feats[1]->getMemoryState() == cpu);  // origin state restored
  CHECK(dump(prefix + ".match", m) == 0 && dump(prefix + ".dmatch", d) == 0 && dump(prefix + ".pairs", p) == 0);
  std::printf("counts %lu %lu %lu\n", (unsigned long)m->size(), (unsigned long)d->size(), (unsigned long)p->size());
  std::printf("ok\n");
  return 0;
}
