// tests/cpp/fill_test.cpp -- hole filling through the class API: DisparityFactory::fillHoles.
//   fill_test <map raw float32> <W> <H> <paths> <maxGap> <minHits> <rule> <out prefix>
//     the map starts in host memory and must come back there; fillHoles once without and once with the mask (the two maps must
//     agree).  Writes <prefix>.filled (float32 W x H) and <prefix>.mask (uint8), prints one FNV-1a checksum line per file and "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <typename T>
static bool dump(const std::string& path, const char* what, const T* data, size_t n) {
  std::FILE* o = std::fopen(path.c_str(), "wb");
  if (!o) return false;
  const bool ok = std::fwrite(data, sizeof(T), n, o) == n;
  std::fclose(o);
  unsigned long long hash = 1469598103934665603ull;  // FNV-1a over the bytes
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(data);
  for (size_t i = 0; i < n * sizeof(T); ++i) hash = (hash ^ bytes[i]) * 1099511628211ull;
  std::printf("%s %016llx\n", what, hash);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 9) {
    std::fprintf(stderr, "usage: %s <map float32> <W> <H> <paths> <maxGap> <minHits> <rule> <prefix>\n", argv[0]);
    return 2;
  }
  const unsigned W = (unsigned)std::atoi(argv[2]), H = (unsigned)std::atoi(argv[3]);
  const unsigned paths = (unsigned)std::strtoul(argv[4], nullptr, 0), maxGap = (unsigned)std::strtoul(argv[5], nullptr, 0);
  const unsigned minHits = (unsigned)std::atoi(argv[6]), rule = (unsigned)std::atoi(argv[7]);
  const std::string prefix = argv[8];
  const size_t n = (size_t)W * H;

  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  ptr::host<float> values((long)n, true);
  const size_t got = std::fread(values.get(), sizeof(float), n, f);
  std::fclose(f);
  if (got != n) { std::fprintf(stderr, "short read of %s\n", argv[1]); return 2; }
  ptr::value<Unity<float>> disparity(values, (unsigned long)n, cpu, true);

  DisparityFactory factory(2u);
  factory.setMapSize(W, H);
  auto plain = factory.fillHoles(disparity, paths, maxGap, minHits, rule);
  CHECK(plain->getMemoryState() == gpu && plain->size() == n && disparity->getMemoryState() == cpu);
  ptr::value<Unity<unsigned char>> mask;
  auto filled = factory.fillHoles(disparity, paths, maxGap, minHits, rule, &mask);
  CHECK(filled->getMemoryState() == gpu && mask != nullptr && mask->getMemoryState() == gpu && mask->size() == n);
  plain->transferMemoryTo(cpu);
  filled->transferMemoryTo(cpu);
  mask->transferMemoryTo(cpu);
  CHECK(std::memcmp(plain->host.get(), filled->host.get(), n * sizeof(float)) == 0);
  CHECK(dump(prefix + ".filled", "filled", filled->host.get(), n));
  CHECK(dump(prefix + ".mask", "mask", mask->host.get(), n));
  std::printf("ok\n");
  return 0;
}
