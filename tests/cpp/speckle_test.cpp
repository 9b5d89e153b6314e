// tests/cpp/speckle_test.cpp -- the disparity post-filters through the class API: DisparityFactory::medianFilter + filterSpeckles.
//   speckle_test <left raw u8> <right raw u8> <W> <H> <radius> <dmin> <D> <median radius> <maxSpeckleSize> <maxDiff> <out prefix>
//     pixels start in host memory; block matching without the left-right check, then the median of the map (a new map), then
//     the speckle filter in place on the median's map and on the cost map, both moved to the cpu first: they must come back
//     there.  Writes <prefix>.disparity, <prefix>.median, <prefix>.speckle.disparity (float32 W x H) and <prefix>.speckle.cost
//     (uint32), prints one FNV-1a checksum line per file and "ok".
#include <cstdio>
#include <cstdlib>
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

static ptr::value<Image> load(const char* path, unsigned W, unsigned H, int id) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
  ptr::host<unsigned char> px((long)W * H, true);
  const size_t got = std::fread(px.get(), 1, (size_t)W * H, f);
  std::fclose(f);
  if (got != (size_t)W * H) { std::fprintf(stderr, "short read of %s\n", path); std::exit(2); }
  ptr::value<Unity<unsigned char>> pixels(px, (unsigned long)W * H, cpu, true);
  ptr::value<Image> image(uint2{W, H}, 1u, pixels);
  image->id = id;
  return image;
}

int main(int argc, char** argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s <left> <right> <W> <H> <radius> <dmin> <D> <median radius> <maxSpeckleSize> <maxDiff> <prefix>\n", argv[0]);
    return 2;
  }
  const unsigned W = (unsigned)std::atoi(argv[3]), H = (unsigned)std::atoi(argv[4]);
  ptr::value<Image> left = load(argv[1], W, H, 0), right = load(argv[2], W, H, 1);
  DisparityFactory factory((unsigned)std::atoi(argv[5]));
  factory.setDisparityRange(std::atoi(argv[6]), (unsigned)std::atoi(argv[7]));
  factory.setLeftRightTolerance(-1);
  const unsigned medianRadius = (unsigned)std::atoi(argv[8]), maxSpeckleSize = (unsigned)std::atoi(argv[9]);
  const float maxDiff = (float)std::atof(argv[10]);
  const std::string prefix = argv[11];

  ptr::value<Unity<unsigned int>> cost;
  auto disparity = factory.generateDisparities(left, right, &cost);
  CHECK(disparity->getMemoryState() == gpu && disparity->size() == (unsigned long)W * H);

  auto median = factory.medianFilter(disparity, medianRadius);
  CHECK(median->getMemoryState() == gpu && median->size() == disparity->size() && disparity->getMemoryState() == gpu);
  disparity->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".disparity", "disparity", disparity->host.get(), disparity->size()));

  median->setMemoryState(cpu);  // the filters force their maps onto the gpu and restore them
  cost->setMemoryState(cpu);
  CHECK(dump(prefix + ".median", "median", median->host.get(), median->size()));
  factory.filterSpeckles(median, cost, maxSpeckleSize, maxDiff);
  CHECK(median->getMemoryState() == cpu && cost->getMemoryState() == cpu);
  CHECK(dump(prefix + ".speckle.disparity", "speckle.disparity", median->host.get(), median->size()));
  CHECK(dump(prefix + ".speckle.cost", "speckle.cost", cost->host.get(), cost->size()));

  // without a cost map, on the gpu, from the unfiltered map: the same call with cost == nullptr
  disparity->setMemoryState(gpu);
  factory.filterSpeckles(disparity, nullptr, maxSpeckleSize, maxDiff);
  CHECK(disparity->getMemoryState() == gpu);
  disparity->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".speckle.only", "speckle.only", disparity->host.get(), disparity->size()));
  std::printf("ok\n");
  return 0;
}
