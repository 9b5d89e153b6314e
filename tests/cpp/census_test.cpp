// tests/cpp/census_test.cpp -- the census cost through the class API: DisparityFactory::setCensus + generateDisparities.
//   census_test <left raw u8> <right raw u8> <W> <H> <census> <radius> <dmin> <D> <costClamp> <P1> <P2> <paths> <lr> <subpixel> <out prefix>
//     pixels start in host memory; writes <prefix>.disparity (float32 W x H) and <prefix>.cost (uint32) of census block
//     matching, <prefix>.sgm.disparity and <prefix>.sgm.cost of semi-global matching over the same costs; then clears the
//     census and the semi-global mode and writes the SAD maps of the same factory at the footprint radius as
//     <prefix>.sad.disparity; prints "ok".
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
static bool dump(const std::string& path, const T* data, size_t n) {
  std::FILE* o = std::fopen(path.c_str(), "wb");
  if (!o) return false;
  const bool ok = std::fwrite(data, sizeof(T), n, o) == n;
  std::fclose(o);
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
  static_assert(sizeof(ssrlcv_stereo_params) == 24 && sizeof(ssrlcv_sgm_params) == 36, "the census calls add no struct and no field");
  if (argc < 16) {
    std::fprintf(stderr, "usage: %s <left> <right> <W> <H> <census> <radius> <dmin> <D> <costClamp> <P1> <P2> <paths> <lr> <subpixel> <prefix>\n",
                 argv[0]);
    return 2;
  }
  const unsigned W = (unsigned)std::atoi(argv[3]), H = (unsigned)std::atoi(argv[4]);
  const unsigned census = (unsigned)std::atoi(argv[5]), radius = (unsigned)std::atoi(argv[6]);
  ptr::value<Image> left = load(argv[1], W, H, 0), right = load(argv[2], W, H, 1);
  DisparityFactory factory(radius);
  factory.setCensus(census);
  CHECK(factory.footprintRadius() == radius + census);
  factory.setDisparityRange(std::atoi(argv[7]), (unsigned)std::atoi(argv[8]));
  factory.setLeftRightTolerance(std::atoi(argv[13]));
  factory.setSubpixel(std::atoi(argv[14]) != 0);
  const std::string prefix = argv[15];

  ptr::value<Unity<unsigned int>> cost;
  auto disparity = factory.generateDisparities(left, right, &cost);
  CHECK(left->pixels->getMemoryState() == cpu && right->pixels->getMemoryState() == cpu);  // origin state restored
  CHECK(disparity->getMemoryState() == gpu && disparity->size() == (unsigned long)W * H);
  disparity->transferMemoryTo(cpu);
  cost->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".disparity", disparity->host.get(), disparity->size()));
  CHECK(dump(prefix + ".cost", cost->host.get(), cost->size()));

  factory.setSemiGlobal((unsigned)std::atoi(argv[9]), (unsigned)std::atoi(argv[10]), (unsigned)std::atoi(argv[11]),
                        (unsigned)std::strtoul(argv[12], nullptr, 0));
  ptr::value<Unity<unsigned int>> sgmCost;
  auto sgm = factory.generateDisparities(left, right, &sgmCost);
  sgm->transferMemoryTo(cpu);
  sgmCost->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".sgm.disparity", sgm->host.get(), sgm->size()));
  CHECK(dump(prefix + ".sgm.cost", sgmCost->host.get(), sgmCost->size()));

  factory.clearSemiGlobal();
  factory.clearCensus();  // the same factory gives SAD's winners again
  factory.setRadius(radius + census);
  CHECK(factory.footprintRadius() == radius + census);
  auto sad = factory.generateDisparities(left, right);
  sad->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".sad.disparity", sad->host.get(), sad->size()));
  std::printf("ok\n");
  return 0;
}
