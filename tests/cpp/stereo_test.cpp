// tests/cpp/stereo_test.cpp -- dense stereo through the class API: DisparityFactory + PointCloudFactory::stereo_disparity.
//   stereo_test --windows                                                                         (no GPU)
//     prints sizeof and two distProtocol values of every Window_NxN, then "ok"
//   stereo_test <left raw u8> <right raw u8> <W> <H> <radius> <dmin> <D> <lr> <subpixel> <step> <foc> <baseline> <doffset>
//               <cx> <cy> <out prefix>                                                            (GPU)
//     pixels start in host memory; writes <prefix>.disparity (float32 W x H), <prefix>.cost (uint32), <prefix>.matches
//     (Match records) and <prefix>.points (float3), prints the match count, then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <int N>
static void window_line() {
  // a: value = 3 x + y; b: the same with the corners raised by 10, the centre lowered by 7 (bounded below by 0)
  Window_NxN<N> a, b;
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x) a.values[y][x] = b.values[y][x] = (unsigned char)(3 * x + y);
  b.values[0][0] += 10;
  b.values[0][N - 1] += 10;
  b.values[N - 1][0] += 10;
  b.values[N - 1][N - 1] += 10;
  const int c = N / 2;
  const int lowered = b.values[c][c] >= 7 ? 7 : b.values[c][c];
  b.values[c][c] = (unsigned char)(b.values[c][c] - lowered);
  // full distance both ways, the distance of a window to itself, and the early exit (stops after the first row: 20)
  std::printf("window %d size %lu dist %.1f %.1f self %.1f early %.1f\n", N, (unsigned long)sizeof(Window_NxN<N>), a.distProtocol(b),
              b.distProtocol(a), a.distProtocol(a), a.distProtocol(b, 15.0f));
}

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
  if (argc >= 2 && std::string(argv[1]) == "--windows") {
    window_line<3>();
    window_line<9>();
    window_line<15>();
    window_line<25>();
    window_line<31>();
    static_assert(sizeof(Window_3x3) == 9 && sizeof(Window_31x31) == 961, "Window sizes");
    std::printf("ok\n");
    return 0;
  }
  if (argc < 17) { std::fprintf(stderr, "usage: %s --windows | <left> <right> <W> <H> <radius> <dmin> <D> <lr> <subpixel> <step> <foc> <baseline> <doffset> <cx> <cy> <prefix>\n", argv[0]); return 2; }
  const unsigned W = (unsigned)std::atoi(argv[3]), H = (unsigned)std::atoi(argv[4]);
  ptr::value<Image> left = load(argv[1], W, H, 0), right = load(argv[2], W, H, 1);
  DisparityFactory factory((unsigned)std::atoi(argv[5]));
  factory.setDisparityRange(std::atoi(argv[6]), (unsigned)std::atoi(argv[7]));
  factory.setLeftRightTolerance(std::atoi(argv[8]));
  factory.setSubpixel(std::atoi(argv[9]) != 0);
  factory.setStep((unsigned)std::atoi(argv[10]));
  const float foc = (float)std::atof(argv[11]), baseline = (float)std::atof(argv[12]), doffset = (float)std::atof(argv[13]);
  const float2 center{(float)std::atof(argv[14]), (float)std::atof(argv[15])};
  const std::string prefix = argv[16];

  ptr::value<Unity<unsigned int>> cost;
  auto disparity = factory.generateDisparities(left, right, &cost);
  CHECK(left->pixels->getMemoryState() == cpu && right->pixels->getMemoryState() == cpu);  // origin state restored
  CHECK(disparity->getMemoryState() == gpu && disparity->size() == (unsigned long)W * H);
  auto matches = factory.generateMatches(disparity, left, right);
  CHECK(matches->getMemoryState() == gpu);
  auto cloud = PointCloudFactory().stereo_disparity(matches, foc, baseline, doffset, center);
  CHECK(cloud->getMemoryState() == cpu && cloud->size() == matches->size());
  CHECK(matches->getMemoryState() == gpu);
  disparity->transferMemoryTo(cpu);
  cost->transferMemoryTo(cpu);
  matches->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".disparity", disparity->host.get(), disparity->size()));
  CHECK(dump(prefix + ".cost", cost->host.get(), cost->size()));
  CHECK(dump(prefix + ".matches", matches->host.get(), matches->size()));
  CHECK(dump(prefix + ".points", cloud->host.get(), cloud->size()));
  std::printf("count %lu\n", (unsigned long)matches->size());
  std::printf("ok\n");
  return 0;
}
