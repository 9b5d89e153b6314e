// tests/cpp/rectify_test.cpp -- rectification through the class API: DisparityFactory::rectify, maskRectified, unrectifyMatches.
//   rectify_test <left raw u8> <right raw u8> <W> <H> <left camera> <right camera> <radius> <dmin> <D> <lr> <subpixel> <step>
//                <out prefix>                                                                       (GPU)
//     the cameras are files of one Image::Camera record (80 bytes) each; pixels start in host memory; writes <prefix>.left and
//     <prefix>.right (the rectified images), <prefix>.disparity (float32 W x H, after the mask), <prefix>.cost (uint32, after
//     the mask) and <prefix>.matches (Match records in source pixels), prints the match count, then "ok".
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
static bool dump(const std::string& path, const T* data, size_t n) {
  std::FILE* o = std::fopen(path.c_str(), "wb");
  if (!o) return false;
  const bool ok = std::fwrite(data, sizeof(T), n, o) == n;
  std::fclose(o);
  return ok;
}

static void slurp(const char* path, void* dst, size_t bytes) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
  const size_t got = std::fread(dst, 1, bytes, f);
  std::fclose(f);
  if (got != bytes) { std::fprintf(stderr, "short read of %s\n", path); std::exit(2); }
}

static ptr::value<Image> load(const char* path, const char* cameraPath, unsigned W, unsigned H, int id) {
  ptr::host<unsigned char> px((long)W * H, true);
  slurp(path, px.get(), (size_t)W * H);
  ptr::value<Unity<unsigned char>> pixels(px, (unsigned long)W * H, cpu, true);
  ptr::value<Image> image(uint2{W, H}, 1u, pixels);
  image->id = id;
  slurp(cameraPath, &image->camera, sizeof(Image::Camera));
  return image;
}

int main(int argc, char** argv) {
  if (argc < 14) {
    std::fprintf(stderr, "usage: %s <left> <right> <W> <H> <left camera> <right camera> <radius> <dmin> <D> <lr> <subpixel> <step> <prefix>\n", argv[0]);
    return 2;
  }
  const unsigned W = (unsigned)std::atoi(argv[3]), H = (unsigned)std::atoi(argv[4]);
  ptr::value<Image> left = load(argv[1], argv[5], W, H, 0), right = load(argv[2], argv[6], W, H, 1);
  DisparityFactory factory((unsigned)std::atoi(argv[7]));
  factory.setDisparityRange(std::atoi(argv[8]), (unsigned)std::atoi(argv[9]));
  factory.setLeftRightTolerance(std::atoi(argv[10]));
  factory.setSubpixel(std::atoi(argv[11]) != 0);
  factory.setStep((unsigned)std::atoi(argv[12]));
  const std::string prefix = argv[13];

  ptr::value<Image> leftR, rightR;
  const Rectification rect = factory.rectify(left, right, leftR, rightR);
  CHECK(left->pixels->getMemoryState() == cpu && right->pixels->getMemoryState() == cpu);  // origin state restored
  CHECK(leftR->pixels->getMemoryState() == gpu && rightR->pixels->getMemoryState() == gpu);
  CHECK(leftR->size.x == W && leftR->size.y == H && leftR->id == 0 && rightR->id == 1 && rect.w == W && rect.h == H);
  ptr::value<Unity<unsigned int>> cost;
  auto disparity = factory.generateDisparities(leftR, rightR, &cost);
  CHECK(leftR->pixels->getMemoryState() == gpu);
  factory.maskRectified(disparity, cost, rect);
  CHECK(disparity->getMemoryState() == gpu && cost->getMemoryState() == gpu);
  auto matches = factory.generateMatches(disparity, left, right);
  factory.unrectifyMatches(matches, rect);
  CHECK(matches->getMemoryState() == gpu);
  leftR->pixels->transferMemoryTo(cpu);
  rightR->pixels->transferMemoryTo(cpu);
  disparity->transferMemoryTo(cpu);
  cost->transferMemoryTo(cpu);
  matches->transferMemoryTo(cpu);
  CHECK(dump(prefix + ".left", leftR->pixels->host.get(), leftR->pixels->size()));
  CHECK(dump(prefix + ".right", rightR->pixels->host.get(), rightR->pixels->size()));
  CHECK(dump(prefix + ".disparity", disparity->host.get(), disparity->size()));
  CHECK(dump(prefix + ".cost", cost->host.get(), cost->size()));
  CHECK(dump(prefix + ".matches", matches->host.get(), matches->size()));
  std::printf("count %lu\n", (unsigned long)matches->size());
  std::printf("ok\n");
  return 0;
}
