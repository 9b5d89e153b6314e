// tests/cpp/shift_test.cpp -- the shift search through the class API: MeshFactory::searchShift of two height maps of one grid, and,
// with a cloud, registerToReference from the pose it found.
//   shift_test <frame raw (ssrlcv_dsm_frame, 60 bytes)> <moving height raw float32 x w h> <reference height raw> <radius>
//              <strides, e.g. 4,1> <gateFactor, 0 = no gate> <min overlap share> <out prefix> [<cloud raw float32 x 3> <iterations>]
//     the maps start in host memory and must come back there.  Per level prints "level <k> stride <g> center <x> <y> radius <S>
//     centerQ <c> gateQ <g> checksum <FNV-1a 64 of the table's bytes>" and "result <shiftX> <shiftY> <n> <candidates> <the bits of
//     subX subY bias variance second as hex>"; then "shift <x> <y>" (%.17g), and writes <prefix>.pose (the 60 bytes of
//     ssrlcv_register_pose) and <prefix>.table (the last level's table).  With a cloud: registers it from that pose with the same
//     gate, prints "registered <iterations run> converged <0|1>" and writes <prefix>.registered (the pose).  Then "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(ssrlcv_shift_params) == 28 && sizeof(ssrlcv_shift_entry) == 24 && sizeof(ssrlcv_shift_table) == 16 && sizeof(ssrlcv_shift_result) == 64,
              "the records of the shift search");

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

static bool write_bytes(const std::string& path, const void* data, size_t bytes) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  const bool ok = f && std::fwrite(data, 1, bytes, f) == bytes;
  if (f) std::fclose(f);
  return ok;
}

static unsigned long long fnv1a(const std::vector<unsigned char>& bytes) {
  unsigned long long hash = 0xcbf29ce484222325ull;
  for (unsigned char b : bytes) hash = (hash ^ b) * 0x100000001b3ull;
  return hash;
}

static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 9 && argc != 11) {
    std::fprintf(stderr, "usage: %s <frame raw> <moving raw> <reference raw> <radius> <strides> <gateFactor> <min overlap> <out prefix> [<cloud raw> <iterations>]\n",
                 argv[0]);
    return 2;
  }
  ssrlcv_dsm_frame frame;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&frame, sizeof frame, 1, f) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::fclose(f);
  auto moving = load<float>(argv[2]);
  auto reference = load<float>(argv[3]);
  if (moving == nullptr || reference == nullptr) { std::fprintf(stderr, "cannot read the maps\n"); return 2; }
  const uint32_t radius = (uint32_t)std::atoi(argv[4]);
  std::vector<uint32_t> strides;
  for (const char* p = argv[5]; *p;) {
    strides.push_back((uint32_t)std::strtoul(p, const_cast<char**>(&p), 10));
    if (*p == ',') ++p;
  }
  const float gateFactor = (float)std::atof(argv[6]);
  const double minOverlap = std::atof(argv[7]);
  const std::string prefix = argv[8];

  CHECK(!MeshFactory::searchShift(moving, reference, frame, 33u, strides, gateFactor, 0.0f, minOverlap).found);  // a radius above 32 is refused
  const MeshFactory::ShiftSearch found = MeshFactory::searchShift(moving, reference, frame, radius, strides, gateFactor, 0.0f, minOverlap);
  CHECK(found.found && found.levels.size() == strides.size());
  CHECK(moving->getMemoryState() == cpu && reference->getMemoryState() == cpu);
  for (size_t k = 0; k < found.levels.size(); ++k) {
    const MeshFactory::ShiftLevel& level = found.levels[k];
    const ssrlcv_shift_result& r = level.result;
    std::printf("level %zu stride %u center %d %d radius %u centerQ %d gateQ %u checksum %016llx\n", k, level.params.stride, level.params.centerX,
                level.params.centerY, level.params.radius, level.params.centerQ, level.params.gateQ, fnv1a(level.table));
    std::printf("result %lld %lld %u %u %016llx %016llx %016llx %016llx %016llx\n", (long long)r.shiftX, (long long)r.shiftY, r.n, r.candidates, bits(r.subX),
                bits(r.subY), bits(r.bias), bits(r.variance), bits(r.second));
  }
  std::printf("shift %.17g %.17g\n", found.shiftX, found.shiftY);
  CHECK(write_bytes(prefix + ".pose", &found.pose, sizeof found.pose));
  CHECK(write_bytes(prefix + ".table", found.levels.back().table.data(), found.levels.back().table.size()));

  if (argc == 11) {
    auto cloud = load<float3>(argv[9]);
    if (cloud == nullptr) { std::fprintf(stderr, "cannot read the cloud\n"); return 2; }
    MeshFactory factory;
    factory.setReferenceSurface(reference, frame);
    const MeshFactory::Registration reg = factory.registerToReference(cloud, found.pose, 0x3Fu, (unsigned)std::atoi(argv[10]), gateFactor);
    CHECK(cloud->getMemoryState() == cpu && !reg.history.empty());
    std::printf("registered %zu converged %d\n", reg.history.size(), reg.converged ? 1 : 0);
    CHECK(write_bytes(prefix + ".registered", &reg.pose, sizeof reg.pose));
  }
  std::printf("ok\n");
  return 0;
}
