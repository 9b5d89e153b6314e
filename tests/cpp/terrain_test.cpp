// tests/cpp/terrain_test.cpp -- the terrain filter through the class API: MeshFactory::terrainSchedule, extractTerrain, the
// footprints closed by DisparityFactory::fillHoles, objectHeights and morphology.
//   terrain_test <w> <h> <height raw float32, w x h> <cell> <max radius> <slope> <initial> <maximum> <out dir>
//     the map starts in host memory and must come back there.  Writes <out dir>level.raw (uint8), bare.raw, terrain.raw and
//     objects.raw (float32); prints "levels <n>", "flagged <n> ground <n> invalid <n>", then "ok".
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

static_assert(sizeof(ssrlcv_terrain_params) == 68, "the parameters are 68 bytes");

template <typename T>
static bool write_raw(const std::string& path, ptr::value<Unity<T>> map) {
  map->setMemoryState(cpu);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  const bool ok = f && std::fwrite(map->host.get(), sizeof(T), map->size(), f) == map->size();
  if (f) std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s <w> <h> <height raw> <cell> <max radius> <slope> <initial> <maximum> <out dir>\n", argv[0]);
    return 2;
  }
  const unsigned int w = (unsigned int)std::atoi(argv[1]), h = (unsigned int)std::atoi(argv[2]);
  const size_t cells = (size_t)w * h;
  ptr::host<float> values((long)cells, true);
  std::FILE* f = std::fopen(argv[3], "rb");
  if (!f || std::fread(values.get(), sizeof(float), cells, f) != cells) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  std::fclose(f);
  const std::string dir = argv[9];
  ptr::value<Unity<float>> height(values, (unsigned long)cells, cpu, true);

  std::vector<uint32_t> radii;
  std::vector<float> thresholds;
  CHECK(MeshFactory::terrainSchedule(std::atof(argv[4]), (unsigned int)std::atoi(argv[5]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]), radii,
                                     thresholds));
  CHECK(radii.size() == thresholds.size() && !radii.empty());
  std::printf("levels %zu\n", radii.size());
  std::vector<uint32_t> many;
  std::vector<float> none;
  CHECK(!MeshFactory::terrainSchedule(1.0, 1000u, 0.3, 0.5, 1.5, many, none));  // 1, 2, .., 512, 1000: eleven levels

  ptr::value<Unity<unsigned char>> level;
  auto bare = MeshFactory::extractTerrain(height, w, h, radii, thresholds, &level);
  CHECK(bare != nullptr && level != nullptr && height->getMemoryState() == cpu);
  CHECK(MeshFactory::extractTerrain(height, w, h, {2u, 2u}, {0.5f, 0.5f}) == nullptr);  // not ascending: refused
  DisparityFactory factory(2u);
  factory.setMapSize(w, h);
  auto terrain = factory.fillHoles(bare, 0xFFu, 0xFFFFFFFFu, 1u, 1u);
  auto objects = MeshFactory::objectHeights(height, terrain, w, h);
  CHECK(terrain != nullptr && objects != nullptr && height->getMemoryState() == cpu);

  // an opening never raises a cell, and the whole-map erosion is one value
  auto opened = MeshFactory::morphology(height, w, h, radii.back(), SSRLCV_MORPH_OPEN);
  auto lowest = MeshFactory::morphology(height, w, h, 0xFFFFFFFFu, SSRLCV_MORPH_ERODE);
  CHECK(opened != nullptr && lowest != nullptr && MeshFactory::morphology(height, w, h, 0u, SSRLCV_MORPH_OPEN) == nullptr);
  opened->setMemoryState(cpu);
  lowest->setMemoryState(cpu);
  for (size_t p = 0; p < cells; ++p) {
    CHECK(!(opened->host.get()[p] > height->host.get()[p]));
    CHECK(std::memcmp(&lowest->host.get()[p], &lowest->host.get()[0], 4) == 0);
  }

  level->setMemoryState(cpu);
  unsigned long flagged = 0, ground = 0, invalid = 0;
  for (size_t p = 0; p < cells; ++p) {
    const unsigned char l = level->host.get()[p];
    if (l == 0) ++ground; else if (l == 255) ++invalid; else ++flagged;
  }
  std::printf("flagged %lu ground %lu invalid %lu\n", flagged, ground, invalid);
  CHECK(write_raw(dir + "level.raw", level) && write_raw(dir + "bare.raw", bare) && write_raw(dir + "terrain.raw", terrain) &&
        write_raw(dir + "objects.raw", objects));
  std::printf("ok\n");
  return 0;
}
