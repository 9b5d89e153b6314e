// tests/cpp/objects_test.cpp -- surface objects through the class API: MeshFactory::extractObjects and objectMeasures.
//   objects_test <w> <h> <objects raw float32, w x h> <min height> <max diff | inf> <min cells> <scale> <cell> <out dir>
//     the map starts in host memory and must come back there.  Writes <out dir>ids.raw (uint32), records.raw (104 bytes a record)
//     and measures.raw (152 bytes a record, on the axis-aligned frame of side <cell> at the origin); prints "objects <n>", one
//     line "<number> label <l> cells <c> box <x0> <y0> <x1> <y1> perimeter <p>" an object, then "ok".
#include <cmath>
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

static_assert(sizeof(ssrlcv_object_params) == 16 && sizeof(ssrlcv_object_record) == 104 && sizeof(ssrlcv_object_measures) == 152,
              "the layouts of include/ssrlcv_hip.h");

template <typename T>
static bool write_raw(const std::string& path, const T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  const bool ok = f && std::fwrite(data, sizeof(T), n, f) == n;
  if (f) std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s <w> <h> <objects raw> <min height> <max diff | inf> <min cells> <scale> <cell> <out dir>\n", argv[0]);
    return 2;
  }
  const unsigned int w = (unsigned int)std::atoi(argv[1]), h = (unsigned int)std::atoi(argv[2]);
  const size_t cells = (size_t)w * h;
  ptr::host<float> values((long)cells, true);
  std::FILE* f = std::fopen(argv[3], "rb");
  if (!f || std::fread(values.get(), sizeof(float), cells, f) != cells) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
  std::fclose(f);
  ptr::value<Unity<float>> map(values, (unsigned long)cells, cpu, true);
  ssrlcv_object_params params = {(float)std::atof(argv[4]), std::strcmp(argv[5], "inf") ? (float)std::atof(argv[5]) : INFINITY,
                                 (float)std::atof(argv[7]), (uint32_t)std::atoi(argv[6])};
  const std::string dir = argv[9];
  ssrlcv_dsm_frame frame = {};
  frame.ex[0] = frame.ey[1] = frame.ez[2] = 1.0f;
  frame.cell = (float)std::atof(argv[8]);
  frame.w = w, frame.h = h;

  std::vector<ssrlcv_object_record> records;
  ptr::value<Unity<uint32_t>> ids;
  CHECK(MeshFactory::extractObjects(map, w, h, params, records, &ids));
  CHECK(ids != nullptr && ids->size() == cells && map->getMemoryState() == cpu);
  std::vector<ssrlcv_object_record> again;
  CHECK(MeshFactory::extractObjects(map, w, h, params, again) && again.size() == records.size());  // without ids: the same records
  CHECK(records.empty() || std::memcmp(again.data(), records.data(), records.size() * sizeof(ssrlcv_object_record)) == 0);
  ssrlcv_object_params refused = params;
  refused.scale = 0.0f;
  CHECK(!MeshFactory::extractObjects(map, w, h, refused, again) && again.empty());

  std::printf("objects %zu\n", records.size());
  std::vector<ssrlcv_object_measures> measures(records.size());
  for (size_t k = 0; k < records.size(); ++k) {
    const ssrlcv_object_record& r = records[k];
    std::printf("%zu label %u cells %u box %u %u %u %u perimeter %u\n", k, r.label, r.cells, r.minX, r.minY, r.maxX, r.maxY, r.perimeter);
    CHECK(MeshFactory::objectMeasures(r, frame, params.scale, measures[k]));
    CHECK(measures[k].area == (double)r.cells * ((double)frame.cell * (double)frame.cell));
  }
  ssrlcv_object_measures none;
  CHECK(records.empty() || !MeshFactory::objectMeasures(records[0], frame, 0.0f, none));
  ids->setMemoryState(cpu);
  CHECK(write_raw(dir + "ids.raw", ids->host.get(), cells) && write_raw(dir + "records.raw", records.data(), records.size()) &&
        write_raw(dir + "measures.raw", measures.data(), measures.size()));
  std::printf("ok\n");
  return 0;
}
