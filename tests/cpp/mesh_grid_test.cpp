// tests/cpp/mesh_grid_test.cpp -- the disparity mesh through the class API: DisparityFactory::generateMesh and MeshFactory's
// setSurface / computeSurfaceNormals / faces / saveMesh, with filterByNeighborDistance carrying the surface along.
//   mesh_grid_test ply <dir>                          (no GPU) writePLY with faces of a fixed three-triangle mesh -> <dir>/fan.ply
//   mesh_grid_test <map raw float32> <W> <H> <step> <maxJump> <foc> <baseline> <doffset> <cx> <cy> <k> <sigma> <out dir/>
//     the map starts in host memory and must come back there.  generateMatches -> stereo_disparity gives the cloud, generateMesh
//     the surface; writes <dir>mesh.ply (points, surface normals, faces), then filterByNeighborDistance(k, sigma) and
//     <dir>filtered.ply.  Prints "vertices <n> faces <t>", "kept <m> faces <t>", then "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(uint3) == 12, "a face is three uint32");

static ptr::value<Image> blank(unsigned W, unsigned H, int id) {
  ptr::value<Unity<unsigned char>> pixels(nullptr, (unsigned long)W * H, cpu);
  ptr::value<Image> image(uint2{W, H}, 1u, pixels);
  image->id = id;
  return image;
}

int main(int argc, char** argv) {
  if (argc >= 3 && std::string(argv[1]) == "ply") {
    ptr::value<Unity<float3>> p(nullptr, 5ul, cpu), n(nullptr, 5ul, cpu);
    ptr::value<Unity<uint3>> f(nullptr, 3ul, cpu);
    const float3 pv[5] = {{6371.00049f, -0.1f, 1e-7f}, {1.0f / 3.0f, 2.5f, -3.25e5f}, {0.0f, -0.0f, 123456.789f}, {1e-40f, 3.4e38f, -1.17549435e-38f},
                          {0.1f, 0.2f, 0.3f}};
    const float3 nv[5] = {{0.0f, 0.0f, -1.0f}, {0.577350269f, -0.577350269f, 0.577350269f}, {0.0f, 0.0f, 0.0f}, {-0.267261242f, 0.534522484f, -0.801783726f},
                          {1.0f, 0.0f, 0.0f}};
    const uint3 fv[3] = {{0u, 2u, 3u}, {0u, 3u, 1u}, {1u, 3u, 4u}};
    for (int i = 0; i < 5; ++i) p->host.get()[i] = pv[i], n->host.get()[i] = nv[i];
    for (int i = 0; i < 3; ++i) f->host.get()[i] = fv[i];
    writePLY("fan", p, n, f, std::string(argv[2]) + "/");
    writePLY("bare", p, ptr::value<Unity<float3>>(), ptr::value<Unity<uint3>>(), std::string(argv[2]) + "/");  // no normals, no face
    CHECK(p->getMemoryState() == cpu && n->getMemoryState() == cpu && f->getMemoryState() == cpu);
    std::printf("ok\n");
    return 0;
  }
  if (argc < 14) {
    std::fprintf(stderr, "usage: %s ply <dir> | <map float32> <W> <H> <step> <maxJump> <foc> <baseline> <doffset> <cx> <cy> <k> <sigma> <dir/>\n", argv[0]);
    return 2;
  }
  const unsigned W = (unsigned)std::atoi(argv[2]), H = (unsigned)std::atoi(argv[3]), step = (unsigned)std::atoi(argv[4]);
  const float maxJump = (float)std::atof(argv[5]);
  const float foc = (float)std::atof(argv[6]), baseline = (float)std::atof(argv[7]), doffset = (float)std::atof(argv[8]);
  const float2 center{(float)std::atof(argv[9]), (float)std::atof(argv[10])};
  const int k = std::atoi(argv[11]);
  const float sigma = (float)std::atof(argv[12]);
  const std::string dir = argv[13];
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
  factory.setStep(step);
  auto matches = factory.generateMatches(disparity, blank(W, H, 0), blank(W, H, 1));
  auto cloud = PointCloudFactory().stereo_disparity(matches, foc, baseline, doffset, center);
  GridMesh surface = factory.generateMesh(disparity, step, maxJump);
  CHECK(disparity->getMemoryState() == cpu);
  CHECK(surface.gw == (W - 1) / step + 1 && surface.gh == (H - 1) / step + 1 && surface.vertexCount == cloud->size());
  CHECK(surface.vertexIndex->getMemoryState() == gpu && surface.cells->getMemoryState() == gpu);

  MeshFactory mesh;
  mesh.setPoints(cloud);
  CHECK(mesh.faces() == nullptr);  // no surface yet
  mesh.setSurface(surface);
  CHECK(mesh.hasSurface);
  mesh.computeSurfaceNormals();
  CHECK(mesh.normals != nullptr && mesh.normals->size() == cloud->size() && mesh.normals->getMemoryState() == cloud->getMemoryState());
  auto faces = mesh.faces();
  CHECK(faces != nullptr && faces->getMemoryState() == gpu);
  std::printf("vertices %lu faces %lu\n", cloud->size(), faces->size());
  mesh.saveMesh("mesh", dir);

  mesh.filterByNeighborDistance(k, sigma);
  CHECK(mesh.points != nullptr && mesh.hasSurface && mesh.surface.vertexCount == mesh.points->size());
  CHECK(surface.vertexCount == cloud->size());  // the caller's mesh is left as it is
  auto kept = mesh.faces();
  std::printf("kept %lu faces %lu\n", mesh.points->size(), kept != nullptr ? kept->size() : 0ul);
  mesh.saveMesh("filtered", dir);
  std::printf("ok\n");
  return 0;
}
