// ssrlcv_amd/host/io_util.hpp -- the one IO routine the stage flow needs: the simple ASCII PLY writer
// (src/io_util.cpp:740-754, called by doTriangulation src/Pipeline.cu:276).  Same header lines, vertex format and
// default float formatting; `dir` defaults to the reference's "out/".  Image decoding, tinyply and CSV writers are out
// of scope.
#pragma once
#include <fstream>
#include <string>
#include "Scoped.hpp"
#include "Unity.hpp"
#include "cuda_vec_types.hpp"

namespace ssrlcv {
inline void writePLY(std::string filename, ptr::value<Unity<float3>> points, std::string dir = "out/") {
  CpuRead<float3> onCpu(points);
  std::ofstream of;
  of.open(dir + filename + ".ply");
  of << "ply\nformat ascii 1.0\n";
  of << "comment author: SSRLCV simple PLY writer (MI355X build)\n";
  of << "element vertex " << points->size() << "\n";
  of << "property float x\nproperty float y\nproperty float z\n";
  of << "end_header\n";
  float3* p = points->host.get();
  for (unsigned long i = 0; i < points->size(); i++) of << p[i].x << " " << p[i].y << " " << p[i].z << "\n";
  of.close();
}

// The same writer with a normal per vertex (property float nx / ny / nz; MeshFactory::savePoints once normals exist).
// Floats are written with 9 significant digits, so that they read back bit for bit.  Both Unitys come back to their
// origin state.
inline void writePLY(std::string filename, ptr::value<Unity<float3>> points, ptr::value<Unity<float3>> normals,
                     std::string dir = "out/") {
  if (normals->size() != points->size()) {
    logger.err.printf("writePLY: %lu normals for %lu points", normals->size(), points->size());
    return;
  }
  CpuRead<float3> onCpu(points), normalsOnCpu(normals);
  std::ofstream of;
  of.open(dir + filename + ".ply");
  of.precision(9);
  of << "ply\nformat ascii 1.0\n";
  of << "comment author: SSRLCV simple PLY writer (MI355X build)\n";
  of << "element vertex " << points->size() << "\n";
  of << "property float x\nproperty float y\nproperty float z\n";
  of << "property float nx\nproperty float ny\nproperty float nz\n";
  of << "end_header\n";
  const float3* p = points->host.get();
  const float3* n = normals->host.get();
  for (unsigned long i = 0; i < points->size(); i++)
    of << p[i].x << " " << p[i].y << " " << p[i].z << " " << n[i].x << " " << n[i].y << " " << n[i].z << "\n";
  of.close();
}

// The same writer with triangles behind the vertices (element face / property list uchar int vertex_indices;
// MeshFactory::saveMesh): `normals` may be null, `faces` may be null for a mesh without a triangle.  Floats with 9 significant
// digits.  Every Unity comes back to its origin state.
inline void writePLY(std::string filename, ptr::value<Unity<float3>> points, ptr::value<Unity<float3>> normals,
                     ptr::value<Unity<uint3>> faces, std::string dir = "out/") {
  const bool withNormals = normals != nullptr;
  if (withNormals && normals->size() != points->size()) {
    logger.err.printf("writePLY: %lu normals for %lu points", normals->size(), points->size());
    return;
  }
  const unsigned long numFaces = faces != nullptr ? faces->size() : 0ul;
  CpuRead<float3> onCpu(points), normalsOnCpu(normals);
  CpuRead<uint3> facesOnCpu(numFaces ? faces : ptr::value<Unity<uint3>>());
  std::ofstream of;
  of.open(dir + filename + ".ply");
  of.precision(9);
  of << "ply\nformat ascii 1.0\n";
  of << "comment author: SSRLCV simple PLY writer (MI355X build)\n";
  of << "element vertex " << points->size() << "\n";
  of << "property float x\nproperty float y\nproperty float z\n";
  if (withNormals) of << "property float nx\nproperty float ny\nproperty float nz\n";
  of << "element face " << numFaces << "\n";
  of << "property list uchar int vertex_indices\n";
  of << "end_header\n";
  const float3* p = points->host.get();
  const float3* n = withNormals ? normals->host.get() : nullptr;
  for (unsigned long i = 0; i < points->size(); i++) {
    of << p[i].x << " " << p[i].y << " " << p[i].z;
    if (n) of << " " << n[i].x << " " << n[i].y << " " << n[i].z;
    of << "\n";
  }
  const uint3* f = numFaces ? faces->host.get() : nullptr;
  for (unsigned long i = 0; i < numFaces; i++) of << "3 " << f[i].x << " " << f[i].y << " " << f[i].z << "\n";
  of.close();
}

// The same writer with a grey per vertex behind the normals (property uchar red / green / blue, the grey three times;
// MeshFactory::saveMesh once setVertexColors has run).  `colors` is read in host memory.
inline void writePLY(std::string filename, ptr::value<Unity<float3>> points, ptr::value<Unity<float3>> normals,
                     ptr::value<Unity<unsigned char>> colors, ptr::value<Unity<uint3>> faces, std::string dir = "out/") {
  const bool withNormals = normals != nullptr;
  if ((withNormals && normals->size() != points->size()) || colors == nullptr || colors->size() != points->size()) {
    logger.err.printf("writePLY: %lu normals and %lu colours for %lu points", withNormals ? normals->size() : 0ul,
                      colors == nullptr ? 0ul : colors->size(), points->size());
    return;
  }
  const unsigned long numFaces = faces != nullptr ? faces->size() : 0ul;
  CpuRead<float3> onCpu(points), normalsOnCpu(normals);
  CpuRead<uint3> facesOnCpu(numFaces ? faces : ptr::value<Unity<uint3>>());
  CpuRead<unsigned char> colorsOnCpu(colors);
  std::ofstream of;
  of.open(dir + filename + ".ply");
  of.precision(9);
  of << "ply\nformat ascii 1.0\n";
  of << "comment author: SSRLCV simple PLY writer (MI355X build)\n";
  of << "element vertex " << points->size() << "\n";
  of << "property float x\nproperty float y\nproperty float z\n";
  if (withNormals) of << "property float nx\nproperty float ny\nproperty float nz\n";
  of << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
  of << "element face " << numFaces << "\n";
  of << "property list uchar int vertex_indices\n";
  of << "end_header\n";
  const float3* p = points->host.get();
  const float3* n = withNormals ? normals->host.get() : nullptr;
  const unsigned char* g = colors->host.get();
  for (unsigned long i = 0; i < points->size(); i++) {
    of << p[i].x << " " << p[i].y << " " << p[i].z;
    if (n) of << " " << n[i].x << " " << n[i].y << " " << n[i].z;
    of << " " << (unsigned)g[i] << " " << (unsigned)g[i] << " " << (unsigned)g[i] << "\n";
  }
  const uint3* f = numFaces ? faces->host.get() : nullptr;
  for (unsigned long i = 0; i < numFaces; i++) of << "3 " << f[i].x << " " << f[i].y << " " << f[i].z << "\n";
  of.close();
}
}  // namespace ssrlcv
