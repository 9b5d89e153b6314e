// ssrlcv_amd/host/MeshFactory.hpp -- ssrlcv::MeshFactory's point-cloud stage (include/MeshFactory.cuh upstream): the
// statistical neighbour-distance filter and oriented normals over the device k-nearest neighbours of csrc/cloud.hip
// (ssrlcv_hip_knn, ssrlcv_hip_neighbor_distance_filter, ssrlcv_hip_point_normals), and savePoints.  PARITY UNPINNED:
// upstream's Octree-based filters have no fixture; the contract in include/ssrlcv_hip.h is the definition.  Surface
// reconstruction from an unorganised cloud and the Octree / Quadtree classes are not mirrored.  The surface of a DENSE STEREO
// cloud is: its disparity map's grid gives the triangles (DisparityFactory::generateMesh, include/ssrlcv_hip.h "disparity
// mesh"); setSurface takes them, computeSurfaceNormals, faces and saveMesh work on them, and filterByNeighborDistance keeps
// them in step with the points it keeps.
//
// Memory state: `points` goes to the gpu for a call and comes back to its origin state; Unitys this class creates
// (filtered points, normals, mean distances) are left in the state the points were in.
#pragma once
#include <cstdio>
#include <string>
#include "GridMesh.hpp"
#include "Unity.hpp"
#include "cuda_vec_types.hpp"
#include "io_util.hpp"

namespace ssrlcv {

class MeshFactory {
 private:
  // the k-NN of `points` (on the gpu) -> neighbour indices, and their d2 when dist2 != nullptr
  void knn(int k, ptr::device<uint32_t>& nbr, ptr::device<float>* dist2) {
    const uint32_t n = (uint32_t)points->size();
    const size_t wsb = ssrlcv_hip_knn_workspace_bytes(n, (uint32_t)k);
    ptr::device<unsigned char> ws(wsb);
    HipSafeCall(ssrlcv_hip_knn((const ssrlcv_float3*)points->device.get(), n, (uint32_t)k, 0.0f, nbr.get(),
                               dist2 ? dist2->get() : nullptr, nullptr, ws.get(), wsb, nullptr));
  }
  // the filter on `points` (on the gpu): kept points, their normals (when `normals` matches), mean distances, count
  uint32_t filter(int k, float sigma, ptr::device<ssrlcv_float3>& kept, ptr::device<float>* keptNormals,
                  ptr::device<float>* meanDist, bool followSurface = false) {
    const uint32_t n = (uint32_t)points->size();
    ptr::device<uint32_t> nbr((size_t)n * k);
    ptr::device<float> d2((size_t)n * k);
    knn(k, nbr, &d2);
    ptr::device<uint32_t> index(n);
    ptr::device<double> stats(3);
    ptr::device<uint32_t> count(1);
    const size_t wsb = ssrlcv_hip_neighbor_filter_workspace_bytes(n, (uint32_t)k);
    ptr::device<unsigned char> ws(wsb);
    HipSafeCall(ssrlcv_hip_neighbor_distance_filter((const ssrlcv_float3*)points->device.get(), n, d2.get(), (uint32_t)k,
                                                    sigma, meanDist ? meanDist->get() : nullptr, stats.get(), kept.get(),
                                                    index.get(), keptNormals ? (const float*)normals->device.get() : nullptr,
                                                    keptNormals ? keptNormals->get() : nullptr, count.get(), ws.get(), wsb,
                                                    nullptr));
    uint32_t c = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&c, count.get(), sizeof c, 1));
    HipSafeCall(ssrlcv_hip_memcpy(filterStats, stats.get(), sizeof filterStats, 1));
    if (followSurface) {  // the kept rows, ascending, are the vertices the surface keeps: kept point j is vertex j
      const size_t sel = ssrlcv_hip_mesh_select_workspace_bytes(surface.vertexCount);
      ptr::device<unsigned char> selWs(sel ? sel : 1);
      HipSafeCall(ssrlcv_hip_mesh_select(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh,
                                         surface.vertexCount, index.get(), c, selWs.get(), sel, nullptr));
      HipSafeCall(ssrlcv_hip_device_synchronize());  // the workspace and the index go out of scope
      surface.vertexCount = c;
    }
    return c;
  }
  template <typename T>
  static ptr::value<Unity<T>> copyToGpu(ptr::value<Unity<T>> from) {
    ptr::value<Unity<T>> to(nullptr, from->size(), gpu);
    const bool onGpu = from->getMemoryState() == gpu || from->getMemoryState() == both;
    HipSafeCall(ssrlcv_hip_memcpy(to->device.get(), onGpu ? (const void*)from->device.get() : (const void*)from->host.get(),
                                  from->size() * sizeof(T), onGpu ? 2 : 0));
    return to;
  }
  bool usable(int k, const char* what) const {
    if (points == nullptr || k < 1 || k > SSRLCV_KNN_MAX_K || points->size() < (unsigned long)k + 1) {
      logger.err.printf("MeshFactory::%s: needs 1 <= k <= %d and more than k points", what, SSRLCV_KNN_MAX_K);
      return false;
    }
    return true;
  }

 public:
  ptr::value<Unity<float3>> points;
  ptr::value<Unity<float3>> normals;  // null until computeNormals; kept row for row with points by the filter
  double filterStats[3] = {0, 0, 0};  // {mu, std, threshold} of the last filterByNeighborDistance
  GridMesh surface;                   // set by setSurface: vertex v is points[v]; its own copy of the maps, in state gpu
  bool hasSurface = false;

  MeshFactory() {}
  explicit MeshFactory(ptr::value<Unity<float3>> points) : points(points) {}

  // a new cloud: normals computed for the previous one are dropped
  void setPoints(ptr::value<Unity<float3>> pts) {
    points = pts;
    normals = ptr::value<Unity<float3>>();
    clearSurface();
  }

  // the triangles of the points' disparity map (DisparityFactory::generateMesh for the map and step the points' records were
  // taken at): vertex v of the mesh is points[v].  The factory works on a copy of the two maps, so `mesh` stays as it is.
  void setSurface(const GridMesh& mesh) {
    if (points == nullptr || mesh.vertexIndex == nullptr || mesh.cells == nullptr || mesh.vertexCount != points->size()) {
      logger.err.printf("MeshFactory::setSurface: the mesh has %u vertices, the cloud %lu points", mesh.vertexCount,
                        points == nullptr ? 0ul : points->size());
      return;
    }
    surface = mesh;
    surface.vertexIndex = copyToGpu(mesh.vertexIndex);
    surface.cells = copyToGpu(mesh.cells);
    hasSurface = true;
  }
  void clearSurface() {
    surface = GridMesh();
    hasSurface = false;
  }

  // unit normals from the surface's triangles, facing the camera of the disparity map; (0, 0, 0) for a vertex without one
  void computeSurfaceNormals() {
    if (!hasSurface || points == nullptr || surface.vertexCount != points->size()) {
      logger.err << "MeshFactory::computeSurfaceNormals: needs a surface of these points (setSurface)";
      return;
    }
    MemoryState origin = points->getMemoryState();
    if (origin == cpu || points->getFore() == cpu) points->transferMemoryTo(gpu);
    const uint32_t n = (uint32_t)points->size();
    normals = ptr::value<Unity<float3>>(ptr::device<float3>(n), (unsigned long)n, gpu);
    HipSafeCall(ssrlcv_hip_memset(normals->device.get(), 0, (size_t)n * sizeof(float3)));
    HipSafeCall(ssrlcv_hip_mesh_normals((const ssrlcv_float3*)points->device.get(), n, surface.vertexIndex->device.get(),
                                        surface.cells->device.get(), surface.gw, surface.gh, (float*)normals->device.get(), nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    if (origin == cpu) {
      points->setMemoryState(cpu);
      normals->setMemoryState(cpu);
    }
  }

  // the surface's triangles as vertex index triples, in state gpu; null without a surface or without a triangle
  ptr::value<Unity<uint3>> faces() {
    if (!hasSurface) return ptr::value<Unity<uint3>>();
    const size_t wsb = ssrlcv_hip_mesh_triangles_workspace_bytes(surface.gw, surface.gh);
    ptr::device<unsigned char> ws(wsb ? wsb : 1);
    ptr::device<uint32_t> count(1);
    HipSafeCall(ssrlcv_hip_mesh_triangles(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh, nullptr,
                                          0, count.get(), ws.get(), wsb, nullptr));
    uint32_t t = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&t, count.get(), sizeof t, 1));
    if (t == 0) return ptr::value<Unity<uint3>>();
    ptr::value<Unity<uint3>> out(nullptr, (unsigned long)t, gpu);
    HipSafeCall(ssrlcv_hip_mesh_triangles(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh,
                                          (uint32_t*)out->device.get(), t, count.get(), ws.get(), wsb, nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());  // the workspace goes out of scope
    return out;
  }

  // m_i: the mean distance of every point to its k nearest neighbours (+inf for non-finite points)
  ptr::value<Unity<float>> calculateAverageDistancesToNeighbors(int k) {
    if (!usable(k, "calculateAverageDistancesToNeighbors")) return ptr::value<Unity<float>>();
    MemoryState origin = points->getMemoryState();
    if (origin == cpu || points->getFore() == cpu) points->transferMemoryTo(gpu);
    const unsigned long n = points->size();
    ptr::device<ssrlcv_float3> kept(n);
    ptr::device<float> mean(n);
    filter(k, 0.0f, kept, nullptr, &mean);
    ptr::value<Unity<float>> out(mean, n, gpu);
    if (origin == cpu) {
      points->setMemoryState(cpu);
      out->setMemoryState(cpu);
    }
    return out;
  }

  // removes the points whose mean neighbour distance exceeds mu + sigma * std (the non-finite ones always); normals,
  // when computed for these points, are kept in step, and so is a surface (ssrlcv_hip_mesh_select: a triangle that loses a
  // corner goes, nothing is re-triangulated).  Input order is kept.
  void filterByNeighborDistance(int k, float sigma) {
    if (!usable(k, "filterByNeighborDistance")) return;
    MemoryState origin = points->getMemoryState();
    if (origin == cpu || points->getFore() == cpu) points->transferMemoryTo(gpu);
    const unsigned long n = points->size();
    const bool withNormals = normals != nullptr && normals->size() == n;
    MemoryState originN = withNormals ? normals->getMemoryState() : null;
    if (withNormals && (originN == cpu || normals->getFore() == cpu)) normals->transferMemoryTo(gpu);
    ptr::device<ssrlcv_float3> kept(n);
    ptr::device<float> keptNormals(withNormals ? 3 * n : 1);
    const uint32_t c = filter(k, sigma, kept, withNormals ? &keptNormals : nullptr, nullptr, hasSurface);
    logger.info.printf("MeshFactory::filterByNeighborDistance: %u of %lu points kept (mu %.6g, std %.6g, threshold %.6g)",
                       c, n, filterStats[0], filterStats[1], filterStats[2]);
    if (c == 0) {
      points = ptr::value<Unity<float3>>();
      normals = ptr::value<Unity<float3>>();
      clearSurface();
      return;
    }
    points = ptr::value<Unity<float3>>(ptr::device<float3>(c), (unsigned long)c, gpu);
    HipSafeCall(ssrlcv_hip_memcpy(points->device.get(), kept.get(), (size_t)c * sizeof(float3), 2));
    if (origin == cpu) points->setMemoryState(cpu);
    if (withNormals) {
      normals = ptr::value<Unity<float3>>(ptr::device<float3>(c), (unsigned long)c, gpu);
      HipSafeCall(ssrlcv_hip_memcpy(normals->device.get(), keptNormals.get(), (size_t)c * sizeof(float3), 2));
      if (originN == cpu) normals->setMemoryState(cpu);
    } else if (normals != nullptr) {
      normals = ptr::value<Unity<float3>>();  // computed for another cloud
    }
  }

  // unit normals from the k nearest neighbours, oriented towards viewpoint (e.g. the mean camera position)
  void computeNormals(int k, float3 viewpoint) {
    if (!usable(k, "computeNormals")) return;
    MemoryState origin = points->getMemoryState();
    if (origin == cpu || points->getFore() == cpu) points->transferMemoryTo(gpu);
    const uint32_t n = (uint32_t)points->size();
    ptr::device<uint32_t> nbr((size_t)n * k);
    knn(k, nbr, nullptr);
    normals = ptr::value<Unity<float3>>(ptr::device<float3>(n), (unsigned long)n, gpu);
    const ssrlcv_float3 vp = {viewpoint.x, viewpoint.y, viewpoint.z};
    HipSafeCall(ssrlcv_hip_point_normals((const ssrlcv_float3*)points->device.get(), n, nbr.get(), (uint32_t)k, vp,
                                         (float*)normals->device.get(), nullptr));
    if (origin == cpu) {
      points->setMemoryState(cpu);
      normals->setMemoryState(cpu);
    }
  }

  // ASCII PLY of the points (and their normals once computed) as <dir><filename>.ply
  void savePoints(std::string filename, std::string dir = "out/") {
    if (points == nullptr) return;
    if (normals != nullptr && normals->size() == points->size()) writePLY(filename, points, normals, dir);
    else writePLY(filename, points, dir);
  }

  // ASCII PLY of the points, their normals once computed, and the surface's triangles as <dir><filename>.ply
  void saveMesh(std::string filename, std::string dir = "out/") {
    if (points == nullptr) return;
    const bool withNormals = normals != nullptr && normals->size() == points->size();
    writePLY(filename, points, withNormals ? normals : ptr::value<Unity<float3>>(), faces(), dir);
  }
};

}  // namespace ssrlcv
