// ssrlcv_amd/host/MeshFactory.hpp -- ssrlcv::MeshFactory's point-cloud stage (include/MeshFactory.cuh upstream): the
// statistical neighbour-distance filter and oriented normals over the device k-nearest neighbours of csrc/cloud.hip
// (ssrlcv_hip_knn, ssrlcv_hip_neighbor_distance_filter, ssrlcv_hip_point_normals), and savePoints.  PARITY UNPINNED:
// upstream's Octree-based filters have no fixture; the contract in include/ssrlcv_hip.h is the definition.  Surface
// reconstruction and the Octree / Quadtree classes are not mirrored.
//
// Memory state: `points` goes to the gpu for a call and comes back to its origin state; Unitys this class creates
// (filtered points, normals, mean distances) are left in the state the points were in.
#pragma once
#include <cstdio>
#include <string>
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
                  ptr::device<float>* meanDist) {
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
    return c;
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

  MeshFactory() {}
  explicit MeshFactory(ptr::value<Unity<float3>> points) : points(points) {}

  // a new cloud: normals computed for the previous one are dropped
  void setPoints(ptr::value<Unity<float3>> pts) {
    points = pts;
    normals = ptr::value<Unity<float3>>();
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
  // when computed for these points, are kept in step.  Input order is kept.
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
    const uint32_t c = filter(k, sigma, kept, withNormals ? &keptNormals : nullptr, nullptr);
    logger.info.printf("MeshFactory::filterByNeighborDistance: %u of %lu points kept (mu %.6g, std %.6g, threshold %.6g)",
                       c, n, filterStats[0], filterStats[1], filterStats[2]);
    if (c == 0) {
      points = ptr::value<Unity<float3>>();
      normals = ptr::value<Unity<float3>>();
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
};

}  // namespace ssrlcv
