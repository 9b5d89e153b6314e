// ssrlcv_amd/host/MeshFactory.hpp -- ssrlcv::MeshFactory's point-cloud stage (include/MeshFactory.cuh upstream): the
// statistical neighbour-distance filter and oriented normals over the device k-nearest neighbours of csrc/cloud.hip
// (ssrlcv_hip_knn, ssrlcv_hip_neighbor_distance_filter, ssrlcv_hip_point_normals), and savePoints.  PARITY UNPINNED:
// upstream's Octree-based filters have no fixture; the contract in include/ssrlcv_hip.h is the definition.  Surface
// reconstruction from an unorganised cloud and the Octree / Quadtree classes are not mirrored.  The surface of a DENSE STEREO
// cloud is: its disparity map's grid gives the triangles (DisparityFactory::generateMesh, include/ssrlcv_hip.h "disparity
// mesh"); setSurface takes them, computeSurfaceNormals, faces and saveMesh work on them, and filterByNeighborDistance keeps
// them in step with the points it keeps.  How far a cloud lies from a reference surface -- upstream's
// calculatePerPointDifference / calculateAverageDifference -- is measured against a height map (setReferenceSurface).
// The surface of a height map is thinned to an error-bounded right-triangle mesh by simplifySurface (include/ssrlcv_hip.h
// "surface simplification"); it is then a triangle list and no grid mesh.
//
// Memory state: `points` goes to the gpu for a call and comes back to its origin state; Unitys this class creates
// (filtered points, normals, mean distances) are left in the state the points were in.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <limits>
#include <string>
#include <vector>
#include "GridMesh.hpp"
#include "Image.hpp"
#include "Scoped.hpp"
#include "Unity.hpp"
#include "cuda_vec_types.hpp"
#include "io_util.hpp"

namespace ssrlcv {

class MeshFactory {
 private:
  // the k-NN of `points` (on the gpu) -> neighbour indices, and their d2 when dist2 != nullptr
  void knn(int k, ptr::device<uint32_t>& nbr, ptr::device<float>* dist2) {
    const uint32_t n = (uint32_t)points->size();
    DeviceScratch ws(ssrlcv_hip_knn_workspace_bytes(n, (uint32_t)k));
    HipSafeCall(ssrlcv_hip_knn((const ssrlcv_float3*)points->device.get(), n, (uint32_t)k, 0.0f, nbr.get(),
                               dist2 ? dist2->get() : nullptr, nullptr, ws.get(), ws.bytes(), nullptr));
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
    DeviceScratch ws(ssrlcv_hip_neighbor_filter_workspace_bytes(n, (uint32_t)k));
    HipSafeCall(ssrlcv_hip_neighbor_distance_filter((const ssrlcv_float3*)points->device.get(), n, d2.get(), (uint32_t)k,
                                                    sigma, meanDist ? meanDist->get() : nullptr, stats.get(), kept.get(),
                                                    index.get(), keptNormals ? (const float*)normals->device.get() : nullptr,
                                                    keptNormals ? keptNormals->get() : nullptr, count.get(), ws.get(),
                                                    ws.bytes(), nullptr));
    uint32_t c = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&c, count.get(), sizeof c, 1));
    HipSafeCall(ssrlcv_hip_memcpy(filterStats, stats.get(), sizeof filterStats, 1));
    if (followSurface) {  // the kept rows, ascending, are the vertices the surface keeps: kept point j is vertex j
      DeviceScratch selWs(ssrlcv_hip_mesh_select_workspace_bytes(surface.vertexCount));
      HipSafeCall(ssrlcv_hip_mesh_select(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh,
                                         surface.vertexCount, index.get(), c, selWs.get(), selWs.bytes(), nullptr));
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
  // rows `rows` (ascending) of `from`, in the state `from` is in
  template <typename T>
  static ptr::value<Unity<T>> gathered(ptr::value<Unity<T>> from, const std::vector<uint32_t>& rows) {
    CpuRead<T> onCpu(from);
    ptr::host<T> values((long)rows.size(), true);
    for (size_t k = 0; k < rows.size(); ++k) values.get()[k] = from->host.get()[rows[k]];
    ptr::value<Unity<T>> out(values, (unsigned long)rows.size(), cpu, true);
    if (onCpu.entry() == gpu) out->setMemoryState(gpu);
    return out;
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
  ptr::value<Unity<unsigned char>> colors;  // null until setVertexColors: one grey a point; dropped by setPoints and by the filter
  double filterStats[3] = {0, 0, 0};  // {mu, std, threshold} of the last filterByNeighborDistance
  GridMesh surface;                   // set by setSurface: vertex v is points[v]; its own copy of the maps, in state gpu
  bool hasSurface = false;
  ptr::value<Unity<float>> surfaceHeight;  // set by setPointsFromHeightMap: its own copy of the map the points came from, in state gpu
  ssrlcv_dsm_frame surfaceFrame = {};
  ptr::value<Unity<uint3>> simplifiedFaces;  // set by simplifySurface: the surface is then this triangle list, no GridMesh
  bool hasSimplified = false;

  MeshFactory() {}
  explicit MeshFactory(ptr::value<Unity<float3>> points) : points(points) {}

  // a new cloud: normals computed for the previous one are dropped
  void setPoints(ptr::value<Unity<float3>> pts) {
    points = pts;
    normals = ptr::value<Unity<float3>>();
    colors = ptr::value<Unity<unsigned char>>();
    clearSurface();
    surfaceHeight = ptr::value<Unity<float>>();
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
    simplifiedFaces = ptr::value<Unity<uint3>>();
    hasSimplified = false;
  }
  // a simplified surface is a triangle list: the calls that read a GridMesh say so and leave it alone
  bool refusesSimplified(const char* what) const {
    if (!hasSimplified) return false;
    logger.err.printf("MeshFactory::%s: the surface was simplified (simplifySurface) and is a triangle list, not a grid mesh", what);
    return true;
  }

  // unit normals from the surface's triangles, facing the camera of the disparity map; (0, 0, 0) for a vertex without one
  void computeSurfaceNormals() {
    if (refusesSimplified("computeSurfaceNormals")) return;
    if (!hasSurface || points == nullptr || surface.vertexCount != points->size()) {
      logger.err << "MeshFactory::computeSurfaceNormals: needs a surface of these points (setSurface)";
      return;
    }
    GpuRead<float3> onGpu(points);
    const uint32_t n = (uint32_t)points->size();
    normals = ptr::value<Unity<float3>>(ptr::device<float3>(n), (unsigned long)n, gpu);
    HipSafeCall(ssrlcv_hip_memset(normals->device.get(), 0, (size_t)n * sizeof(float3)));
    HipSafeCall(ssrlcv_hip_mesh_normals((const ssrlcv_float3*)points->device.get(), n, surface.vertexIndex->device.get(),
                                        surface.cells->device.get(), surface.gw, surface.gh, (float*)normals->device.get(), nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    if (onGpu.entry() == cpu) normals->setMemoryState(cpu);
  }

  // the surface's triangles as vertex index triples, in state gpu; null without a surface or without a triangle
  ptr::value<Unity<uint3>> faces() {
    if (hasSimplified) return simplifiedFaces;
    if (!hasSurface) return ptr::value<Unity<uint3>>();
    DeviceScratch ws(ssrlcv_hip_mesh_triangles_workspace_bytes(surface.gw, surface.gh));
    ptr::device<uint32_t> count(1);
    HipSafeCall(ssrlcv_hip_mesh_triangles(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh, nullptr,
                                          0, count.get(), ws.get(), ws.bytes(), nullptr));
    uint32_t t = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&t, count.get(), sizeof t, 1));
    if (t == 0) return ptr::value<Unity<uint3>>();
    ptr::value<Unity<uint3>> out(nullptr, (unsigned long)t, gpu);
    HipSafeCall(ssrlcv_hip_mesh_triangles(surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh,
                                          (uint32_t*)out->device.get(), t, count.get(), ws.get(), ws.bytes(), nullptr));
    return out;
  }

  // m_i: the mean distance of every point to its k nearest neighbours (+inf for non-finite points)
  ptr::value<Unity<float>> calculateAverageDistancesToNeighbors(int k) {
    if (!usable(k, "calculateAverageDistancesToNeighbors")) return ptr::value<Unity<float>>();
    GpuRead<float3> onGpu(points);
    const unsigned long n = points->size();
    ptr::device<ssrlcv_float3> kept(n);
    ptr::device<float> mean(n);
    filter(k, 0.0f, kept, nullptr, &mean);
    ptr::value<Unity<float>> out(mean, n, gpu);
    if (onGpu.entry() == cpu) out->setMemoryState(cpu);
    return out;
  }

  // removes the points whose mean neighbour distance exceeds mu + sigma * std (the non-finite ones always); normals,
  // when computed for these points, are kept in step, and so is a surface (ssrlcv_hip_mesh_select: a triangle that loses a
  // corner goes, nothing is re-triangulated).  Input order is kept.
  void filterByNeighborDistance(int k, float sigma) {
    if (!usable(k, "filterByNeighborDistance")) return;
    if (hasSimplified) {  // the triangle list indexes the points as they are: it does not follow a filter
      logger.err << "MeshFactory::filterByNeighborDistance: drops the simplified surface (filter before simplifySurface)";
      clearSurface();
    }
    const unsigned long n = points->size();
    const bool withNormals = normals != nullptr && normals->size() == n;
    // the guards hold the Unitys that came in: `points` and `normals` are replaced below
    GpuRead<float3> onGpu(points), normalsOnGpu(withNormals ? normals : ptr::value<Unity<float3>>());
    ptr::device<ssrlcv_float3> kept(n);
    ptr::device<float> keptNormals(withNormals ? 3 * n : 1);
    const uint32_t c = filter(k, sigma, kept, withNormals ? &keptNormals : nullptr, nullptr, hasSurface);
    colors = ptr::value<Unity<unsigned char>>();  // set for the points as they were
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
    if (onGpu.entry() == cpu) points->setMemoryState(cpu);
    if (withNormals) {
      normals = ptr::value<Unity<float3>>(ptr::device<float3>(c), (unsigned long)c, gpu);
      HipSafeCall(ssrlcv_hip_memcpy(normals->device.get(), keptNormals.get(), (size_t)c * sizeof(float3), 2));
      if (normalsOnGpu.entry() == cpu) normals->setMemoryState(cpu);
    } else if (normals != nullptr) {
      normals = ptr::value<Unity<float3>>();  // computed for another cloud
    }
  }

  // unit normals from the k nearest neighbours, oriented towards viewpoint (e.g. the mean camera position)
  void computeNormals(int k, float3 viewpoint) {
    if (!usable(k, "computeNormals")) return;
    GpuRead<float3> onGpu(points);
    const uint32_t n = (uint32_t)points->size();
    ptr::device<uint32_t> nbr((size_t)n * k);
    knn(k, nbr, nullptr);
    normals = ptr::value<Unity<float3>>(ptr::device<float3>(n), (unsigned long)n, gpu);
    const ssrlcv_float3 vp = {viewpoint.x, viewpoint.y, viewpoint.z};
    HipSafeCall(ssrlcv_hip_point_normals((const ssrlcv_float3*)points->device.get(), n, nbr.get(), (uint32_t)k, vp,
                                         (float*)normals->device.get(), nullptr));
    if (onGpu.entry() == cpu) normals->setMemoryState(cpu);
  }

  // ---- the surface model (include/ssrlcv_hip.h "surface model"): the clouds of several pairs become one surface through a
  // height map on a ground grid.  generateHeightMap per cloud, fuseHeightMaps over them (DisparityFactory's medianFilter,
  // filterSpeckles and fillHoles take the result as it is: a height map has a disparity map's form), then
  // setPointsFromHeightMap(height, frame) and setSurface(DisparityFactory::generateMesh(height, 1, maxJump)) with the factory's
  // map size set to the grid; saveMesh then writes the fused surface.

  // the height map of the points this factory holds: per cell of `frame` the greatest (rule 0) or least (rule 1) height; in
  // state gpu, frame.w x frame.h, 0x7FC00000 in an empty cell; null for an empty grid or a refused frame
  ptr::value<Unity<float>> generateHeightMap(const ssrlcv_dsm_frame& frame, unsigned int rule) {
    const unsigned long cells = (unsigned long)frame.w * frame.h;
    if (points == nullptr || cells == 0) {
      logger.err << "MeshFactory::generateHeightMap: needs points and a grid with a cell";
      return ptr::value<Unity<float>>();
    }
    GpuRead<float3> onGpu(points);
    DeviceScratch ws(ssrlcv_hip_dsm_rasterize_workspace_bytes(frame.w, frame.h));
    ptr::value<Unity<float>> height(nullptr, cells, gpu);
    HipSafeCall(ssrlcv_hip_dsm_rasterize((const ssrlcv_float3*)points->device.get(), (uint32_t)points->size(), &frame, rule, height->device.get(),
                                         nullptr, nullptr, ws.get(), ws.bytes(), nullptr));
    return height;
  }

  // 1 to 8 height maps of one w x h grid fused per cell: at least minViews valid entries whose largest and smallest differ by
  // at most maxSpread give their smallest (rule 0), lower median (1) or largest (2); in state gpu.  *views, when asked for,
  // holds the number of valid entries of every cell.  The maps are left in the state they came in.
  static ptr::value<Unity<float>> fuseHeightMaps(const std::vector<ptr::value<Unity<float>>>& maps, unsigned int w, unsigned int h,
                                                 unsigned int minViews, float maxSpread, unsigned int rule,
                                                 ptr::value<Unity<unsigned char>>* views = nullptr) {
    const unsigned long cells = (unsigned long)w * h;
    if (maps.empty() || maps.size() > 8 || cells == 0) {
      logger.err << "MeshFactory::fuseHeightMaps: needs 1 to 8 maps of a grid with a cell";
      return ptr::value<Unity<float>>();
    }
    std::deque<GpuRead<float>> onGpu;  // a deque constructs its guards in place
    std::vector<const float*> dev;
    for (auto& m : maps) {
      if (m == nullptr || m->size() != cells) {
        logger.err << "MeshFactory::fuseHeightMaps: every map has w h entries";
        return ptr::value<Unity<float>>();
      }
      onGpu.emplace_back(m);
      dev.push_back(m->device.get());
    }
    ptr::value<Unity<float>> out(nullptr, cells, gpu);
    if (views) *views = ptr::value<Unity<unsigned char>>(nullptr, cells, gpu);
    HipSafeCall(ssrlcv_hip_dsm_fuse(dev.data(), (uint32_t)maps.size(), w, h, minViews, maxSpread, rule, out->device.get(),
                                    views ? (*views)->device.get() : nullptr, nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    return out;
  }

  // ---- the terrain filter (include/ssrlcv_hip.h "terrain filter"): the ground under a surface model and the heights of what
  // stands on it.  extractTerrain(height, w, h, radii, thresholds) gives the bare earth with the objects' footprints cut out;
  // DisparityFactory::fillHoles closes them (a height map has a disparity map's form); objectHeights(height, terrain, w, h) is
  // the normalised surface.  The maps are left in the state they came in; the results are in state gpu.

  // the windows and thresholds of the progressive morphological filter (Zhang et al. 2003): radii 1, 2, 4, ... with maxRadius as
  // the last entry if it is not one of them, unless `radii` comes filled; t_1 = initial, t_k = min(initial + slope cell 2 (r_k -
  // r_{k-1}), maximum), computed in double and rounded to float once.  false if that takes more than 8 levels or the radii
  // are not ascending from 1
  static bool terrainSchedule(double cell, unsigned int maxRadius, double slope, double initial, double maximum, std::vector<uint32_t>& radii,
                              std::vector<float>& thresholds) {
    if (radii.empty()) {
      for (uint64_t r = 1; r < maxRadius; r *= 2) radii.push_back((uint32_t)r);
      radii.push_back(maxRadius);
    }
    thresholds.clear();
    if (radii.size() > 8 || radii[0] < 1) return false;
    thresholds.push_back((float)initial);
    for (size_t k = 1; k < radii.size(); ++k) {
      if (radii[k] <= radii[k - 1]) return false;
      thresholds.push_back((float)std::min(initial + slope * cell * 2.0 * (double)(radii[k] - radii[k - 1]), maximum));
    }
    return true;
  }

  // ERODE (op 0), DILATE (1), OPEN (2) or CLOSE (3) of a w x h map with the clipped square window of `radius` cells; null for
  // an empty grid or a refused call
  static ptr::value<Unity<float>> morphology(ptr::value<Unity<float>> height, unsigned int w, unsigned int h, unsigned int radius, unsigned int op) {
    const unsigned long cells = (unsigned long)w * h;
    if (height == nullptr || cells == 0 || height->size() != cells) {
      logger.err << "MeshFactory::morphology: the map has w h entries";
      return ptr::value<Unity<float>>();
    }
    GpuRead<float> onGpu(height);
    DeviceScratch ws(ssrlcv_hip_dsm_morphology_workspace_bytes(w, h));
    ptr::value<Unity<float>> out(nullptr, cells, gpu);
    const int status = ssrlcv_hip_dsm_morphology(height->device.get(), out->device.get(), w, h, radius, op, ws.get(), ws.bytes(), nullptr);
    if (status != SSRLCV_OK) {
      logger.err.printf("MeshFactory::morphology: refused (%s)", ssrlcv_hip_status_string(status));
      return ptr::value<Unity<float>>();
    }
    return out;
  }

  // the bare earth of a w x h height map: the height at the cells no level of the filter flagged, 0x7FC00000 elsewhere.
  // *level, when asked for: 0 ground, k the first level that flagged the cell, 255 an invalid cell.  Null for a refused call
  static ptr::value<Unity<float>> extractTerrain(ptr::value<Unity<float>> height, unsigned int w, unsigned int h, const std::vector<uint32_t>& radii,
                                                 const std::vector<float>& thresholds, ptr::value<Unity<unsigned char>>* level = nullptr) {
    const unsigned long cells = (unsigned long)w * h;
    if (height == nullptr || cells == 0 || height->size() != cells || radii.empty() || radii.size() > 8 || radii.size() != thresholds.size()) {
      logger.err << "MeshFactory::extractTerrain: the map has w h entries, and 1 to 8 radii a threshold each";
      return ptr::value<Unity<float>>();
    }
    ssrlcv_terrain_params params = {};
    params.levels = (uint32_t)radii.size();
    for (size_t k = 0; k < radii.size(); ++k) {
      params.radius[k] = radii[k];
      params.threshold[k] = thresholds[k];
    }
    GpuRead<float> onGpu(height);
    DeviceScratch ws(ssrlcv_hip_dsm_terrain_workspace_bytes(w, h));
    ptr::value<Unity<float>> terrain(nullptr, cells, gpu);
    if (level) *level = ptr::value<Unity<unsigned char>>(nullptr, cells, gpu);
    const int status = ssrlcv_hip_dsm_terrain(height->device.get(), w, h, &params, terrain->device.get(), level ? (*level)->device.get() : nullptr, nullptr,
                                              ws.get(), ws.bytes(), nullptr);
    if (status != SSRLCV_OK) {
      logger.err.printf("MeshFactory::extractTerrain: refused (%s)", ssrlcv_hip_status_string(status));
      if (level) *level = ptr::value<Unity<unsigned char>>();
      return ptr::value<Unity<float>>();
    }
    return terrain;
  }

  // height - terrain where both are valid and the difference is a number, 0x7FC00000 elsewhere: the form differenceStats takes
  static ptr::value<Unity<float>> objectHeights(ptr::value<Unity<float>> height, ptr::value<Unity<float>> terrain, unsigned int w, unsigned int h) {
    const unsigned long cells = (unsigned long)w * h;
    if (height == nullptr || terrain == nullptr || cells == 0 || height->size() != cells || terrain->size() != cells) {
      logger.err << "MeshFactory::objectHeights: both maps have w h entries";
      return ptr::value<Unity<float>>();
    }
    GpuRead<float> heightOnGpu(height), terrainOnGpu(terrain);
    ptr::value<Unity<float>> out(nullptr, cells, gpu);
    HipSafeCall(ssrlcv_hip_dsm_subtract(height->device.get(), terrain->device.get(), w, h, out->device.get(), nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    return out;
  }

  // ---- surface objects (include/ssrlcv_hip.h "surface objects"): what stands on the terrain, one record an object.
  // extractObjects(objects, w, h, params) takes objectHeights' map: the 4-connected footprints of the cells at least
  // params.minHeight high, those of params.minCells cells and more numbered in raster order of their first cells.  A first call
  // counts them, a second one writes every record (host memory, in that order).  *ids, when asked for (state gpu): the number of
  // a cell's object, UINT32_MAX for a cell of none.  false for an empty grid or a refused call; the map is left in the state it
  // came in.
  static bool extractObjects(ptr::value<Unity<float>> objects, unsigned int w, unsigned int h, const ssrlcv_object_params& params,
                             std::vector<ssrlcv_object_record>& records, ptr::value<Unity<uint32_t>>* ids = nullptr) {
    const unsigned long cells = (unsigned long)w * h;
    records.clear();
    if (ids) *ids = ptr::value<Unity<uint32_t>>();
    if (objects == nullptr || cells == 0 || objects->size() != cells) {
      logger.err << "MeshFactory::extractObjects: the map has w h entries";
      return false;
    }
    GpuRead<float> onGpu(objects);
    ptr::device<uint32_t> count(1);
    DeviceScratch ws(ssrlcv_hip_dsm_objects_workspace_bytes(w, h));
    int status = ssrlcv_hip_dsm_objects(objects->device.get(), w, h, &params, nullptr, nullptr, 0, count.get(), ws.get(), ws.bytes(), nullptr);
    if (status != SSRLCV_OK) {
      logger.err.printf("MeshFactory::extractObjects: refused (%s)", ssrlcv_hip_status_string(status));
      return false;
    }
    uint32_t n = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&n, count.get(), sizeof n, 1));
    if (ids) *ids = ptr::value<Unity<uint32_t>>(nullptr, cells, gpu);
    ptr::device<uint64_t> device((unsigned long)(n ? n : 1) * (sizeof(ssrlcv_object_record) / 8));  // 8-byte aligned: the sums are added in place
    HipSafeCall(ssrlcv_hip_dsm_objects(objects->device.get(), w, h, &params, ids ? (*ids)->device.get() : nullptr, (ssrlcv_object_record*)device.get(), n,
                                       count.get(), ws.get(), ws.bytes(), nullptr));
    records.resize(n);
    if (n) HipSafeCall(ssrlcv_hip_memcpy(records.data(), device.get(), (size_t)n * sizeof(ssrlcv_object_record), 1));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    return true;
  }

  // area, outline length, compactness, centroid (cells, and on the frame's plane in the world), mean height, volume, RMS height,
  // second moments, major axis and elongation of one record; host arithmetic, no device.  `scale` is the params' scale
  static bool objectMeasures(const ssrlcv_object_record& record, const ssrlcv_dsm_frame& frame, float scale, ssrlcv_object_measures& out) {
    return ssrlcv_object_measures_host(&record, &frame, scale, &out) == SSRLCV_OK;
  }

  // the valid cells of a height map become this factory's points, in raster order: the vertex numbering of
  // DisparityFactory::generateMesh(height, 1, maxJump), so that mesh is the surface of these points
  void setPointsFromHeightMap(ptr::value<Unity<float>> height, const ssrlcv_dsm_frame& frame) {
    const unsigned long cells = (unsigned long)frame.w * frame.h;
    if (height == nullptr || cells == 0 || height->size() != cells) {
      logger.err << "MeshFactory::setPointsFromHeightMap: the map has frame.w frame.h entries";
      return;
    }
    GpuRead<float> onGpu(height);
    ptr::device<uint32_t> count(1);
    DeviceScratch ws(ssrlcv_hip_dsm_points_workspace_bytes(frame.w, frame.h));
    HipSafeCall(ssrlcv_hip_dsm_points(height->device.get(), &frame, nullptr, 0, count.get(), ws.get(), ws.bytes(), nullptr));
    uint32_t n = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&n, count.get(), sizeof n, 1));
    if (n == 0) {
      setPoints(ptr::value<Unity<float3>>());
      return;
    }
    ptr::value<Unity<float3>> pts(nullptr, (unsigned long)n, gpu);
    HipSafeCall(ssrlcv_hip_dsm_points(height->device.get(), &frame, (ssrlcv_float3*)pts->device.get(), n, count.get(), ws.get(), ws.bytes(), nullptr));
    setPoints(pts);
    surfaceHeight = copyToGpu(height);  // simplifySurface works on the map the points came from
    surfaceFrame = frame;
  }

  // ---- surface simplification (include/ssrlcv_hip.h "surface simplification"): the surface of the height map thinned to a
  // right-triangle mesh whose midpoint errors stay within `tolerance`, in the map's height units.  Needs points from
  // setPointsFromHeightMap, unfiltered.  Points, normals and colours are replaced by the kept ones (normals and colours where they
  // match the points; set them before: the full-resolution normals are gathered, none are recomputed), faces() and saveMesh give the
  // simplified triangle list, and the surface is no GridMesh any longer: computeSurfaceNormals, renderView and photoConsistency
  // refuse it.  Returns the number of triangles; 0 when refused or when nothing is left.
  unsigned long simplifySurface(float tolerance) {
    const unsigned long cells = (unsigned long)surfaceFrame.w * surfaceFrame.h;
    if (refusesSimplified("simplifySurface")) return 0;
    if (points == nullptr || surfaceHeight == nullptr || surfaceHeight->size() != cells || !std::isfinite(tolerance)) {
      logger.err << "MeshFactory::simplifySurface: needs points from setPointsFromHeightMap and a finite tolerance";
      return 0;
    }
    const uint32_t w = surfaceFrame.w, h = surfaceFrame.h;
    const float* height = surfaceHeight->device.get();
    // the numbering of the points: the vertexIndex of the map's mesh at step 1
    ssrlcv_mesh_params meshParams = {1u, std::numeric_limits<float>::infinity()};
    const size_t meshWsb = ssrlcv_hip_disparity_mesh_workspace_bytes(w, h, &meshParams);
    const size_t wsb = std::max(meshWsb, ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(w, h));
    const unsigned long meshCells = (unsigned long)(w - 1) * (h - 1);
    ptr::device<unsigned char> gridCells(meshCells ? meshCells : 1);
    ptr::device<uint32_t> nodeIndex(cells), vertexIndex(cells), counts(2);
    DeviceScratch ws(wsb);
    HipSafeCall(ssrlcv_hip_disparity_mesh(height, w, h, &meshParams, nodeIndex.get(), gridCells.get(), counts.get(), ws.get(), wsb, nullptr));
    uint32_t c[2] = {0, 0};
    HipSafeCall(ssrlcv_hip_memcpy(c, counts.get(), 4, 1));
    if (c[0] != points->size()) {
      logger.err.printf("MeshFactory::simplifySurface: the map has %u valid cells, the cloud %lu points (filtered?)", c[0], points->size());
      return 0;
    }
    ptr::device<float> error(cells);
    HipSafeCall(ssrlcv_hip_dsm_simplify_errors(height, w, h, error.get(), nullptr));
    const int status = ssrlcv_hip_dsm_simplify_mesh(height, error.get(), w, h, tolerance, nodeIndex.get(), vertexIndex.get(), nullptr, 0, counts.get(),
                                                    nullptr, 0, counts.get() + 1, ws.get(), wsb, nullptr);
    if (status != SSRLCV_OK) {
      logger.err.printf("MeshFactory::simplifySurface: refused (%s)", ssrlcv_hip_status_string(status));
      return 0;
    }
    HipSafeCall(ssrlcv_hip_memcpy(c, counts.get(), 8, 1));
    const uint32_t t = c[0], m = c[1];
    clearSurface();
    if (t == 0) {
      points = ptr::value<Unity<float3>>();
      normals = ptr::value<Unity<float3>>();
      colors = ptr::value<Unity<unsigned char>>();
      return 0;
    }
    ptr::value<Unity<uint3>> tris(nullptr, (unsigned long)t, gpu);
    ptr::device<uint32_t> kept(m);
    HipSafeCall(ssrlcv_hip_dsm_simplify_mesh(height, error.get(), w, h, tolerance, nodeIndex.get(), vertexIndex.get(), (uint32_t*)tris->device.get(), t,
                                             counts.get(), kept.get(), m, counts.get() + 1, ws.get(), wsb, nullptr));
    std::vector<uint32_t> keptHost(m);
    HipSafeCall(ssrlcv_hip_memcpy(keptHost.data(), kept.get(), (size_t)m * 4, 1));
    const unsigned long n = points->size();
    const bool withNormals = normals != nullptr && normals->size() == n, withColors = colors != nullptr && colors->size() == n;
    points = gathered(points, keptHost);
    normals = withNormals ? gathered(normals, keptHost) : ptr::value<Unity<float3>>();
    colors = withColors ? gathered(colors, keptHost) : ptr::value<Unity<unsigned char>>();
    simplifiedFaces = tris;
    hasSimplified = true;
    logger.info.printf("MeshFactory::simplifySurface: %u of %lu vertices, %u of %lu triangles at tolerance %g", m, n, t, 2 * meshCells, (double)tolerance);
    return t;
  }

  // ---- the ortho-image (include/ssrlcv_hip.h "ortho-image"): the picture on the surface model.  generateOrthoImage on the fused,
  // filled height map, then setVertexColors(ortho, height) behind setPointsFromHeightMap(height, frame): saveMesh writes the greys.

  // the grey of every valid cell of `height` from 1 to 8 source images (uint8, cameras[k].size) and their cameras, each view tested
  // for occlusion by a march over the map; in state gpu, frame.w x frame.h, 0 where no view sees the cell; null when refused.
  // *seen and *which, when asked for, hold the views that see a cell as bits and the view its grey came from (0xFF: none).
  // The map and the images are left in the state they came in.
  static ptr::value<Unity<unsigned char>> generateOrthoImage(ptr::value<Unity<float>> height, const ssrlcv_dsm_frame& frame,
                                                             const std::vector<ptr::value<Unity<unsigned char>>>& images,
                                                             const std::vector<ssrlcv_camera>& cameras, const ssrlcv_ortho_params& params,
                                                             ptr::value<Unity<unsigned char>>* seen = nullptr,
                                                             ptr::value<Unity<unsigned char>>* which = nullptr) {
    const unsigned long cells = (unsigned long)frame.w * frame.h;
    if (height == nullptr || cells == 0 || height->size() != cells || images.empty() || images.size() > 8 || images.size() != cameras.size()) {
      logger.err << "MeshFactory::generateOrthoImage: needs a map of frame.w frame.h entries and 1 to 8 images with their cameras";
      return ptr::value<Unity<unsigned char>>();
    }
    std::vector<ssrlcv_ortho_view> views(images.size());
    std::deque<GpuRead<unsigned char>> imagesOnGpu;  // a deque constructs its guards in place
    for (size_t k = 0; k < images.size(); ++k) {
      views[k].image = nullptr;
      if (ssrlcv_dsm_ortho_view_host(&cameras[k], &frame, &views[k]) != SSRLCV_OK || images[k] == nullptr ||
          images[k]->size() != (unsigned long)views[k].w * views[k].h) {
        logger.err.printf("MeshFactory::generateOrthoImage: view %lu: a refused camera, or an image that has not its size", (unsigned long)k);
        return ptr::value<Unity<unsigned char>>();
      }
      imagesOnGpu.emplace_back(images[k]);
      views[k].image = images[k]->device.get();
    }
    GpuRead<float> heightOnGpu(height);
    DeviceScratch ws(ssrlcv_hip_dsm_ortho_workspace_bytes(frame.w, frame.h, (uint32_t)views.size()));
    ptr::value<Unity<unsigned char>> ortho(nullptr, cells, gpu);
    if (seen) *seen = ptr::value<Unity<unsigned char>>(nullptr, cells, gpu);
    if (which) *which = ptr::value<Unity<unsigned char>>(nullptr, cells, gpu);
    HipSafeCall(ssrlcv_hip_dsm_ortho(height->device.get(), &frame, views.data(), (uint32_t)views.size(), &params, ortho->device.get(),
                                     seen ? (*seen)->device.get() : nullptr, which ? (*which)->device.get() : nullptr, ws.get(), ws.bytes(), nullptr));
    return ortho;
  }

  // one grey a point: the ortho-image's bytes of the valid cells of `height` in raster order, the order setPointsFromHeightMap
  // gave the points of the same map.  In state cpu; both maps come back to the state they came in.
  void setVertexColors(ptr::value<Unity<unsigned char>> ortho, ptr::value<Unity<float>> height) {
    if (points == nullptr || ortho == nullptr || height == nullptr || ortho->size() != height->size()) {
      logger.err << "MeshFactory::setVertexColors: needs points, and an ortho-image and a height map of one grid";
      return;
    }
    std::vector<unsigned char> kept;
    {
      CpuRead<unsigned char> orthoOnCpu(ortho);
      CpuRead<float> heightOnCpu(height);
      const unsigned char* grey = ortho->host.get();
      const float* z = height->host.get();
      for (unsigned long c = 0; c < height->size(); ++c) {
        uint32_t bits;
        std::memcpy(&bits, z + c, 4);
        if (bits != 0x7FC00000u) kept.push_back(grey[c]);
      }
    }
    if (kept.size() != points->size()) {
      logger.err.printf("MeshFactory::setVertexColors: the map has %lu valid cells, the cloud %lu points", (unsigned long)kept.size(), points->size());
      return;
    }
    ptr::host<unsigned char> values((long)kept.size(), true);
    std::memcpy(values.get(), kept.data(), kept.size());
    colors = ptr::value<Unity<unsigned char>>(values, (unsigned long)kept.size(), cpu, true);
  }

  // ---- surface accuracy (include/ssrlcv_hip.h "surface accuracy"): how far a cloud lies from a reference surface -- upstream's
  // calculatePerPointDifference / calculateAverageDifference.  The reference is a height map on a ground grid, triangulated as
  // DisparityFactory::generateMesh(height, 1, maxJump) triangulates it; differences are measured along the frame's ez.

  struct AccuracyReport {
    unsigned long n = 0;  // the points
    double coverage = 0, bias = 0, nmad = 0, mean = 0, rms = 0, le68 = 0, le90 = 0, le95 = 0, min = 0, max = 0;  // NaN where there is no value
  };

  // the surface the differences are taken to: its own copy of the map, in state gpu, and the cells of its mesh at step 1
  void setReferenceSurface(ptr::value<Unity<float>> height, const ssrlcv_dsm_frame& frame, float maxJump = std::numeric_limits<float>::infinity()) {
    const unsigned long cells = (unsigned long)frame.w * frame.h;
    hasReference = false;
    if (height == nullptr || cells == 0 || height->size() != cells || !(maxJump >= 0.0f)) {
      logger.err << "MeshFactory::setReferenceSurface: the map has frame.w frame.h entries and maxJump is not negative";
      return;
    }
    referenceHeight = copyToGpu(height);
    referenceFrame = frame;
    const unsigned long meshCells = (unsigned long)(frame.w - 1) * (frame.h - 1);
    referenceCells = ptr::value<Unity<unsigned char>>(nullptr, meshCells ? meshCells : 1, gpu);  // never NULL: NULL would mean CELL mode
    ssrlcv_mesh_params params = {1u, maxJump};
    ptr::device<uint32_t> vertexIndex(cells), count(1);
    DeviceScratch ws(ssrlcv_hip_disparity_mesh_workspace_bytes(frame.w, frame.h, &params));
    HipSafeCall(ssrlcv_hip_disparity_mesh(referenceHeight->device.get(), frame.w, frame.h, &params, vertexIndex.get(), referenceCells->device.get(),
                                          count.get(), ws.get(), ws.bytes(), nullptr));
    hasReference = true;
  }

  // the signed difference of every point of `cloud` to the reference surface along planeNormal, which must be the reference
  // frame's ez (after normalising both in float, a dot product below 0.999999f is refused; another direction is out of scope);
  // in state gpu, 0x7FC00000 where there is no difference; null when refused.  The cloud is left in the state it came in.
  ptr::value<Unity<float>> calculatePerPointDifference(ptr::value<Unity<float3>> cloud, float3 planeNormal) {
    if (!hasReference || cloud == nullptr || cloud->size() == 0 || cloud->size() > 0xFFFFFFFFul) {
      logger.err << "MeshFactory::calculatePerPointDifference: needs a reference surface (setReferenceSurface) and points";
      return ptr::value<Unity<float>>();
    }
    const float* ez = referenceFrame.ez;
    const float ln = std::sqrt(planeNormal.x * planeNormal.x + planeNormal.y * planeNormal.y + planeNormal.z * planeNormal.z);
    const float le = std::sqrt(ez[0] * ez[0] + ez[1] * ez[1] + ez[2] * ez[2]);
    const float dot = (planeNormal.x / ln) * (ez[0] / le) + (planeNormal.y / ln) * (ez[1] / le) + (planeNormal.z / ln) * (ez[2] / le);
    if (!(dot >= 0.999999f)) {  // false for a NaN: a zero vector
      logger.err.printf("MeshFactory::calculatePerPointDifference: planeNormal is not the reference frame's ez (dot %g)", (double)dot);
      return ptr::value<Unity<float>>();
    }
    GpuRead<float3> onGpu(cloud);
    ptr::value<Unity<float>> diff(nullptr, cloud->size(), gpu);
    HipSafeCall(ssrlcv_hip_dsm_difference((const ssrlcv_float3*)cloud->device.get(), (uint32_t)cloud->size(), referenceHeight->device.get(),
                                          &referenceFrame, referenceCells->device.get(), diff->device.get(), nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
    return diff;
  }

  // the mean of the finite differences, in host float64 from the device's fixed-shape sums; NaN when there is none or when refused
  double calculateAverageDifference(ptr::value<Unity<float3>> cloud, float3 planeNormal) {
    auto diff = calculatePerPointDifference(cloud, planeNormal);
    if (diff == nullptr) return std::numeric_limits<double>::quiet_NaN();
    const ssrlcv_diff_stats s = differenceStats(diff, 0.0f, false, {});
    return s.finite ? s.sum / (double)s.finite : std::numeric_limits<double>::quiet_NaN();
  }

  // ssrlcv_hip_difference_stats of a Unity of differences -> the record on the host; the values come back to the state they came in
  static ssrlcv_diff_stats differenceStats(ptr::value<Unity<float>> values, float center, bool absolute, const std::vector<uint32_t>& quantiles) {
    ssrlcv_diff_stats_params params = {center, absolute ? 1u : 0u, (uint32_t)quantiles.size(), {0, 0, 0, 0, 0, 0, 0, 0}};
    for (size_t k = 0; k < quantiles.size() && k < 8; ++k) params.quantile[k] = quantiles[k];
    GpuRead<float> onGpu(values);
    ptr::device<ssrlcv_diff_stats> record(1);
    DeviceScratch ws(ssrlcv_hip_difference_stats_workspace_bytes((uint32_t)values->size(), &params));
    HipSafeCall(ssrlcv_hip_difference_stats(values->device.get(), (uint32_t)values->size(), &params, record.get(), ws.get(), ws.bytes(), nullptr));
    ssrlcv_diff_stats host;
    HipSafeCall(ssrlcv_hip_memcpy(&host, record.get(), sizeof host, 1));
    return host;
  }

  // pipeline.surface_accuracy's fields for `cloud` against the reference surface: three statistics calls on the differences
  AccuracyReport accuracyReport(ptr::value<Unity<float3>> cloud, ptr::value<Unity<float>>* differences = nullptr) {
    AccuracyReport r;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    r.coverage = r.bias = r.nmad = r.mean = r.rms = r.le68 = r.le90 = r.le95 = r.min = r.max = nan;
    if (!hasReference) {
      logger.err << "MeshFactory::accuracyReport: needs a reference surface (setReferenceSurface)";
      return r;
    }
    auto diff = calculatePerPointDifference(cloud, {referenceFrame.ez[0], referenceFrame.ez[1], referenceFrame.ez[2]});
    if (diff == nullptr) return r;
    if (differences) *differences = diff;
    const ssrlcv_diff_stats s = differenceStats(diff, 0.0f, false, {5000u});
    r.n = s.n;
    r.coverage = (double)s.finite / (double)s.n;
    if (s.finite == 0) return r;
    r.bias = s.quantile[0];
    r.mean = s.sum / (double)s.finite;
    r.rms = std::sqrt(s.sumSq / (double)s.finite);
    r.min = s.min;
    r.max = s.max;
    r.nmad = 1.4826 * (double)differenceStats(diff, s.quantile[0], true, {5000u}).quantile[0];
    const ssrlcv_diff_stats a = differenceStats(diff, 0.0f, true, {6827u, 9000u, 9500u});
    r.le68 = a.quantile[0];
    r.le90 = a.quantile[1];
    r.le95 = a.quantile[2];
    return r;
  }

  // ---- surface registration (include/ssrlcv_hip.h "surface registration"): the pose that aligns a cloud to the reference surface
  // by point-to-plane steps -- pipeline.surface_register's loop, call for call.  dofMask bits 0..6 = tx, ty, tz, rx, ry, rz, scale
  // (0x07 a shift, 0x3F rigid, 0x7F a similarity); gateFactor > 0: only points within gateFactor x NMAD of the median difference
  // take part, otherwise all that have one.  The cloud is not moved (PointCloudFactory::transformPointCloud does that) and is
  // left in the state it came in.
  struct RegistrationStep {
    uint32_t used = 0, inside = 0;
    double rms = 0, center = 0, gate = 0;
    double delta[7] = {0, 0, 0, 0, 0, 0, 0};
    bool stepped = false;  // false: the step was refused and delta holds nothing
  };
  struct Registration {
    ssrlcv_register_pose pose = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 0, 0}};
    bool converged = false;
    std::vector<RegistrationStep> history;
  };

  Registration registerToReference(ptr::value<Unity<float3>> cloud, uint32_t dofMask = 0x3Fu, unsigned iterations = 8, float gateFactor = 3.0f,
                                   double damping = 0.0) {
    return registerToReference(cloud, Registration().pose, dofMask, iterations, gateFactor, damping);
  }

  // the same from a start pose -- searchShift's, for a cloud that lies many cells off; its pivot is replaced like the identity's
  Registration registerToReference(ptr::value<Unity<float3>> cloud, const ssrlcv_register_pose& start, uint32_t dofMask = 0x3Fu, unsigned iterations = 8,
                                   float gateFactor = 3.0f, double damping = 0.0) {
    Registration reg;
    reg.pose = start;
    if (!hasReference || cloud == nullptr || cloud->size() == 0 || cloud->size() > 0xFFFFFFFFul) {
      logger.err << "MeshFactory::registerToReference: needs a reference surface (setReferenceSurface) and points";
      return reg;
    }
    const uint32_t n = (uint32_t)cloud->size();
    GpuRead<float3> onGpu(cloud);
    const ssrlcv_float3* points =(const ssrlcv_float3*)cloud->device.get();
    ptr::value<Unity<float3>> posed(nullptr, n, gpu);
    ptr::value<Unity<float>> diff(nullptr, n, gpu);
    auto difference = [&]() {
      HipSafeCall(ssrlcv_hip_transform_points(points, n, &reg.pose, (ssrlcv_float3*)posed->device.get(), nullptr));
      HipSafeCall(ssrlcv_hip_dsm_difference((const ssrlcv_float3*)posed->device.get(), n, referenceHeight->device.get(), &referenceFrame,
                                            referenceCells->device.get(), diff->device.get(), nullptr));
      HipSafeCall(ssrlcv_hip_device_synchronize());
    };
    // the pivot: the float64 mean of the points that have a difference under the initial pose; the corners of the cloud's box
    difference();
    std::vector<float3> posedHost(n), cloudHost(n);
    std::vector<uint32_t> diffBits(n);
    HipSafeCall(ssrlcv_hip_memcpy(posedHost.data(), posed->device.get(), (size_t)n * sizeof(float3), 1));
    HipSafeCall(ssrlcv_hip_memcpy(cloudHost.data(), points, (size_t)n * sizeof(float3), 1));
    HipSafeCall(ssrlcv_hip_memcpy(diffBits.data(), diff->device.get(), (size_t)n * sizeof(float), 1));
    double sum[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    unsigned long has = 0, kept = 0;
    for (uint32_t k = 0; k < n; ++k) {
      const float c[3] = {cloudHost[k].x, cloudHost[k].y, cloudHost[k].z};
      if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) || (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f)) continue;
      for (int a = 0; a < 3; ++a) {
        lo[a] = kept ? std::min(lo[a], (double)c[a]) : (double)c[a];
        hi[a] = kept ? std::max(hi[a], (double)c[a]) : (double)c[a];
      }
      ++kept;
      if (diffBits[k] == 0x7FC00000u) continue;
      sum[0] += (double)posedHost[k].x, sum[1] += (double)posedHost[k].y, sum[2] += (double)posedHost[k].z;
      ++has;
    }
    for (int a = 0; a < 3; ++a) reg.pose.pivot[a] = has ? (float)(sum[a] / (double)has) : 0.0f;
    ptr::device<ssrlcv_register_terms> record(1);
    DeviceScratch ws(ssrlcv_hip_register_terms_workspace_bytes(n));
    const double inf = std::numeric_limits<double>::infinity();
    for (unsigned it = 0; it < iterations; ++it) {
      ssrlcv_register_params params = {0.0f, (float)inf};
      if (gateFactor > 0.0f) {
        difference();
        const ssrlcv_diff_stats s = differenceStats(diff, 0.0f, false, {5000u});
        if (s.finite == 0) break;
        params.center = s.quantile[0];
        params.gate = (float)((double)gateFactor * (1.4826 * (double)differenceStats(diff, params.center, true, {5000u}).quantile[0]));
      }
      HipSafeCall(ssrlcv_hip_register_terms(points, n, &reg.pose, referenceHeight->device.get(), &referenceFrame, referenceCells->device.get(), &params,
                                            record.get(), ws.get(), ws.bytes(), nullptr));
      ssrlcv_register_terms terms;
      HipSafeCall(ssrlcv_hip_memcpy(&terms, record.get(), sizeof terms, 1));
      RegistrationStep step;
      step.used = terms.used, step.inside = terms.inside;
      step.rms = terms.used ? std::sqrt(terms.ee / (double)terms.used) : std::numeric_limits<double>::quiet_NaN();
      step.center = params.center, step.gate = params.gate;
      step.stepped = ssrlcv_register_step_host(&terms, dofMask, damping, step.delta) == SSRLCV_OK;
      reg.history.push_back(step);
      if (!step.stepped) break;
      ssrlcv_register_pose next;
      if (ssrlcv_register_compose_host(&reg.pose, step.delta, &next) != SSRLCV_OK) break;
      double moved = 0.0;  // the largest displacement of a corner of the cloud's box
      for (int k = 0; k < 8 && kept; ++k) {
        const double c[3] = {(k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]};
        double d2 = 0.0;
        for (int r = 0; r < 3; ++r) {
          const float *a = reg.pose.m + 4 * r, *b = next.m + 4 * r;
          const double before = (c[0] * (double)a[0] + c[1] * (double)a[1] + c[2] * (double)a[2]) + (double)a[3];
          const double after = (c[0] * (double)b[0] + c[1] * (double)b[1] + c[2] * (double)b[2]) + (double)b[3];
          d2 += (after - before) * (after - before);
        }
        moved = std::max(moved, std::sqrt(d2));
      }
      reg.pose = next;
      if (moved <= 1e-3 * (double)referenceFrame.cell) {
        reg.converged = true;
        break;
      }
    }
    return reg;
  }

  // ---- shift search (include/ssrlcv_hip.h "shift search"): the whole-cell shift that lays a height map tens of cells off onto a
  // reference map of the same grid, coarse to fine -- pipeline.surface_shift_search on two maps, call for call.  `moving` is
  // generateHeightMap(frame, rule) of the subject cloud.  One ssrlcv_hip_shift_search a level: the first at strides[0], centred on
  // 0 with `radius`; each later one centred on the shift found so far with radius ceil(g_prev / g) + 1.  gateFactor > 0: only
  // differences within gateFactor x NMAD of the median at the level's centre shift take part (objectHeights of the two overlapping
  // slices, two differenceStats).  scale 0: 64 / cell.  minOverlap: the share of the level's valid moving cells a shift needs.
  // `pose` is `start` (null: the identity) with T moved by cell (x ex + y ey) - bias ez, which is exact for an orthonormal frame:
  // registerToReference(cloud, pose, ..) takes it as its start.  found is false when a call is refused or a level has no candidate.
  struct ShiftLevel {
    ssrlcv_shift_params params;
    ssrlcv_shift_result result;
    std::vector<unsigned char> table;  // as the device wrote it: the head, then the entries
  };
  struct ShiftSearch {
    bool found = false;
    double shiftX = 0, shiftY = 0;  // in cells, the last level's best shift with its sub-cell step
    ssrlcv_shift_result result = {};
    ssrlcv_register_pose pose = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 0, 0}};
    std::vector<ShiftLevel> levels;
  };

  static ShiftSearch searchShift(ptr::value<Unity<float>> moving, ptr::value<Unity<float>> reference, const ssrlcv_dsm_frame& frame, uint32_t radius = 8,
                                 const std::vector<uint32_t>& strides = {4u, 1u}, float gateFactor = 3.0f, float scale = 0.0f, double minOverlap = 0.25,
                                 const ssrlcv_register_pose* start = nullptr) {
    ShiftSearch found;
    const uint32_t w = frame.w, h = frame.h;
    const unsigned long cells = (unsigned long)w * h;
    if (moving == nullptr || reference == nullptr || cells == 0 || moving->size() != cells || reference->size() != cells || strides.empty()) {
      logger.err << "MeshFactory::searchShift: both maps have the frame's w h entries, and there is a stride";
      return found;
    }
    if (start) found.pose = *start;
    GpuRead<float> movingOnGpu(moving), referenceOnGpu(reference);
    std::vector<float> hostM(cells), hostR(cells);  // the gate's slices are cut on the host
    HipSafeCall(ssrlcv_hip_memcpy(hostM.data(), moving->device.get(), cells * sizeof(float), 1));
    HipSafeCall(ssrlcv_hip_memcpy(hostR.data(), reference->device.get(), cells * sizeof(float), 1));
    const double cell = (double)frame.cell;
    const float quanta = scale > 0.0f ? scale : (float)(64.0 / cell);
    int64_t best[2] = {0, 0};
    bool ok = true;
    for (size_t k = 0; k < strides.size() && ok; ++k) {
      const uint32_t g = strides[k];
      if (g == 0) { ok = false; break; }
      ShiftLevel level;
      level.params.scale = quanta;
      level.params.stride = g;
      level.params.centerX = k == 0 ? 0 : (int32_t)std::floor((double)best[0] / (double)g + 0.5);
      level.params.centerY = k == 0 ? 0 : (int32_t)std::floor((double)best[1] / (double)g + 0.5);
      level.params.radius = k == 0 ? radius : (strides[k - 1] + g - 1u) / g + 1u;
      level.params.centerQ = 0;
      level.params.gateQ = 0xFFFFFFFFu;
      const uint32_t sw = (uint32_t)(((uint64_t)w + g - 1u) / g), sh = (uint32_t)(((uint64_t)h + g - 1u) / g);
      if (gateFactor > 0.0f) {  // the median and the NMAD of the differences at the centre shift, in quanta
        const int64_t cx = level.params.centerX, cy = level.params.centerY;
        const int64_t x0 = std::max<int64_t>(0, -cx), x1 = std::min<int64_t>(sw, (int64_t)sw - cx);
        const int64_t y0 = std::max<int64_t>(0, -cy), y1 = std::min<int64_t>(sh, (int64_t)sh - cy);
        if (x1 > x0 && y1 > y0) {
          const unsigned long sliceW = (unsigned long)(x1 - x0), sliceH = (unsigned long)(y1 - y0);
          ptr::host<float> a((long)(sliceW * sliceH), true), b((long)(sliceW * sliceH), true);
          for (unsigned long y = 0; y < sliceH; ++y)
            for (unsigned long x = 0; x < sliceW; ++x) {
              a.get()[y * sliceW + x] = hostM[(size_t)((y0 + (int64_t)y) * g) * w + (size_t)((x0 + (int64_t)x) * g)];
              b.get()[y * sliceW + x] = hostR[(size_t)((y0 + cy + (int64_t)y) * g) * w + (size_t)((x0 + cx + (int64_t)x) * g)];
            }
          ptr::value<Unity<float>> sliceM(a, sliceW * sliceH, cpu, true), sliceR(b, sliceW * sliceH, cpu, true);
          auto diff = objectHeights(sliceM, sliceR, (unsigned int)sliceW, (unsigned int)sliceH);
          const ssrlcv_diff_stats s = differenceStats(diff, 0.0f, false, {5000u});
          if (s.finite != 0) {
            const double mad = (double)differenceStats(diff, s.quantile[0], true, {5000u}).quantile[0];
            const double cq = std::nearbyint((double)s.quantile[0] * (double)quanta);
            const double gq = std::floor((double)gateFactor * (1.4826 * mad) * (double)quanta);
            level.params.centerQ = (int32_t)std::max(-262144.0, std::min(262144.0, cq));
            level.params.gateQ = (uint32_t)std::max(0.0, std::min(4294967294.0, gq));
          }
        }
      }
      const size_t tableBytes = ssrlcv_shift_table_bytes(level.params.radius);
      if (tableBytes == 0) { ok = false; break; }
      ptr::device<unsigned char> table(tableBytes);
      DeviceScratch ws(ssrlcv_hip_shift_search_workspace_bytes(w, h, &level.params));
      const int status = ssrlcv_hip_shift_search(moving->device.get(), reference->device.get(), w, h, &level.params, (ssrlcv_shift_table*)table.get(), ws.get(),
                                                 ws.bytes(), nullptr);
      if (status != SSRLCV_OK) {
        logger.err.printf("MeshFactory::searchShift: refused (%s)", ssrlcv_hip_status_string(status));
        ok = false;
        break;
      }
      level.table.resize(tableBytes);
      HipSafeCall(ssrlcv_hip_memcpy(level.table.data(), table.get(), tableBytes, 1));
      ssrlcv_shift_table head;
      std::memcpy(&head, level.table.data(), sizeof head);
      const uint32_t least = (uint32_t)(minOverlap * (double)head.validMoving);
      if (ssrlcv_shift_pick_host((const ssrlcv_shift_table*)level.table.data(), tableBytes, &level.params, least, &level.result) != SSRLCV_OK) {
        logger.err.printf("MeshFactory::searchShift: no shift of level %zu has the overlap asked for", k);
        ok = false;
        break;
      }
      best[0] = level.result.shiftX, best[1] = level.result.shiftY;
      found.levels.push_back(level);
    }
    if (!ok || found.levels.empty()) return found;
    found.result = found.levels.back().result;
    found.shiftX = (double)best[0] + found.result.subX;
    found.shiftY = (double)best[1] + found.result.subY;
    for (int r = 0; r < 3; ++r) {
      const double along = cell * (found.shiftX * (double)frame.ex[r] + found.shiftY * (double)frame.ey[r]);
      found.pose.m[4 * r + 3] = (float)(((double)found.pose.m[4 * r + 3] + along) - found.result.bias * (double)frame.ez[r]);
    }
    found.found = true;
    return found;
  }

  // ---- mesh render (include/ssrlcv_hip.h "mesh render"): the surface drawn into a camera, and compared with that camera's own
  // picture -- an accuracy measure that needs no reference surface.  Needs points with a surface (setPointsFromHeightMap, then
  // setSurface(DisparityFactory::generateMesh(height, 1, maxJump))); the greys are `colors` (setVertexColors), 0 without.
  struct RenderedView {
    unsigned int w = 0, h = 0;                   // the camera's image
    ptr::value<Unity<float>> depth;              // in state gpu: the distance along the optical axis, 0x7FC00000 where nothing was drawn
    ptr::value<Unity<unsigned int>> triangle;    // 2 cell + t of the surface's grid, UINT32_MAX for none
    ptr::value<Unity<unsigned char>> shade;      // the vertices' greys, interpolated; 0 where nothing was drawn
    uint32_t drawn = 0, tooLarge = 0, unusable = 0;  // triangles drawn, skipped as above maxExtent pixels, skipped for a corner or no area
  };
  struct PhotoConsistency {
    double coverage = 0, median = 0, nmad = 0, rms = 0;  // of image minus model, in grey levels; NaN where there is no value
    RenderedView view;
    ptr::value<Unity<float>> residual;           // in state gpu, 0x7FC00000 where nothing was drawn
  };

  // pipeline.surface_render's maps; depth is null when refused.  The points and the colours are left in the state they came in.
  RenderedView renderView(const Image::Camera& camera, const ssrlcv_dsm_frame& frame, uint32_t maxExtent = 8) {
    RenderedView r;
    ssrlcv_ortho_view view;
    view.image = nullptr;
    const bool colored = colors != nullptr && points != nullptr && colors->size() == points->size();
    if (refusesSimplified("renderView")) return r;
    if (!hasSurface || points == nullptr || surface.vertexCount != points->size() || points->size() > 0xFFFFFFFFul ||
        ssrlcv_dsm_ortho_view_host((const ssrlcv_camera*)&camera, &frame, &view) != SSRLCV_OK) {
      logger.err << "MeshFactory::renderView: needs a surface of these points (setSurface) and a camera the ortho-image takes";
      return r;
    }
    GpuRead<float3> onGpu(points);
    GpuRead<unsigned char> colorsOnGpu(colored ? colors : ptr::value<Unity<unsigned char>>());
    const uint32_t n = (uint32_t)points->size();
    const unsigned long pixels = (unsigned long)view.w * view.h;
    const ssrlcv_render_params params = {maxExtent};
    ptr::device<uint32_t> counts(3);
    DeviceScratch ws(ssrlcv_hip_mesh_render_workspace_bytes(n, view.w, view.h));
    r.w = view.w, r.h = view.h;
    r.depth = ptr::value<Unity<float>>(nullptr, pixels, gpu);
    r.triangle = ptr::value<Unity<unsigned int>>(nullptr, pixels, gpu);
    r.shade = ptr::value<Unity<unsigned char>>(nullptr, pixels, gpu);
    const int status = ssrlcv_hip_mesh_render((const ssrlcv_float3*)points->device.get(), n, colored ? colors->device.get() : nullptr,
                                              surface.vertexIndex->device.get(), surface.cells->device.get(), surface.gw, surface.gh, &view, &params,
                                              r.depth->device.get(), r.triangle->device.get(), r.shade->device.get(), counts.get(), ws.get(), ws.bytes(), nullptr);
    if (status == SSRLCV_OK) {
      uint32_t c[3] = {0, 0, 0};
      HipSafeCall(ssrlcv_hip_memcpy(c, counts.get(), sizeof c, 1));
      r.drawn = c[0], r.tooLarge = c[1], r.unusable = c[2];
    } else {
      logger.err.printf("MeshFactory::renderView: refused (%s)", ssrlcv_hip_status_string(status));
      r = RenderedView();
    }
    return r;
  }

  // pipeline.surface_photo_check's figures for `image` (uint8, the camera's size), the picture `camera` took: the surface with its
  // colours drawn into the camera, subtracted from the image, through the statistics as it is.  The image is left in its state.
  PhotoConsistency photoConsistency(ptr::value<Unity<unsigned char>> image, const Image::Camera& camera, const ssrlcv_dsm_frame& frame,
                                    uint32_t maxExtent = 8) {
    PhotoConsistency p;
    p.coverage = p.median = p.nmad = p.rms = std::numeric_limits<double>::quiet_NaN();
    if (refusesSimplified("photoConsistency")) return p;
    p.view = renderView(camera, frame, maxExtent);
    if (p.view.depth == nullptr || image == nullptr || image->size() != (unsigned long)p.view.w * p.view.h) {
      logger.err << "MeshFactory::photoConsistency: needs a view that renders and an image of the camera's size";
      return p;
    }
    p.residual = ptr::value<Unity<float>>(nullptr, image->size(), gpu);
    {
      GpuRead<unsigned char> onGpu(image);
      HipSafeCall(ssrlcv_hip_image_residual(image->device.get(), p.view.shade->device.get(), p.view.depth->device.get(), p.view.w, p.view.h,
                                            p.residual->device.get(), nullptr));
      HipSafeCall(ssrlcv_hip_device_synchronize());
    }
    const ssrlcv_diff_stats s = differenceStats(p.residual, 0.0f, false, {5000u});
    p.coverage = (double)s.finite / (double)s.n;
    if (s.finite == 0) return p;
    p.median = s.quantile[0];
    p.rms = std::sqrt(s.sumSq / (double)s.finite);
    p.nmad = 1.4826 * (double)differenceStats(p.residual, s.quantile[0], true, {5000u}).quantile[0];
    return p;
  }

  ptr::value<Unity<float>> referenceHeight;           // set by setReferenceSurface, in state gpu
  ptr::value<Unity<unsigned char>> referenceCells;
  ssrlcv_dsm_frame referenceFrame = {};
  bool hasReference = false;

  // ASCII PLY of the points (and their normals once computed) as <dir><filename>.ply
  void savePoints(std::string filename, std::string dir = "out/") {
    if (points == nullptr) return;
    if (normals != nullptr && normals->size() == points->size()) writePLY(filename, points, normals, dir);
    else writePLY(filename, points, dir);
  }

  // ASCII PLY of the points, their normals once computed, their greys once set (uchar red green blue, the grey three times), and
  // the surface's triangles as <dir><filename>.ply
  void saveMesh(std::string filename, std::string dir = "out/") {
    if (points == nullptr) return;
    const bool withNormals = normals != nullptr && normals->size() == points->size();
    if (colors != nullptr && colors->size() == points->size())
      writePLY(filename, points, withNormals ? normals : ptr::value<Unity<float3>>(), colors, faces(), dir);
    else
      writePLY(filename, points, withNormals ? normals : ptr::value<Unity<float3>>(), faces(), dir);
  }
};

}  // namespace ssrlcv
