// ssrlcv_amd/host/DisparityFactory.hpp -- dense stereo through the class API: this project's form of upstream's pair of a
// Window_NxN feature factory and MatchFactory<Window_NxN>'s disparity matcher.  Upstream fills one window descriptor per
// pixel (up to 961 bytes) and runs its generic matcher over them; here two rectified Images go in and the C ABI's
// ssrlcv_hip_stereo_sad_u8 works from their pixels directly (include/ssrlcv_hip.h "dense stereo" is the contract).
//
//   DisparityFactory factory(4);                    // 9 x 9 windows (Window_9x9); radius 1, 4, 7, 12, 15 are upstream's sizes
//   factory.setDisparityRange(0, 64);
//   auto disparity = factory.generateDisparities(left, right);        // Unity<float>, w x h, gpu; invalid = NaN 0x7FC00000
//   auto matches = factory.generateMatches(disparity, left, right);   // Unity<Match>, gpu: the sparse path's records
//   auto cloud = PointCloudFactory().stereo_disparity(matches, foc, baseline, doffset);
//
// Semi-global matching over the same costs (include/ssrlcv_hip.h "semi-global matching") is one setter away; the maps and
// everything after them are the same:
//
//   factory.setSemiGlobal(1000, 40, 400);           // costClamp, P1, P2, paths = 0xFF; clearSemiGlobal() returns to SAD winners
//
// The census cost (include/ssrlcv_hip.h "census cost") is another setter, for block matching and semi-global matching alike;
// the radius is then the AGGREGATION radius (0 .. 7, 0 being the usual form under semi-global matching):
//
//   factory.setCensus(2);                           // 5 x 5 census codes; clearCensus() returns to SAD costs
//
// An unrectified pair of pinhole Images goes through rectify() first (include/ssrlcv_hip.h "rectification"):
//
//   ptr::value<Image> leftR, rightR;
//   Rectification rect = factory.rectify(left, right, leftR, rightR);  // from left->camera, right->camera
//   auto disparity = factory.generateDisparities(leftR, rightR);
//   factory.maskRectified(disparity, nullptr, rect);                   // the windows that left a source image
//   auto matches = factory.generateMatches(disparity, left, right);
//   factory.unrectifyMatches(matches, rect);                           // source pixels: triangulate with the original cameras
//
// The map-domain post-filters (include/ssrlcv_hip.h "disparity post-filters") are two explicit steps between the map and the
// matches, behind maskRectified where there is one; the median first is the usual order:
//
//   disparity = factory.medianFilter(disparity, 1);                    // a new map: the lower median of the valid 3 x 3 neighbours
//   factory.filterSpeckles(disparity, nullptr, 200, 1.0f);             // in place: components of at most 200 pixels become invalid
//   disparity = factory.fillHoles(disparity, 0xFF, 32, 5, 0);          // a new map: holes take the smallest of >= 5 measured neighbours
//
// The surface of the final map (include/ssrlcv_hip.h "disparity mesh"), with the vertex numbering of generateMatches' records at
// the same step, goes to a MeshFactory beside the cloud of those records:
//
//   GridMesh surface = factory.generateMesh(disparity, 1, 1.0f);       // triangles over the step-1 grid, cut at jumps above 1
//   meshFactory.setPoints(cloud); meshFactory.setSurface(surface); meshFactory.computeSurfaceNormals();
//
// Pixels and maps are on the gpu for the call and leave it in the state they came in (Scoped.hpp).
#pragma once
#include "GridMesh.hpp"
#include "Image.hpp"
#include "MatchFactory.hpp"
#include "Scoped.hpp"

namespace ssrlcv {

typedef ssrlcv_rectification Rectification;

class DisparityFactory {
  ssrlcv_stereo_params params;
  unsigned int step = 1;
  bool semiGlobal = false;
  unsigned int sgmClamp = 0, sgmP1 = 0, sgmP2 = 0, sgmPaths = 0xFFu;
  unsigned int census = 0;  // 0: SAD costs
  uint2 mapSize = {0u, 0u};  // of the last generateDisparities: a Unity<float> does not carry its width

  static const ptr::value<Unity<unsigned char>>& grey(const ptr::value<Image>& image) {
    if (image->colorDepth != 1) {
      logger.err << "ERROR: dense stereo takes single-channel images (convertToBW first)";
      std::exit(-1);
    }
    return image->pixels;
  }

 public:
  explicit DisparityFactory(unsigned int radius = 4) {
    params.radius = radius;
    params.minDisparity = 0;
    params.numDisparities = 64;
    params.maxCost = 0xFFFFFFFFu;
    params.lrTolerance = 1;
    params.subpixel = 1;
  }
  void setRadius(unsigned int radius) { params.radius = radius; }
  void setDisparityRange(int minDisparity, unsigned int numDisparities) {
    params.minDisparity = minDisparity;
    params.numDisparities = numDisparities;
  }
  void setMaxCost(unsigned int maxCost) { params.maxCost = maxCost; }  // 0xFFFFFFFF: no limit
  void setLeftRightTolerance(int tolerance) { params.lrTolerance = tolerance; }  // < 0: no check
  void setSubpixel(bool on) { params.subpixel = on ? 1u : 0u; }
  void setStep(unsigned int s) { step = s; }  // generateMatches takes every s-th pixel of every s-th row
  // generateDisparities aggregates the clamped costs along the directions of `paths` (ssrlcv_hip_stereo_sgm_u8) instead of
  // taking each pixel's own winner; it has no cost limit, so maxCost must stay at "no limit"
  void setSemiGlobal(unsigned int costClamp, unsigned int P1, unsigned int P2, unsigned int paths = 0xFFu) {
    semiGlobal = true;
    sgmClamp = costClamp;
    sgmP1 = P1;
    sgmP2 = P2;
    sgmPaths = paths;
  }
  void clearSemiGlobal() { semiGlobal = false; }
  // the matching cost becomes the Hamming distance of (2 censusRadius + 1)^2 census codes (ssrlcv_hip_stereo_census_u8,
  // ssrlcv_hip_stereo_sgm_census_u8), censusRadius 1, 2 or 3; the radius is then the aggregation radius, 0 .. 7
  void setCensus(unsigned int censusRadius) { census = censusRadius; }
  void clearCensus() { census = 0; }
  // the radius of everything a pixel's cost reads: what maskRectified masks with
  unsigned int footprintRadius() const { return params.radius + census; }
  // the size of the maps filterSpeckles and medianFilter take; generateDisparities sets it to its pair's
  void setMapSize(unsigned int w, unsigned int h) { mapSize = uint2{w, h}; }

  // disparity of every left pixel (row-major, w x h), in state gpu; `cost` (optional out) receives the winners' costs
  ptr::value<Unity<float>> generateDisparities(ptr::value<Image> left, ptr::value<Image> right,
                                               ptr::value<Unity<unsigned int>>* cost = nullptr) {
    if (left->size.x != right->size.x || left->size.y != right->size.y) {
      logger.err << "ERROR: a rectified pair has two images of one size";
      std::exit(-1);
    }
    const uint32_t w = left->size.x, h = left->size.y;
    mapSize = uint2{w, h};
    ssrlcv_sgm_params sgm;
    sgm.radius = params.radius;
    sgm.minDisparity = params.minDisparity;
    sgm.numDisparities = params.numDisparities;
    sgm.costClamp = sgmClamp;
    sgm.P1 = sgmP1;
    sgm.P2 = sgmP2;
    sgm.paths = sgmPaths;
    sgm.lrTolerance = params.lrTolerance;
    sgm.subpixel = params.subpixel;
    if (semiGlobal && params.maxCost != 0xFFFFFFFFu) {
      logger.err << "ERROR: semi-global matching has no cost limit (setMaxCost(0xFFFFFFFF) or clearSemiGlobal())";
      std::exit(-1);
    }
    const size_t wsBytes = census ? (semiGlobal ? ssrlcv_hip_stereo_sgm_census_workspace_bytes(w, h, &sgm, census)
                                                : ssrlcv_hip_stereo_census_workspace_bytes(w, h, &params, census))
                                  : (semiGlobal ? ssrlcv_hip_stereo_sgm_workspace_bytes(w, h, &sgm) : ssrlcv_hip_stereo_workspace_bytes(w, h, &params));
    if (wsBytes == 0) {
      if (census)
        logger.err << "ERROR: census parameters outside the contract (census radius 1..3, aggregation radius 0..7, and the SAD call's other limits)";
      else if (semiGlobal)
        logger.err << "ERROR: semi-global parameters outside the contract (P1 <= P2, paths 1..0xFF, popcount(paths) (costClamp + P2) <= 65535)";
      else
        logger.err << "ERROR: dense stereo parameters outside the contract (radius 1..15, 1..256 disparities from -32768..32767)";
      std::exit(-1);
    }
    GpuRead<unsigned char> leftOnGpu(grey(left)), rightOnGpu(grey(right));
    const unsigned long n = (unsigned long)w * h;
    DeviceScratch workspace(wsBytes);
    ptr::value<Unity<float>> disparity(nullptr, n ? n : 1ul, gpu);
    ptr::value<Unity<unsigned int>> costs;
    if (cost) costs = ptr::value<Unity<unsigned int>>(nullptr, n ? n : 1ul, gpu);
    if (census && semiGlobal)
      HipSafeCall(ssrlcv_hip_stereo_sgm_census_u8(left->pixels->device.get(), right->pixels->device.get(), w, h, &sgm, census, workspace.get(), wsBytes,
                                                  disparity->device.get(), cost ? costs->device.get() : nullptr, nullptr));
    else if (census)
      HipSafeCall(ssrlcv_hip_stereo_census_u8(left->pixels->device.get(), right->pixels->device.get(), w, h, &params, census, workspace.get(), wsBytes,
                                              disparity->device.get(), cost ? costs->device.get() : nullptr, nullptr));
    else if (semiGlobal)
      HipSafeCall(ssrlcv_hip_stereo_sgm_u8(left->pixels->device.get(), right->pixels->device.get(), w, h, &sgm, workspace.get(), wsBytes,
                                           disparity->device.get(), cost ? costs->device.get() : nullptr, nullptr));
    else
      HipSafeCall(ssrlcv_hip_stereo_sad_u8(left->pixels->device.get(), right->pixels->device.get(), w, h, &params, workspace.get(), wsBytes,
                                           disparity->device.get(), cost ? costs->device.get() : nullptr, nullptr));
    HipCheckError();
    if (cost) *cost = costs;
    return disparity;
  }

  // the valid pixels of the step grid as Match records {left id, (x, y)} / {right id, (x - disparity, y)}, in state gpu
  ptr::value<Unity<Match>> generateMatches(ptr::value<Unity<float>> disparity, ptr::value<Image> left, ptr::value<Image> right) {
    const uint32_t w = left->size.x, h = left->size.y;
    const size_t wsBytes = ssrlcv_hip_stereo_matches_workspace_bytes(w, h, step);
    if (wsBytes == 0) {
      logger.err << "ERROR: the sampling step of dense stereo matches is at least 1";
      std::exit(-1);
    }
    GpuRead<float> onGpu(disparity);
    // samples per row and column: ceil(n / step) without the sum n + step - 1, which wraps for a step near 2^32
    const uint32_t cap = (w ? (w - 1) / step + 1 : 0) * (h ? (h - 1) / step + 1 : 0);
    ptr::device<Match> staging((long)(cap ? cap : 1));
    ptr::device<uint32_t> countDev(1);
    DeviceScratch workspace(wsBytes);
    uint32_t count = 0;
    HipSafeCall(ssrlcv_hip_stereo_matches(disparity->device.get(), w, h, step, left->id, right->id,
                                          reinterpret_cast<ssrlcv_match*>(staging.get()), cap, countDev.get(), workspace.get(), wsBytes, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_memcpy(&count, countDev.get(), sizeof count, 1));
    if (count == 0) {
      logger.err << "ERROR: dense stereo left no valid pixel";
      std::exit(0);
    }
    if (count == cap) return ptr::value<Unity<Match>>(staging, (unsigned long)count, gpu);
    ptr::device<Match> exact((long)count);
    HipSafeCall(ssrlcv_hip_memcpy(exact.get(), staging.get(), (size_t)count * sizeof(Match), 2));
    return ptr::value<Unity<Match>>(exact, (unsigned long)count, gpu);
  }

  // the pair warped by the homographies of ssrlcv_rectify_cameras_host(left->camera, right->camera): two new single-channel
  // Images in state gpu with the sources' ids; the returned record holds the homographies and the rectified pair's foc,
  // baseline, doffset and principal point (PointCloudFactory::stereo_disparity's parameters)
  Rectification rectify(ptr::value<Image> left, ptr::value<Image> right, ptr::value<Image>& leftOut, ptr::value<Image>& rightOut) {
    Rectification rect;
    const int rc = ssrlcv_rectify_cameras_host(reinterpret_cast<const ssrlcv_camera*>(&left->camera),
                                               reinterpret_cast<const ssrlcv_camera*>(&right->camera), &rect);
    if (rc != 0) {
      logger.err << "ERROR: this camera pair cannot be rectified: " + std::string(ssrlcv_hip_status_string(rc));
      std::exit(-1);
    }
    if (left->size.x != rect.w || left->size.y != rect.h || right->size.x != rect.w || right->size.y != rect.h) {
      logger.err << "ERROR: the images of a pair to rectify have their cameras' size";
      std::exit(-1);
    }
    GpuRead<unsigned char> leftOnGpu(grey(left)), rightOnGpu(grey(right));
    const unsigned long n = (unsigned long)rect.w * rect.h;
    ptr::value<Unity<unsigned char>> pixelsL(nullptr, n, gpu), pixelsR(nullptr, n, gpu);
    HipSafeCall(ssrlcv_hip_warp_homography_u8(left->pixels->device.get(), rect.w, rect.h, rect.Hl, pixelsL->device.get(), rect.w, rect.h, nullptr));
    HipSafeCall(ssrlcv_hip_warp_homography_u8(right->pixels->device.get(), rect.w, rect.h, rect.Hr, pixelsR->device.get(), rect.w, rect.h, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_device_synchronize());  // the sources may leave the gpu
    leftOut = ptr::value<Image>(uint2{rect.w, rect.h}, 1u, pixelsL);
    rightOut = ptr::value<Image>(uint2{rect.w, rect.h}, 1u, pixelsR);
    leftOut->id = left->id;
    rightOut->id = right->id;
    return rect;
  }

  // in place on generateDisparities' maps of a pair rectify() made: the pixels whose windows (with a census cost: whose
  // footprints, radius + census radius) left a source image become invalid (it only removes pixels); cost may be nullptr
  void maskRectified(ptr::value<Unity<float>> disparity, ptr::value<Unity<unsigned int>> cost, const Rectification& rect) {
    GpuWrite<float> onGpu(disparity);
    GpuWrite<unsigned int> costOnGpu(cost);
    HipSafeCall(ssrlcv_hip_stereo_mask_rectified(disparity->device.get(), cost != nullptr ? cost->device.get() : nullptr, rect.w, rect.h,
                                                 footprintRadius(), rect.Hl, rect.Hr, rect.w, rect.h, nullptr));
    HipCheckError();
  }

  // in place on a map of generateDisparities (include/ssrlcv_hip.h "disparity post-filters" item 3; the map has the size of
  // the last pair this factory matched, or what setMapSize said): the connected components of at most maxSpeckleSize pixels
  // become invalid, two neighbours being connected when their disparities differ by at most maxDiff; cost may be nullptr
  // (it only removes pixels)
  void filterSpeckles(ptr::value<Unity<float>> disparity, ptr::value<Unity<unsigned int>> cost, unsigned int maxSpeckleSize, float maxDiff) {
    const uint32_t w = mapSize.x, h = mapSize.y;
    const size_t wsBytes = ssrlcv_hip_stereo_filter_speckles_workspace_bytes(w, h);
    if ((unsigned long)w * h != disparity->size() || (wsBytes == 0 && disparity->size() != 0)) {
      logger.err << "ERROR: the speckle filter takes a map of the size of the last pair matched (setMapSize for any other)";
      std::exit(-1);
    }
    GpuWrite<float> onGpu(disparity);
    GpuWrite<unsigned int> costOnGpu(cost);
    DeviceScratch workspace(wsBytes);
    HipSafeCall(ssrlcv_hip_stereo_filter_speckles(disparity->device.get(), cost != nullptr ? cost->device.get() : nullptr, w, h, maxDiff,
                                                  maxSpeckleSize, workspace.get(), wsBytes, nullptr));
    HipCheckError();
  }

  // a new map, in state gpu: every valid pixel becomes the lower median of the valid pixels of its (2 radius + 1)^2 window,
  // radius 1 or 2; holes stay holes (item 4).  A cost map goes on describing the winners before the filter.
  ptr::value<Unity<float>> medianFilter(ptr::value<Unity<float>> disparity, unsigned int radius) {
    const uint32_t w = mapSize.x, h = mapSize.y;
    if ((unsigned long)w * h != disparity->size()) {
      logger.err << "ERROR: the median filter takes a map of the size of the last pair matched (setMapSize for any other)";
      std::exit(-1);
    }
    GpuRead<float> onGpu(disparity);
    ptr::value<Unity<float>> filtered(nullptr, disparity->size(), gpu);
    HipSafeCall(ssrlcv_hip_stereo_filter_median(disparity->device.get(), filtered->device.get(), w, h, radius, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_device_synchronize());  // the source may leave the gpu
    return filtered;
  }

  // a new map, in state gpu (include/ssrlcv_hip.h "hole filling"): every hole takes the smallest (rule 0) or the lower median
  // (rule 1) of the first measured pixels within maxGap steps along the directions of the bit mask `paths` (setSemiGlobal's
  // numbering), if at least minHits directions have one; measured pixels pass through.  Only measured pixels are sources, so
  // a second call may fill more.  A cost map is not touched: a filled pixel keeps its UINT32_MAX.  It runs last, behind
  // medianFilter and filterSpeckles; with a rectification, maskRectified once more behind it.
  ptr::value<Unity<float>> fillHoles(ptr::value<Unity<float>> disparity, unsigned int paths, unsigned int maxGap, unsigned int minHits, unsigned int rule) {
    return fillHoles(disparity, paths, maxGap, minHits, rule, nullptr);
  }

  // ... and *filled (if not nullptr) becomes a new map in state gpu: 1 at the holes that got a value, 0 everywhere else
  ptr::value<Unity<float>> fillHoles(ptr::value<Unity<float>> disparity, unsigned int paths, unsigned int maxGap, unsigned int minHits, unsigned int rule,
                                     ptr::value<Unity<unsigned char>>* filled) {
    const uint32_t w = mapSize.x, h = mapSize.y;
    const ssrlcv_fill_params params = {paths, maxGap, minHits, rule};
    if ((unsigned long)w * h != disparity->size()) {
      logger.err << "ERROR: hole filling takes a map of the size of the last pair matched (setMapSize for any other)";
      std::exit(-1);
    }
    const size_t wsBytes = ssrlcv_hip_stereo_fill_holes_workspace_bytes(w, h, &params);  // 0 for refused parameters: the call says so
    GpuRead<float> onGpu(disparity);
    ptr::value<Unity<float>> out(nullptr, disparity->size(), gpu);
    if (filled != nullptr) *filled = ptr::value<Unity<unsigned char>>(nullptr, disparity->size(), gpu);
    DeviceScratch workspace(wsBytes);
    HipSafeCall(ssrlcv_hip_stereo_fill_holes(disparity->device.get(), out->device.get(), filled != nullptr ? (*filled)->device.get() : nullptr, w, h,
                                             &params, workspace.get(), wsBytes, nullptr));
    HipCheckError();
    return out;
  }

  // the triangle mesh of a map over the grid of meshStep, generateMatches' setStep (include/ssrlcv_hip.h "disparity mesh" items 1-3; the map has the size
  // of the last pair matched, or what setMapSize said): both maps in state gpu, the vertices numbered as generateMatches
  // numbers its records for the same map; two nodes whose disparities differ by more than maxJump are not joined
  GridMesh generateMesh(ptr::value<Unity<float>> disparity, unsigned int meshStep, float maxJump) {
    const uint32_t w = mapSize.x, h = mapSize.y;
    const ssrlcv_mesh_params params = {meshStep, maxJump};
    if ((unsigned long)w * h != disparity->size()) {
      logger.err << "ERROR: the mesh takes a map of the size of the last pair matched (setMapSize for any other)";
      std::exit(-1);
    }
    const size_t wsBytes = ssrlcv_hip_disparity_mesh_workspace_bytes(w, h, &params);  // 0 for refused parameters: the call says so
    GpuRead<float> onGpu(disparity);
    GridMesh mesh;
    mesh.gw = meshStep && w ? (w - 1) / meshStep + 1 : 0;
    mesh.gh = meshStep && h ? (h - 1) / meshStep + 1 : 0;
    const unsigned long nodes = (unsigned long)mesh.gw * mesh.gh;
    mesh.vertexIndex = ptr::value<Unity<unsigned int>>(nullptr, nodes ? nodes : 1ul, gpu);
    mesh.cells = ptr::value<Unity<unsigned char>>(nullptr, mesh.numCells() ? mesh.numCells() : 1ul, gpu);
    ptr::device<uint32_t> countDev(1);
    DeviceScratch workspace(wsBytes);
    HipSafeCall(ssrlcv_hip_disparity_mesh(disparity->device.get(), w, h, &params, mesh.vertexIndex->device.get(), mesh.cells->device.get(),
                                          countDev.get(), workspace.get(), wsBytes, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_memcpy(&mesh.vertexCount, countDev.get(), sizeof mesh.vertexCount, 1));
    return mesh;
  }

  // in place: generateMatches' records of a rectified pair, through Hl and Hr into source pixels; a record that does not
  // map back is removed (validateMatches' stable compaction)
  void unrectifyMatches(ptr::value<Unity<Match>> matches, const Rectification& rect) {
    GpuWrite<Match> onGpu(matches);  // on leaving it brings back what the Unity then holds: the kept records
    const uint32_t n = (uint32_t)matches->size();
    HipSafeCall(ssrlcv_hip_matches_apply_homography(reinterpret_cast<ssrlcv_match*>(matches->device.get()), n, rect.Hl, rect.Hr, nullptr));
    HipCheckError();
    const size_t wsBytes = ssrlcv_hip_match_workspace_bytes(n, 1);
    DeviceScratch workspace(wsBytes);
    uint32_t left = 0;
    HipSafeCall(ssrlcv_hip_compact_matches(SSRLCV_OUT_MATCH, matches->device.get(), n, &left, workspace.get(), wsBytes, nullptr));
    if (left == 0) {
      logger.err << "ERROR: no match of the rectified pair maps back into the sources";
      std::exit(0);
    }
    if (left != n) {
      ptr::device<Match> kept((long)left);
      HipSafeCall(ssrlcv_hip_memcpy(kept.get(), matches->device.get(), (size_t)left * sizeof(Match), 2));
      matches->setData(kept, left, gpu);
    }
  }
};

}  // namespace ssrlcv
