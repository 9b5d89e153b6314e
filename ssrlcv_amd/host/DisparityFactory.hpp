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
// Pixels keep upstream's memory-state contract: forced onto the gpu for the call, restored to their origin state after it.
#pragma once
#include "Image.hpp"
#include "MatchFactory.hpp"

namespace ssrlcv {

class DisparityFactory {
  ssrlcv_stereo_params params;
  unsigned int step = 1;

  static void toGpu(ptr::value<Image> image, MemoryState& origin, bool& keepHost) {
    if (image->colorDepth != 1) {
      logger.err << "ERROR: dense stereo takes single-channel images (convertToBW first)";
      std::exit(-1);
    }
    origin = image->pixels->getMemoryState();
    keepHost = origin == cpu;  // the kernels only read the pixels: keep the host copy, drop the device one afterwards
    if (keepHost) image->pixels->transferMemoryTo(gpu);
    else if (origin != gpu) image->pixels->setMemoryState(gpu);
  }
  static void restore(ptr::value<Image> image, MemoryState origin, bool keepHost) {
    if (keepHost) image->pixels->clear(gpu);
    else if (origin != gpu) image->pixels->setMemoryState(origin);
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

  // disparity of every left pixel (row-major, w x h), in state gpu; `cost` (optional out) receives the winners' costs
  ptr::value<Unity<float>> generateDisparities(ptr::value<Image> left, ptr::value<Image> right,
                                               ptr::value<Unity<unsigned int>>* cost = nullptr) {
    if (left->size.x != right->size.x || left->size.y != right->size.y) {
      logger.err << "ERROR: a rectified pair has two images of one size";
      std::exit(-1);
    }
    const uint32_t w = left->size.x, h = left->size.y;
    const size_t wsBytes = ssrlcv_hip_stereo_workspace_bytes(w, h, &params);
    if (wsBytes == 0) {
      logger.err << "ERROR: dense stereo parameters outside the contract (radius 1..15, 1..256 disparities from -32768..32767)";
      std::exit(-1);
    }
    MemoryState originL, originR;
    bool keepL, keepR;
    toGpu(left, originL, keepL);
    toGpu(right, originR, keepR);
    const unsigned long n = (unsigned long)w * h;
    ptr::device<unsigned char> workspace((long)wsBytes);
    ptr::value<Unity<float>> disparity(nullptr, n ? n : 1ul, gpu);
    ptr::value<Unity<unsigned int>> costs;
    if (cost) costs = ptr::value<Unity<unsigned int>>(nullptr, n ? n : 1ul, gpu);
    HipSafeCall(ssrlcv_hip_stereo_sad_u8(left->pixels->device.get(), right->pixels->device.get(), w, h, &params, workspace.get(), wsBytes,
                                         disparity->device.get(), cost ? costs->device.get() : nullptr, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_device_synchronize());  // the workspace goes out of scope
    restore(left, originL, keepL);
    restore(right, originR, keepR);
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
    MemoryState origin = disparity->getMemoryState();
    if (origin != gpu) disparity->setMemoryState(gpu);
    // samples per row and column: ceil(n / step) without the sum n + step - 1, which wraps for a step near 2^32
    const uint32_t cap = (w ? (w - 1) / step + 1 : 0) * (h ? (h - 1) / step + 1 : 0);
    ptr::device<unsigned char> workspace((long)wsBytes);
    ptr::device<Match> staging((long)(cap ? cap : 1));
    ptr::device<uint32_t> countDev(1);
    uint32_t count = 0;
    HipSafeCall(ssrlcv_hip_stereo_matches(disparity->device.get(), w, h, step, left->id, right->id,
                                          reinterpret_cast<ssrlcv_match*>(staging.get()), cap, countDev.get(), workspace.get(), wsBytes, nullptr));
    HipCheckError();
    HipSafeCall(ssrlcv_hip_memcpy(&count, countDev.get(), sizeof count, 1));
    if (origin != gpu) disparity->setMemoryState(origin);
    if (count == 0) {
      logger.err << "ERROR: dense stereo left no valid pixel";
      std::exit(0);
    }
    if (count == cap) return ptr::value<Unity<Match>>(staging, (unsigned long)count, gpu);
    ptr::device<Match> exact((long)count);
    HipSafeCall(ssrlcv_hip_memcpy(exact.get(), staging.get(), (size_t)count * sizeof(Match), 2));
    return ptr::value<Unity<Match>>(exact, (unsigned long)count, gpu);
  }
};

}  // namespace ssrlcv
