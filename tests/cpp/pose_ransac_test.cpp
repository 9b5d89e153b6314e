// tests/cpp/pose_ransac_test.cpp -- PoseEstimator::estimatePoseRANSAC through the reference's class API.
//   pose_ransac_test <pair.bin> [fallback]   (GPU) pair.bin: uint64 n, two ssrlcv_camera records (query, target),
//                                            n ssrlcv_match
// Prints "ransac <inliers at 2 px> <roll pitch yaw x y z>" and "lm <cost at the RANSAC angles> <cost after LM_optimize>"
// (LM_optimize starts from the RANSAC angles and the cameras' baseline), then "ok".  `fallback`: the pair must have no
// valid F, so estimatePoseRANSAC takes its fallback (the cameras' relative pose); prints the "ransac" line, then "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static_assert(sizeof(Image::Camera) == sizeof(ssrlcv_camera), "Camera layout");
static_assert(sizeof(Match) == sizeof(ssrlcv_match), "Match layout");

static float poseCost(const ptr::value<Unity<Match>>& matches, const Pose& pose, const Image& q, const Image& t) {
  matches->transferMemoryTo(gpu);
  ptr::device<float> c(1);
  HipSafeCall(ssrlcv_hip_pose_cost((const ssrlcv_match*)matches->device.get(), (uint32_t)matches->size(),
                                   (const ssrlcv_pose*)&pose, (const ssrlcv_camera*)&q.camera,
                                   (const ssrlcv_camera*)&t.camera, c.get(), nullptr));
  float h = 0;
  HipSafeCall(ssrlcv_hip_memcpy(&h, c.get(), sizeof h, 1));
  matches->setMemoryState(cpu);
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <pair.bin> [fallback]\n", argv[0]); return 2; }
  const bool fallback = argc > 2 && std::string(argv[2]) == "fallback";
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint64_t n = 0;
  ssrlcv_camera cams[2];
  CHECK(std::fread(&n, sizeof n, 1, f) == 1 && std::fread(cams, sizeof cams, 1, f) == 1);
  ptr::value<Unity<Match>> matches(nullptr, (unsigned long)n, cpu);
  CHECK(std::fread(matches->host.get(), sizeof(Match), n, f) == n);
  std::fclose(f);
  ptr::value<Image> images[2];
  for (int i = 0; i < 2; ++i) {
    images[i].construct();
    std::memcpy((void*)&images[i]->camera, &cams[i], sizeof(ssrlcv_camera));  // same 80-byte layout
    images[i]->id = i;
    images[i]->size = images[i]->camera.size;
  }
  PoseEstimator estim(images[0], images[1], matches);
  const FMatrixInliers fm = estim.estimateFMatrixRANSAC(4096, 2.0f);
  CHECK(fm.valid != fallback && matches->getMemoryState() == cpu);
  Pose pose = estim.estimatePoseRANSAC();
  CHECK(matches->getMemoryState() == cpu);  // origin state restored
  CHECK(std::isfinite(pose.roll) && std::isfinite(pose.pitch) && std::isfinite(pose.yaw) && std::isfinite(pose.x));
  std::printf("ransac %lu %.9g %.9g %.9g %.9g %.9g %.9g\n", fm.inliers, pose.roll, pose.pitch, pose.yaw, pose.x, pose.y,
              pose.z);
  if (fallback) {
    std::printf("ok\n");
    return 0;
  }
  Pose start = pose;
  const float3 b = estim.baselineInQueryFrame();
  start.x = b.x / 1000;
  start.y = b.y / 1000;
  start.z = b.z / 1000;
  const float before = poseCost(matches, start, *images[0], *images[1]);
  Pose refined = pose;
  estim.LM_optimize(&refined);
  const float after = poseCost(matches, refined, *images[0], *images[1]);
  std::printf("lm %.9g %.9g\n", before, after);
  CHECK(std::isfinite(after));
  std::printf("ok\n");
  return 0;
}
