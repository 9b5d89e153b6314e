// ssrlcv_amd/host/PoseEstimator.hpp -- ssrlcv::PoseEstimator's Levenberg-Marquardt refinement of the relative pose
// (include/PoseEstimator.cuh:30-61, src/PoseEstimator.cu:314-515) over the fused HIP terms kernel
// (ssrlcv_hip_pose_lm_terms / ssrlcv_hip_pose_cost), and estimatePoseRANSAC (:92-312) over the device 7-point F-matrix
// RANSAC (ssrlcv_hip_fmatrix_ransac, conventions in include/ssrlcv_hip.h; PARITY UNPINNED) and the E decomposition with
// its cheirality vote (ssrlcv_hip_pose_from_fmatrix).  The reference's own stage flow has the RANSAC commented out
// (src/Pipeline.cu:101) and starts LM from the cameras' relative pose; doPoseEstimation here does the same.
//
// LM_iteration follows upstream step for step: terms at the current pose; then up to 20 trial steps with
// JTJ + lambda I, pseudo-inverse with singular values <= 1e-4 dropped (cusolverDnSgesvd upstream, pseudoInverse()
// here: PARITY UNPINNED), delta = -JTJ^+ JTf, trial cost, lambda doubled per trial; on success lambda /= 4.
#pragma once
#include <cstdio>
#include "Image.hpp"
#include "MatchFactory.hpp"
#include "Scoped.hpp"
#include "matrix_util.hpp"

namespace ssrlcv {

struct FMatrixInliers {
  float fmatrix[3][3];
  unsigned long inliers;
  bool valid;
};

struct Pose {
  float roll;   // x-rotation, in radians
  float pitch;  // y-rotation, in radians
  float yaw;    // z-rotation, in radians
  float x;      // x-position, kilometers
  float y;      // y-position, kilometers
  float z;      // z-position, kilometers
};
static_assert(sizeof(Pose) == sizeof(ssrlcv_pose), "Pose layout");

namespace stage {
// Pose of camera `b` seen from camera `a`: position = (a - b) turned back through a's z, y, x rotations, angles = the
// axis rotations of Ra^T Rb (the starting point the reference hands to its LM refinement, src/Pipeline.cu:103-119).
inline Pose relativePose(const Image::Camera& a, const Image::Camera& b) {
  float3 t = a.cam_pos - b.cam_pos;
  const float3 axes[3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
  const float turn[3] = {-a.cam_rot.z, -a.cam_rot.y, -a.cam_rot.x};
  for (int k = 0; k < 3; ++k) t = rotatePointArbitrary(t, axes[k], turn[k]);
  float Ra[3][3], RaT[3][3], Rb[3][3], Rab[3][3];
  getRotationMatrix(a.cam_rot, Ra);
  transpose(Ra, RaT);
  getRotationMatrix(b.cam_rot, Rb);
  multiply(RaT, Rb, Rab);
  const float3 angles = getAxisRotations(Rab);
  Pose p;
  p.roll = angles.x;
  p.pitch = angles.y;
  p.yaw = angles.z;
  p.x = t.x;
  p.y = t.y;
  p.z = t.z;
  return p;
}
}  // namespace stage

class PoseEstimator {
 private:
  ptr::value<Unity<Match>> matches;  // keypoints should be (query, target)
  ptr::value<Image> query;
  ptr::value<Image> target;

  float cost(const Pose& pose) {
    ptr::device<float> c(1);
    HipSafeCall(ssrlcv_hip_pose_cost((const ssrlcv_match*)matches->device.get(), (uint32_t)matches->size(),
                                     (const ssrlcv_pose*)&pose, (const ssrlcv_camera*)&query->camera,
                                     (const ssrlcv_camera*)&target->camera, c.get(), nullptr));
    float h = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&h, c.get(), sizeof(float), 1));
    return h;
  }

  // the RANSAC call behind both public methods; mask / F (device) receive the inlier mask and F when not null
  FMatrixInliers fmatrixRANSAC(unsigned samples, float threshold, uint64_t seed, ptr::device<unsigned char>* mask,
                               ptr::device<float>* Fdev = nullptr) {
    GpuRead<Match> onGpu(matches);
    const uint32_t n = (uint32_t)matches->size();
    ptr::device<float> Fown(9);
    ptr::device<uint32_t> count(1);
    DeviceScratch ws(ssrlcv_hip_fmatrix_ransac_workspace_bytes(n, samples));
    float* Fd = Fdev ? Fdev->get() : Fown.get();
    HipSafeCall(ssrlcv_hip_fmatrix_ransac((const ssrlcv_match*)matches->device.get(), n, samples, threshold, seed, ws.get(),
                                          ws.bytes(), Fd, count.get(),
                                          mask ? mask->get() : nullptr, nullptr, nullptr, nullptr));
    FMatrixInliers out;
    uint32_t c = 0;
    HipSafeCall(ssrlcv_hip_memcpy(&out.fmatrix[0][0], Fd, 9 * sizeof(float), 1));
    HipSafeCall(ssrlcv_hip_memcpy(&c, count.get(), sizeof c, 1));
    out.inliers = c;
    out.valid = c >= 7;
    return out;
  }

 public:
  // Sets up pose estimator to adjust target image
  PoseEstimator(ptr::value<Image> query, ptr::value<Image> target, ptr::value<Unity<Match>> matches)
      : matches(matches), query(query), target(target) {}

  // 7-point F-matrix RANSAC over `samples` fixed samples (sample hash seeded by `seed`), inlier = Sampson distance below
  // `threshold` px, one least-squares refit; fmatrix row-major in pixels, unit norm.  valid = at least 7 inliers.
  FMatrixInliers estimateFMatrixRANSAC(unsigned samples = 4096, float threshold = 1.0f, uint64_t seed = 0) {
    return fmatrixRANSAC(samples, threshold, seed, nullptr);
  }

  // estimateFMatrixRANSAC with its defaults, then the relative pose of E = K_t^T F K_q (the cheirality vote on its
  // inliers), in LM_optimize's convention.  Without a valid F: an error in the log and the cameras' own relative pose.
  Pose estimatePoseRANSAC() {
    GpuRead<Match> onGpu(matches);
    const unsigned long n = matches->size();
    ptr::device<unsigned char> mask(n ? n : 1);
    ptr::device<float> F(9);
    FMatrixInliers fm = fmatrixRANSAC(4096, 1.0f, 0, &mask, &F);
    Pose pose;
    if (fm.valid) {
      DeviceScratch aux(SSRLCV_FMATRIX_AUX_WORKSPACE_BYTES);
      HipSafeCall(ssrlcv_hip_pose_from_fmatrix((const ssrlcv_match*)matches->device.get(), (uint32_t)n, mask.get(), F.get(),
                                               (const ssrlcv_camera*)&query->camera, (const ssrlcv_camera*)&target->camera,
                                               aux.get(), aux.bytes(), (ssrlcv_pose*)&pose, nullptr));
    } else {
      logger.err.printf("PoseEstimator::estimatePoseRANSAC: no valid F-matrix (%lu inliers); using the cameras' relative pose",
                        fm.inliers);
      pose = stage::relativePose(query->camera, target->camera);
      const float3 b = baselineInQueryFrame();
      pose.x = b.x / 1000;
      pose.y = b.y / 1000;
      pose.z = b.z / 1000;
    }
    return pose;
  }

  // PoseEstimator::LM_optimize (src/PoseEstimator.cu:314-341): the start position is the baseline between the two cameras
  // expressed in the query camera's frame (its z, y, x rotations undone in that order), in the matcher's length unit
  // (1 / 1000 of the cameras'); then at most kMaxLMIterations damped steps, stopping at the first one that does not
  // improve the cost.  The damping starts at 100, as upstream.
  static constexpr int kMaxLMIterations = 50;
  float3 baselineInQueryFrame() const {
    const float3 axis[3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
    const float angle[3] = {query->camera.cam_rot.z, query->camera.cam_rot.y, query->camera.cam_rot.x};
    float3 b = target->camera.cam_pos - query->camera.cam_pos;
    for (int k = 0; k < 3; ++k) b = rotatePointArbitrary(b, axis[k], -angle[k]);
    return b;
  }
  void LM_optimize(Pose* pose) {
    const float3 start = baselineInQueryFrame();
    pose->x = start.x / 1000;
    pose->y = start.y / 1000;
    pose->z = start.z / 1000;
    float damping = 100;
    for (int step = 1; step <= kMaxLMIterations; ++step) {
      logger.info.printf("Pose rotations: %f %f %f", pose->roll, pose->pitch, pose->yaw);
      logger.info.printf("Pose positions: %f %f %f", pose->x, pose->y, pose->z);
      if (!LM_iteration(pose, &damping)) break;
    }
  }

  // public here (private upstream) so that tests can drive single iterations
  bool LM_iteration(Pose* pose, float* lambda) {
    GpuRead<Match> onGpu(matches);
    ptr::device<float> terms(43);
    HipSafeCall(ssrlcv_hip_pose_lm_terms((const ssrlcv_match*)matches->device.get(), (uint32_t)matches->size(),
                                         (const ssrlcv_pose*)pose, (const ssrlcv_camera*)&query->camera,
                                         (const ssrlcv_camera*)&target->camera, terms.get(), nullptr));
    float h[43];
    HipSafeCall(ssrlcv_hip_memcpy(h, terms.get(), sizeof h, 1));
    float* JTJ = h;
    const float* JTf = h + 36;
    const float startCost = h[42];
    logger.info.printf("Starting cost: %f", startCost);
    float newCost = startCost + 100;  // just to make sure it starts off greater
    float old_lambda = 0;
    Pose newPose = *pose;
    int num_iterations = 0;
    bool ok = true;
    while (startCost <= newCost) {
      if (num_iterations >= 20) { ok = false; break; }
      num_iterations += 1;
      for (int i = 0; i < 6; i++) JTJ[i + 6 * i] += (*lambda - old_lambda);
      std::vector<float> JTJ_inv = pseudoInverse(JTJ, 6, 1e-4);
      float delta[6];
      for (int i = 0; i < 6; i++) {
        delta[i] = 0;
        for (int j = 0; j < 6; j++) delta[i] += -JTJ_inv[i * 6 + j] * JTf[j];
      }
      newPose.roll = pose->roll + delta[0];
      newPose.pitch = pose->pitch + delta[1];
      newPose.yaw = pose->yaw + delta[2];
      newPose.x = pose->x + delta[3];
      newPose.y = pose->y + delta[4];
      newPose.z = pose->z + delta[5];
      newCost = cost(newPose);
      logger.info.printf("New cost: %f", newCost);
      old_lambda = *lambda;
      *lambda *= 2;
    }
    if (ok) {
      *lambda /= 4;  // the loop's last doubling plus one real halving
      *pose = newPose;
    }
    return ok;
  }
};

}  // namespace ssrlcv
