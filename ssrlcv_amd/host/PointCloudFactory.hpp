// ssrlcv_amd/host/PointCloudFactory.hpp -- PointCloudFactory with the reference's signatures
// (include/PointCloudFactory.cuh:25-48,93-255), bound to the HIP C ABI: generateBundles, the two-view / N-view
// triangulators and BundleAdjustTwoView.  Memory-state side effects follow upstream: generateBundles leaves the match
// set on the cpu (src/PointCloudFactory.cu:909-914), triangulators return the cloud on the cpu and drop the gpu copies
// of lines/bundles (:286-290).  linearCutoffFilter / deterministicStatisticalFilter (section 8f item 1) and stereo_disparity
// (the cloud of DisparityFactory.hpp's matches) are provided; plane fitting, debug dumps and cloud scale/rotate helpers are
// out of scope.
//
// BundleAdjustTwoView keeps upstream's control flow (:1832-2262) but evaluates all 24 + 588 finite-difference points
// of calculateImageGradient / calculateImageHessian (:1059-1504) in ONE fused launch (ssrlcv_hip_ba_sweep2) instead of
// 612 x (H2D + 2 kernels + D2H).  The 12x12 pseudo-inverse (cusolverDnSgesvd + 2 cublasSgemm upstream, :1511-1824) is a
// host one-sided Jacobi SVD here; PARITY UNPINNED for that step (no reference fixture reaches it: upstream's update is
// never applied because fixed_camera is true, :2150).
#pragma once
#include <cmath>
#include <vector>
#include "Image.hpp"
#include "MatchFactory.hpp"
#include "Scoped.hpp"
#include "matrix_util.hpp"

namespace ssrlcv {

struct Bundle {
  struct Line { float3 vec; float3 pnt; };
  unsigned int numLines;
  int index;
  bool invalid;
};
struct BundleSet {
  ptr::value<Unity<Bundle::Line>> lines;
  ptr::value<Unity<Bundle>> bundles;
};
static_assert(sizeof(Bundle) == sizeof(ssrlcv_bundle) && sizeof(Bundle::Line) == sizeof(ssrlcv_line), "Bundle layouts");

class PointCloudFactory {
 private:
  struct DevFloat {  // one float on the device, zero-initialised (upstream's d_linearError)
    ptr::device<float> p;
    DevFloat() : p(1) { HipSafeCall(ssrlcv_hip_memset(p.get(), 0, sizeof(float))); }
    float get() { float v; HipSafeCall(ssrlcv_hip_memcpy(&v, p.get(), sizeof v, 1)); return v; }
  };

  ptr::value<Unity<float3>> triangulate(bool nview, BundleSet bundleSet, ptr::value<Unity<float>> errors, float* errSum,
                                        float* cutoff, bool wantPoints) {
    // no guards: upstream's end state is not the entry state -- lines, bundles, errors and the cloud all end on the cpu
    bundleSet.lines->transferMemoryTo(gpu);
    bundleSet.bundles->transferMemoryTo(gpu);
    uint32_t n = (uint32_t)bundleSet.bundles->size();
    if (errors != nullptr) errors->transferMemoryTo(gpu);
    ptr::value<Unity<float3>> pointcloud;
    if (wantPoints) pointcloud = ptr::value<Unity<float3>>(nullptr, (unsigned long)n, gpu);
    DevFloat sum;
    ptr::device<float> cut_d;
    if (cutoff) {
      cut_d.set(1);
      HipSafeCall(ssrlcv_hip_memcpy(cut_d.get(), cutoff, sizeof(float), 0));
    }
    auto* lines = reinterpret_cast<const ssrlcv_line*>(bundleSet.lines->device.get());
    auto* bundles = reinterpret_cast<ssrlcv_bundle*>(bundleSet.bundles->device.get());
    auto* pts = wantPoints ? reinterpret_cast<ssrlcv_float3*>(pointcloud->device.get()) : nullptr;
    float* errs = errors != nullptr ? errors->device.get() : nullptr;
    if (nview) HipSafeCall(ssrlcv_hip_triangulateN(lines, bundles, n, pts, errs, cut_d.get(), errSum ? sum.p.get() : nullptr, errSum ? 0 : 1, nullptr));
    else HipSafeCall(ssrlcv_hip_triangulate2(lines, bundles, n, pts, errs, cut_d.get(), errSum ? sum.p.get() : nullptr, nullptr));
    HipCheckError();
    if (wantPoints) {
      pointcloud->transferMemoryTo(cpu);
      pointcloud->clear(gpu);
    }
    if (errors != nullptr) {
      errors->setFore(gpu);
      errors->transferMemoryTo(cpu);
      errors->clear(gpu);
    }
    if (cutoff) {  // cutoff variants write bundles[].invalid: bring it back before dropping the gpu copy
      bundleSet.bundles->setFore(gpu);
      bundleSet.bundles->transferMemoryTo(cpu);
    }
    bundleSet.lines->clear(gpu);
    bundleSet.bundles->clear(gpu);
    if (errSum) *errSum = sum.get();
    return pointcloud;
  }

  static void cameras_of(std::vector<ptr::value<Image>>& images, std::vector<ssrlcv_camera>& out) {
    out.resize(images.size());
    for (size_t i = 0; i < images.size(); ++i) std::memcpy(&out[i], &images[i]->camera, sizeof(ssrlcv_camera));
  }

 public:
  PointCloudFactory() {}

  // src/PointCloudFactory.cu:832-925
  BundleSet generateBundles(MatchSet* matchSet, std::vector<ptr::value<Image>> images) {
    ptr::value<Unity<Bundle>> bundles(nullptr, matchSet->matches->size(), gpu);
    ptr::value<Unity<Bundle::Line>> lines(nullptr, matchSet->keyPoints->size(), gpu);
    // no guards: upstream leaves the match set on the cpu whatever state it came in
    matchSet->matches->transferMemoryTo(gpu);
    matchSet->keyPoints->transferMemoryTo(gpu);
    uint32_t nb = (uint32_t)bundles->size();
    auto* mm = reinterpret_cast<const ssrlcv_multimatch*>(matchSet->matches->device.get());
    auto* kp = reinterpret_cast<const ssrlcv_keypoint*>(matchSet->keyPoints->device.get());
    if (!images.at(0)->isPushbroom) {
      logger.info << "\t Generating standard projective bundles ... ";
      std::vector<ssrlcv_camera> cams;
      cameras_of(images, cams);
      ptr::device<ssrlcv_camera> cams_d((long)cams.size());
      HipSafeCall(ssrlcv_hip_memcpy(cams_d.get(), cams.data(), cams.size() * sizeof(ssrlcv_camera), 0));
      HipSafeCall(ssrlcv_hip_generate_bundles(mm, kp, nb, cams_d.get(), (uint32_t)cams.size(),
                                              reinterpret_cast<ssrlcv_bundle*>(bundles->device.get()),
                                              reinterpret_cast<ssrlcv_line*>(lines->device.get()), nullptr));
      HipCheckError();
    } else {
      logger.info << "\t Generating special pushbroom bundles ... ";
      std::vector<ssrlcv_pushbroom> pbs(images.size());
      for (size_t i = 0; i < images.size(); ++i) std::memcpy(&pbs[i], &images[i]->pushbroom, sizeof(ssrlcv_pushbroom));
      ptr::device<ssrlcv_pushbroom> pbs_d((long)pbs.size());
      HipSafeCall(ssrlcv_hip_memcpy(pbs_d.get(), pbs.data(), pbs.size() * sizeof(ssrlcv_pushbroom), 0));
      HipSafeCall(ssrlcv_hip_generate_pushbroom_bundles(mm, kp, nb, pbs_d.get(), (uint32_t)pbs.size(),
                                                        reinterpret_cast<ssrlcv_bundle*>(bundles->device.get()),
                                                        reinterpret_cast<ssrlcv_line*>(lines->device.get()), nullptr));
      HipCheckError();
    }
    matchSet->matches->setFore(gpu);
    matchSet->keyPoints->setFore(gpu);
    matchSet->matches->transferMemoryTo(cpu);
    matchSet->keyPoints->transferMemoryTo(cpu);
    matchSet->matches->clear(gpu);
    matchSet->keyPoints->clear(gpu);
    bundles->transferMemoryTo(cpu);
    bundles->clear(gpu);
    lines->transferMemoryTo(cpu);
    lines->clear(gpu);
    return {lines, bundles};
  }
  // :934-1051 -- the Image objects are shared with the caller and stay modified, exactly like upstream (its `temp`
  // backup holds the same shared pointers, so the "restore" is a no-op)
  BundleSet generateBundles(MatchSet* matchSet, std::vector<ptr::value<Image>> images, ptr::value<Unity<float>> params) {
    int per = (int)(params->size() / images.size());
    ptr::value<Unity<float>> tmp(nullptr, (unsigned long)per, cpu);
    for (size_t i = 0; i < images.size(); ++i) {
      for (int j = 0; j < per; ++j) tmp->host.get()[j] = params->host.get()[i * per + j];
      images[i]->setFloatVector(tmp);
    }
    return generateBundles(matchSet, images);
  }

  // stereo_disparity: the cloud of a rectified pair's matches, Z = foc baseline / (d + doffset) with d = kp0.x - kp1.x,
  // X = (kp0.x - center.x) Z / foc, Y likewise (ssrlcv_hip_stereo_points); the four-argument form measures from the pixel
  // origin.  Like the triangulators the cloud comes back on the cpu; the matches are restored to their origin state.
  ptr::value<Unity<float3>> stereo_disparity(ptr::value<Unity<Match>> matches, float foc, float baseline, float doffset, float2 center) {
    GpuRead<Match> onGpu(matches);
    const uint32_t n = (uint32_t)matches->size();
    ptr::value<Unity<float3>> pointcloud(nullptr, (unsigned long)n, gpu);
    HipSafeCall(ssrlcv_hip_stereo_points(reinterpret_cast<const ssrlcv_match*>(matches->device.get()), n, foc, baseline, doffset, center.x,
                                         center.y, reinterpret_cast<ssrlcv_float3*>(pointcloud->device.get()), nullptr));
    HipCheckError();
    pointcloud->transferMemoryTo(cpu);
    pointcloud->clear(gpu);
    return pointcloud;
  }
  ptr::value<Unity<float3>> stereo_disparity(ptr::value<Unity<Match>> matches, float foc, float baseline, float doffset) {
    return stereo_disparity(matches, foc, baseline, doffset, float2{0.0f, 0.0f});
  }

  // src/PointCloudFactory.cu:228-556
  ptr::value<Unity<float3>> twoViewTriangulate(BundleSet bundleSet) { return triangulate(false, bundleSet, nullptr, nullptr, nullptr, true); }
  ptr::value<Unity<float3>> twoViewTriangulate(BundleSet bundleSet, float* linearError) {
    *linearError = 0;
    return triangulate(false, bundleSet, nullptr, linearError, nullptr, true);
  }
  ptr::value<Unity<float3>> twoViewTriangulate(BundleSet bundleSet, ptr::value<Unity<float>> errors, float* linearError) {
    *linearError = 0;
    return triangulate(false, bundleSet, errors, linearError, nullptr, true);
  }
  ptr::value<Unity<float3>> twoViewTriangulate(BundleSet bundleSet, ptr::value<Unity<float>> errors, float* linearError, float* linearErrorCutoff) {
    *linearError = 0;
    return triangulate(false, bundleSet, errors, linearError, linearErrorCutoff, true);
  }
  void voidTwoViewTriangulate(BundleSet bundleSet, float* linearError) {
    *linearError = 0;
    triangulate(false, bundleSet, nullptr, linearError, nullptr, false);
  }
  void voidTwoViewTriangulate(BundleSet bundleSet, float* linearError, float* linearErrorCutoff) {
    *linearError = 0;
    triangulate(false, bundleSet, nullptr, linearError, linearErrorCutoff, false);
  }
  // :568-818
  ptr::value<Unity<float3>> nViewTriangulate(BundleSet bundleSet) { return triangulate(true, bundleSet, nullptr, nullptr, nullptr, true); }
  ptr::value<Unity<float3>> nViewTriangulate(BundleSet bundleSet, float* angularError) {
    *angularError = 0;
    return triangulate(true, bundleSet, nullptr, angularError, nullptr, true);
  }
  ptr::value<Unity<float3>> nViewTriangulate(BundleSet bundleSet, ptr::value<Unity<float>> errors, float* angularError) {
    *angularError = 0;
    return triangulate(true, bundleSet, errors, angularError, nullptr, true);
  }
  ptr::value<Unity<float3>> nViewTriangulate(BundleSet bundleSet, ptr::value<Unity<float>> errors, float* angularError, float* angularErrorCutoff) {
    *angularError = 0;
    return triangulate(true, bundleSet, errors, angularError, angularErrorCutoff, true);
  }

  // ---- filters between triangulation and BA (src/Pipeline.cu:297-352) ----------------
  // Round 4: on the device.  Upstream copies bundles and errors to the host, loops over them there and builds a new
  // MatchSet on the host; here bundles, the error triangulation, the statistical cutoff (ssrlcv_hip_error_sample_cutoff:
  // the host's sequential float sums), the cutoff triangulation and the rebuild (ssrlcv_hip_filter_matchset) are queued
  // back to back and two counts come back.  Results and the MatchSet's final memory state (cpu) are upstream's.
 private:
  // kind 0: linearCutoffFilter(cutoff); kind 1: deterministicStatisticalFilter(sigma, sampleJump)
  void filterOnDevice(MatchSet* matchSet, std::vector<ptr::value<Image>>& images, int kind, float cutoff, float sigma, int sampleJump) {
    const bool twoView = images.size() == 2;
    const uint32_t nb = (uint32_t)matchSet->matches->size(), nk = (uint32_t)matchSet->keyPoints->size();
    // no guards: the match set ends on the cpu, as upstream's generateBundles leaves it
    matchSet->matches->transferMemoryTo(gpu);
    matchSet->keyPoints->transferMemoryTo(gpu);
    auto* mm = reinterpret_cast<const ssrlcv_multimatch*>(matchSet->matches->device.get());
    auto* kp = reinterpret_cast<const ssrlcv_keypoint*>(matchSet->keyPoints->device.get());
    ptr::device<ssrlcv_bundle> bundles((long)nb);
    ptr::device<ssrlcv_line> lines((long)nk);
    if (!images.at(0)->isPushbroom) {
      std::vector<ssrlcv_camera> cams;
      cameras_of(images, cams);
      ptr::device<ssrlcv_camera> cams_d((long)cams.size());
      HipSafeCall(ssrlcv_hip_memcpy(cams_d.get(), cams.data(), cams.size() * sizeof(ssrlcv_camera), 0));
      HipSafeCall(ssrlcv_hip_generate_bundles(mm, kp, nb, cams_d.get(), (uint32_t)cams.size(), bundles.get(), lines.get(), nullptr));
      HipSafeCall(ssrlcv_hip_device_synchronize());  // cams_d is freed at the end of this block
    } else {
      std::vector<ssrlcv_pushbroom> pbs(images.size());
      for (size_t i = 0; i < images.size(); ++i) std::memcpy(&pbs[i], &images[i]->pushbroom, sizeof(ssrlcv_pushbroom));
      ptr::device<ssrlcv_pushbroom> pbs_d((long)pbs.size());
      HipSafeCall(ssrlcv_hip_memcpy(pbs_d.get(), pbs.data(), pbs.size() * sizeof(ssrlcv_pushbroom), 0));
      HipSafeCall(ssrlcv_hip_generate_pushbroom_bundles(mm, kp, nb, pbs_d.get(), (uint32_t)pbs.size(), bundles.get(), lines.get(), nullptr));
      HipSafeCall(ssrlcv_hip_device_synchronize());
    }
    ptr::device<float> errors((long)nb), cut_d(1);
    DevFloat sum;
    auto tri = [&](const float* cut) {
      if (twoView) HipSafeCall(ssrlcv_hip_triangulate2(lines.get(), bundles.get(), nb, nullptr, errors.get(), cut, sum.p.get(), nullptr));
      else HipSafeCall(ssrlcv_hip_triangulateN(lines.get(), bundles.get(), nb, nullptr, errors.get(), cut, sum.p.get(), 0, nullptr));
    };
    if (kind == 0) {
      HipSafeCall(ssrlcv_hip_memcpy(cut_d.get(), &cutoff, sizeof(float), 0));
      tri(cut_d.get());
    } else {
      const float zero = 0.0f;  // the initial triangulation runs its cutoff overload with a cutoff of 0 (:3110-3118)
      HipSafeCall(ssrlcv_hip_memcpy(cut_d.get(), &zero, sizeof(float), 0));
      tri(cut_d.get());
      HipSafeCall(ssrlcv_hip_error_sample_cutoff(errors.get(), nb, (uint32_t)sampleJump, sigma, cut_d.get(), nullptr));
      tri(cut_d.get());
    }
    ptr::value<Unity<MultiMatch>> mmOut(nullptr, (unsigned long)nb, gpu);
    ptr::value<Unity<KeyPoint>> kpOut(nullptr, (unsigned long)nk, gpu);
    ptr::device<uint32_t> counts_d(3);
    DeviceScratch ws(ssrlcv_hip_filter_workspace_bytes(nb));
    HipSafeCall(ssrlcv_hip_filter_matchset(bundles.get(), kp, nb, reinterpret_cast<ssrlcv_multimatch*>(mmOut->device.get()),
                                           reinterpret_cast<ssrlcv_keypoint*>(kpOut->device.get()), counts_d.get(), ws.get(), ws.bytes(), nullptr));
    uint32_t counts[3] = {0, 0, 0};
    HipSafeCall(ssrlcv_hip_memcpy(counts, counts_d.get(), sizeof counts, 1));
    HipCheckError();
    // upstream's generateBundles leaves the MatchSet on the host
    matchSet->matches->transferMemoryTo(cpu);
    matchSet->keyPoints->transferMemoryTo(cpu);
    matchSet->matches->clear(gpu);
    matchSet->keyPoints->clear(gpu);
    const uint32_t kept = counts[0], keptKp = counts[1];
    const bool returnIfNoneBad = kind == 0 || !twoView;  // :3236-3239 and :3543; the two-view statistical form rebuilds regardless
    if (returnIfNoneBad && kept == nb) return;
    if (kept == 0 || (!twoView && keptKp == 0)) return;   // "filtering is too aggressive, all points would be removed"
    ptr::value<Unity<MultiMatch>> newMm(nullptr, (unsigned long)kept, gpu);
    ptr::value<Unity<KeyPoint>> newKp(nullptr, (unsigned long)keptKp, gpu);
    HipSafeCall(ssrlcv_hip_memcpy(newMm->device.get(), mmOut->device.get(), sizeof(MultiMatch) * kept, 2));
    HipSafeCall(ssrlcv_hip_memcpy(newKp->device.get(), kpOut->device.get(), sizeof(KeyPoint) * keptKp, 2));
    newMm->transferMemoryTo(cpu);
    newMm->clear(gpu);
    newKp->transferMemoryTo(cpu);
    newKp->clear(gpu);
    matchSet->matches = newMm;
    matchSet->keyPoints = newKp;
  }

 public:
  // src/PointCloudFactory.cu:3500-3644
  void linearCutoffFilter(MatchSet* matchSet, std::vector<ptr::value<Image>> images, float cutoff) {
    if (cutoff < 0.0) return;
    filterOnDevice(matchSet, images, 0, cutoff, 0.0f, 1);
  }
  // src/PointCloudFactory.cu:3070-3275: cutoff = sigma * stddev of every (1/sampleSize)-th error (mean NOT added)
  void deterministicStatisticalFilter(MatchSet* matchSet, std::vector<ptr::value<Image>> images, float sigma, float sampleSize) {
    if (sampleSize > 1.0 || sampleSize < 0.0) return;
    filterOnDevice(matchSet, images, 1, 0.0f, sigma, (int)(1 / sampleSize));
  }

  // f(cameras) for K parameter sets in one launch; params_host = K x (6 * images) floats
  std::vector<float> evaluateCameraSets(MatchSet* matchSet, std::vector<ptr::value<Image>> images, const std::vector<float>& params_host, uint32_t K) {
    // no guards: the match set ends on the cpu, like generateBundles' (it comes in on the cpu from there)
    matchSet->matches->transferMemoryTo(gpu);
    matchSet->keyPoints->transferMemoryTo(gpu);
    std::vector<ssrlcv_camera> cams;
    cameras_of(images, cams);
    ptr::device<ssrlcv_camera> cams_d((long)cams.size());
    HipSafeCall(ssrlcv_hip_memcpy(cams_d.get(), cams.data(), cams.size() * sizeof(ssrlcv_camera), 0));
    ptr::device<float> params_d((long)params_host.size());
    HipSafeCall(ssrlcv_hip_memcpy(params_d.get(), params_host.data(), params_host.size() * sizeof(float), 0));
    ptr::device<float> sums_d((long)K);
    HipSafeCall(ssrlcv_hip_ba_sweep2(reinterpret_cast<const ssrlcv_multimatch*>(matchSet->matches->device.get()),
                                     reinterpret_cast<const ssrlcv_keypoint*>(matchSet->keyPoints->device.get()),
                                     (uint32_t)matchSet->matches->size(), cams_d.get(), (uint32_t)cams.size(),
                                     params_d.get(), K, sums_d.get(), nullptr, 0, nullptr));
    HipCheckError();
    std::vector<float> sums(K);
    HipSafeCall(ssrlcv_hip_memcpy(sums.data(), sums_d.get(), K * sizeof(float), 1));
    matchSet->matches->clear(gpu);
    matchSet->keyPoints->clear(gpu);
    return sums;
  }

  // calculateImageGradient (:1059-1248).  Upstream's `temp` aliases `images`, so its "reset for backwards" is a
  // self-assignment: the two evaluation points are p+h and (p+h)-h, and the parameter keeps the float drift.  Kept.
  void calculateImageGradient(MatchSet* matchSet, std::vector<ptr::value<Image>> images, ptr::value<Unity<float>> g) {
    const float h_linear = 0.00001, h_radial = 0.00001;
    const size_t V = images.size();
    std::vector<float> cur(6 * V);
    for (size_t j = 0; j < V; ++j) {
      auto p = images[j]->getFloatVector(6);
      for (int k = 0; k < 6; ++k) cur[6 * j + k] = p->host.get()[k];
    }
    std::vector<float> sets;
    sets.reserve(2 * 6 * V * 6 * V);
    for (int k = 0; k < 6; ++k) {      // parameter-major, then image: the order of the upstream loops
      float h = k < 3 ? h_linear : h_radial;
      for (size_t j = 0; j < V; ++j) {
        cur[6 * j + k] += h;
        sets.insert(sets.end(), cur.begin(), cur.end());
        cur[6 * j + k] -= h;
        sets.insert(sets.end(), cur.begin(), cur.end());
      }
    }
    std::vector<float> f = evaluateCameraSets(matchSet, images, sets, (uint32_t)(2 * 6 * V));
    size_t e = 0;
    for (int k = 0; k < 6; ++k) {
      float h = k < 3 ? h_linear : h_radial;
      for (size_t j = 0; j < V; ++j) {
        float forward = f[e++], backwards = f[e++];
        g->host.get()[6 * j + k] = (forward - backwards) / (2 * h);
      }
    }
    // the drifted parameters stay in the images, as upstream leaves them
    ptr::value<Unity<float>> tmp(nullptr, 6, cpu);
    for (size_t j = 0; j < V; ++j) {
      for (int k = 0; k < 6; ++k) tmp->host.get()[k] = cur[6 * j + k];
      images[j]->setFloatVector(tmp);
    }
  }

  // calculateImageHessian (:1256-1504): 5-point diagonal, 4-point cross stencils
  void calculateImageHessian(MatchSet* matchSet, std::vector<ptr::value<Image>> images, ptr::value<Unity<float>> hOut) {
    const float h_step[6] = {0.0001, 0.0001, 0.0001, 0.00001, 0.00001, 0.00001};
    const size_t V = images.size(), N = 6 * V;
    std::vector<float> reset(N);
    for (size_t j = 0; j < V; ++j) {
      auto p = images[j]->getFloatVector(6);
      for (int k = 0; k < 6; ++k) reset[6 * j + k] = p->host.get()[k];
    }
    std::vector<float> sets;
    auto push = [&](size_t i, float di, size_t j, float dj, bool pair) {
      std::vector<float> p = reset;
      p[i] += di;
      if (pair) p[j] += dj;
      sets.insert(sets.end(), p.begin(), p.end());
    };
    for (size_t i = 0; i < N; ++i)
      for (size_t j = 0; j < N; ++j) {
        float hi = h_step[i % 6], hj = h_step[j % 6];
        if (i == j) {
          push(i, (float)(2.0 * hi), 0, 0, false);
          push(i, hi, 0, 0, false);
          push(i, 0.0f, 0, 0, false);
          push(i, -hi, 0, 0, false);
          push(i, (float)(-2.0 * hi), 0, 0, false);
        } else {
          push(i, hi, j, hj, true);
          push(i, hi, j, -hj, true);
          push(i, -hi, j, hj, true);
          push(i, -hi, j, -hj, true);
        }
      }
    uint32_t K = (uint32_t)(sets.size() / N);
    std::vector<float> f = evaluateCameraSets(matchSet, images, sets, K);
    size_t e = 0, h_i = 0;
    for (size_t i = 0; i < N; ++i)
      for (size_t j = 0; j < N; ++j) {
        float hi = h_step[i % 6], hj = h_step[j % 6];
        float numer, denom;
        if (i == j) {
          float A = f[e], B = f[e + 1], C = f[e + 2], D = f[e + 3], E = f[e + 4];
          e += 5;
          numer = (float)(-1.0 * A + 16.0 * B - 30.0 * C + 16.0 * D - 1.0 * E);
          denom = (float)(12.0 * hi * hi);
        } else {
          float A = f[e], B = f[e + 1], C = f[e + 2], D = f[e + 3];
          e += 4;
          numer = A - B - C + D;
          denom = (float)(4.0 * hi * hj);
        }
        hOut->host.get()[h_i++] = numer / denom;
      }
    // upstream's last generateBundles(matchSet,temp,params) leaves the images at params_reset
    ptr::value<Unity<float>> tmp(nullptr, 6, cpu);
    for (size_t j = 0; j < V; ++j) {
      for (int k = 0; k < 6; ++k) tmp->host.get()[k] = reset[6 * j + k];
      images[j]->setFloatVector(tmp);
    }
  }

  // calculateImageHessianInverse (:1511-1824): Moore-Penrose pseudo-inverse, singular values below 1e-4 dropped
  // (:1698), pseudoInverse() of matrix_util.hpp (N = 12).  Input/output row-major like the caller's use with
  // cublasSgemv(CUBLAS_OP_N) on a symmetric matrix.
  ptr::value<Unity<float>> calculateImageHessianInverse(ptr::value<Unity<float>> hessian) {
    const int N = (int)std::lround(std::sqrt((double)hessian->size()));
    std::vector<float> pinv = pseudoInverse(hessian->host.get(), N, 1e-4);
    ptr::value<Unity<float>> inv(nullptr, (unsigned long)(N * N), cpu);
    for (int i = 0; i < N * N; ++i) inv->host.get()[i] = pinv[i];
    return inv;
  }

  // src/PointCloudFactory.cu:1832-2262
  ptr::value<Unity<float3>> BundleAdjustTwoView(MatchSet* matchSet, std::vector<ptr::value<Image>> images, unsigned int iterations, const char* /*debugFilename*/) {
    const int num_params = 6;
    const size_t N = num_params * images.size();
    ptr::value<Unity<float>> gradient(nullptr, (unsigned long)N, cpu);
    ptr::value<Unity<float>> hessian(nullptr, (unsigned long)(N * N), cpu);
    const bool fixed_camera = true;  // :1860: every update is relative to camera 0, which stays put
    logger.info << "\t Bundle Adjustment is in Second Order Mode";
    std::vector<Image::Camera> bestParams, secondBestParams;
    for (auto& im : images) { bestParams.push_back(im->camera); secondBestParams.push_back(im->camera); }
    float alpha = 0.1f;
    const float dist_step = 1.0, angle_mag = 1.0;
    float localError = 0, initialError = 0, bestError;
    std::vector<float> errorTracker;
    BundleSet bundleTemp = generateBundles(matchSet, images);
    voidTwoViewTriangulate(bundleTemp, &initialError);
    errorTracker.push_back(initialError);
    bestError = initialError;
    for (unsigned int i = 0; i < iterations; i++) {
      calculateImageGradient(matchSet, images, gradient);
      calculateImageHessian(matchSet, images, hessian);
      ptr::value<Unity<float>> inverse = calculateImageHessianInverse(hessian);
      std::vector<float> update(N, 0.0f);  // cublasSgemv: update = alpha * inverse * gradient (:2081)
      for (size_t r = 0; r < N; ++r) {
        float acc = 0.0f;
        for (size_t c = 0; c < N; ++c) acc += inverse->host.get()[c * N + r] * gradient->host.get()[c];  // column-major A
        update[r] = alpha * acc;
      }
      int g_j = 0;
      for (size_t j = 0; j < images.size(); j++) {
        if (!fixed_camera && j) {  // :2150 -- never true upstream
          images[j]->camera.cam_pos.x = images[j]->camera.cam_pos.x - dist_step * update[g_j];
          images[j]->camera.cam_pos.y = images[j]->camera.cam_pos.y - dist_step * update[g_j + 1];
          images[j]->camera.cam_pos.z = images[j]->camera.cam_pos.z - dist_step * update[g_j + 2];
          images[j]->camera.cam_rot.x = images[j]->camera.cam_rot.x - angle_mag * update[g_j + 3];
          images[j]->camera.cam_rot.y = images[j]->camera.cam_rot.y - angle_mag * update[g_j + 4];
          images[j]->camera.cam_rot.z = images[j]->camera.cam_rot.z - angle_mag * update[g_j + 5];
        }
        g_j += 6;
      }
      bundleTemp = generateBundles(matchSet, images);
      voidTwoViewTriangulate(bundleTemp, &localError);
      if (localError < bestError) {
        bestError = localError;
        for (size_t j = 0; j < bestParams.size(); j++) { secondBestParams[j] = bestParams[j]; bestParams[j] = images[j]->camera; }
        if (i) alpha /= (errorTracker.back() / localError);
        errorTracker.push_back(localError);
      } else {
        for (size_t j = 0; j < images.size(); j++) images[j]->camera = bestParams[j];
        if (!i) alpha /= 100.0f;
        else break;
      }
    }
    bundleTemp = generateBundles(matchSet, images);
    return twoViewTriangulate(bundleTemp, &localError);
  }

  // ---- a pose applied to a cloud (include/ssrlcv_hip.h "surface registration" item 2): p' = M p + T in place, on the device;
  // a "no result" point -- (0, 0, 0) or a non-finite component -- stays what it is.  The cloud is left in the state it came in.
  // MeshFactory::registerToReference finds such a pose.
  void transformPointCloud(ptr::value<Unity<float3>> cloud, const ssrlcv_register_pose& pose) {
    if (cloud == nullptr || cloud->size() == 0 || cloud->size() > 0xFFFFFFFFul) return;
    GpuWrite<float3> onGpu(cloud);
    ssrlcv_float3* p = (ssrlcv_float3*)cloud->device.get();
    HipSafeCall(ssrlcv_hip_transform_points(p, (uint32_t)cloud->size(), &pose, p, nullptr));
    HipSafeCall(ssrlcv_hip_device_synchronize());
  }

  // Upstream's scalePointCloud / translatePointCloud / rotatePointCloud: a pose built on the host, then transformPointCloud.
  // Scaling and rotating are about the origin.  rotatePointCloud turns about the x axis, then y, then z -- R = Rz Ry Rx of the
  // angles in radians, the order of cam_rot everywhere in this mirror; SURVEY.md and INTEGRATION.md do not record upstream's
  // order for this call, so that one is assumed.
  static ssrlcv_register_pose poseOf(const double (&M)[3][3], float3 t) {
    ssrlcv_register_pose g = {};
    const float tv[3] = {t.x, t.y, t.z};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) g.m[4 * r + c] = (float)M[r][c];
      g.m[4 * r + 3] = tv[r];
    }
    return g;
  }
  void scalePointCloud(float scale, ptr::value<Unity<float3>> cloud) {
    const double M[3][3] = {{scale, 0, 0}, {0, scale, 0}, {0, 0, scale}};
    transformPointCloud(cloud, poseOf(M, {0.0f, 0.0f, 0.0f}));
  }
  void translatePointCloud(float3 translate, ptr::value<Unity<float3>> cloud) {
    const double M[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    transformPointCloud(cloud, poseOf(M, translate));
  }
  void rotatePointCloud(float3 rotate, ptr::value<Unity<float3>> cloud) {
    const double cx = std::cos((double)rotate.x), sx = std::sin((double)rotate.x), cy = std::cos((double)rotate.y), sy = std::sin((double)rotate.y),
                 cz = std::cos((double)rotate.z), sz = std::sin((double)rotate.z);
    const double M[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                            {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                            {-sy, cy * sx, cy * cx}};
    transformPointCloud(cloud, poseOf(M, {0.0f, 0.0f, 0.0f}));
  }
};

}  // namespace ssrlcv
