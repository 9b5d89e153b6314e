/*
 * include/ssrlcv_hip.h -- the drop-in boundary: C ABI of libssrlcv_hip.so (MI355X / gfx950).
 *
 * The reference has no FFI layer; its hot path is the set of __global__ kernels launched from the
 * ssrlcv::{SIFT_FeatureFactory, FeatureFactory::ScaleSpace, MatchFactory<T>, PointCloudFactory} host methods over
 * Unity<T>::device pointers.  This header is what those host methods bind instead of the CUDA
 * kernels: plain device pointers (exactly what Unity<T>::device.get() returns), sizes, a hipStream_t and an int status.
 * ssrlcv_amd/host/ *.hpp holds the C++ shells with the reference's class API that call these entry points;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on that stream unless
 *     the doc says "synchronous" (the reference synchronises after every launch; the C++ shells do that for parity);
 *   - no hidden allocation: scratch comes from a caller-provided workspace (query the size with *_workspace_bytes);
 *   - return 0 on success, >0 = hipError_t, <0 = SSRLCV_ERR_*.  The C++ shells map non-zero to
 *     logger.err + exit(-1) like CudaSafeCall/CudaCheckError (include/Memory.cuh:33-74).
 */
#ifndef SSRLCV_HIP_H
#define SSRLCV_HIP_H
#include "ssrlcv_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSRLCV_OK 0
#define SSRLCV_ERR_INVALID_ARG (-1)
#define SSRLCV_ERR_CAPACITY (-2)  /* a device-side list outgrew the capacity the caller provisioned */
#define SSRLCV_ERR_WORKSPACE (-3) /* workspace too small */
#define SSRLCV_ERR_UNSUPPORTED (-4)

typedef void* ssrlcv_stream_t; /* hipStream_t */

/* ABI version: bumped on EVERY change of an exported signature, of a struct layout in ssrlcv_types.h or of the meaning of
 * an argument.  A pure addition of new entry points (no existing signature, layout or meaning changes) keeps the number:
 * a binder that does not call them is unaffected, and one that does fails loudly against an older library (C++ at
 * symbol resolution; Python in ssrlcv_amd/_lib.py, which checks that every name of its EXPORTED list resolves).  A caller
 * compiled against this header compares the library it loaded with the number it was built for before the first call:
 * the C++ mirror does (host/Memory.hpp ssrlcv::requireAbi, on first use) and so does the Python loader.
 *   1  rounds 1-4 (unversioned)
 *   2  round 5: ssrlcv_hip_merge_matches counts[2] -> counts[4] and one argument fewer; select_pair_bundles,
 *      set/get_match_arithmetic, ssrlcv_sift_plan_set_stage_event added
 *   3  round 6: ssrlcv_hip_abi_version itself
 *   4  fundamental-matrix RANSAC: fmatrix_ransac (+ its workspace query), fmatrix_score, pose_from_fmatrix added;
 *      later, as pure additions: knn, neighbor_distance_filter (+ their workspace queries), point_normals;
 *      match2_workspace_bytes, match_knn2_u8x128, match_ratio_u8x128;
 *      dense SIFT: sift_dense_grid, sift_dense_max_features, sift_dense_workspace_bytes, sift_dense_u8;
 *      dense stereo: stereo_workspace_bytes, stereo_sad_u8, stereo_matches_workspace_bytes, stereo_matches, stereo_points;
 *      rectification: rectify_cameras_host, warp_homography_u8, stereo_mask_rectified, matches_apply_homography;
 *      semi-global matching: stereo_sgm_workspace_bytes, stereo_sgm_u8, stereo_sgm_set_pass_events;
 *      census cost: census_u8, stereo_census_workspace_bytes, stereo_census_u8, stereo_sgm_census_workspace_bytes,
 *      stereo_sgm_census_u8;
 *      disparity post-filters: disparity_components, stereo_filter_speckles (+ their workspace queries), stereo_filter_median;
 *      hole filling: stereo_fill_holes (+ its workspace query);
 *      disparity mesh: disparity_mesh, mesh_select, mesh_triangles (+ their workspace queries), mesh_normals;
 *      surface accuracy: dsm_difference, difference_stats (+ its workspace query);
 *      surface registration: register_terms (+ its workspace query), transform_points, register_step_host,
 *      register_compose_host;
 *      mesh render: mesh_render (+ its workspace query), image_residual;
 *      surface simplification: dsm_simplify_errors, dsm_simplify_mesh (+ its workspace query);
 *      terrain filter: dsm_morphology, dsm_terrain (+ their workspace queries), dsm_subtract;
 *      shift search: shift_search (+ its workspace query), shift_table_bytes, shift_pick_host;
 *      surface objects: dsm_objects (+ its workspace query), object_measures_host */
#define SSRLCV_HIP_ABI_VERSION 4
int ssrlcv_hip_abi_version(void);
const char* ssrlcv_hip_version(void);
const char* ssrlcv_hip_status_string(int status);

/* ============================== L0: device memory for the Unity<T> host mirror ================================ */
/* What ptr::device / ptr::host(pinned) / Unity<T>::transferMemoryTo reach through cudaMalloc, cudaMallocHost,
 * cudaMemcpy, cudaFree, cudaFreeHost and cudaDeviceSynchronize (include/Memory.cuh:96-245, include/Unity.cuh:820-854).
 * Exported so that host code above the boundary needs no HIP headers.  kind: 0 H2D, 1 D2H, 2 D2D (synchronous, ordered
 * behind the null stream like cudaMemcpy).  Copies of 4 MB and more to or from PAGEABLE host memory (Unity<T>'s unpinned
 * `new T[]` state) are pipelined through two pinned 8 MB bounce buffers by a small team of host threads instead of the
 * runtime's own staging (csrc/capi_common.hip). */
int ssrlcv_hip_device_count(int* count_host);
int ssrlcv_hip_malloc(void** devPtr_host, size_t bytes);
int ssrlcv_hip_free(void* devPtr);
int ssrlcv_hip_host_malloc(void** hostPtr_host, size_t bytes);
int ssrlcv_hip_host_free(void* hostPtr);
int ssrlcv_hip_memcpy(void* dst, const void* src, size_t bytes, int kind);
int ssrlcv_hip_memset(void* devPtr, int value, size_t bytes);
int ssrlcv_hip_device_synchronize(void);

/* ============================== P: point cloud ==================================================== */

/* generateBundle kernel (src/PointCloudFactory.cu:4166-4199), launched by PointCloudFactory::generateBundles
 * (:832-925, :934-1051).  One thread per multi-match; lines[i] for every key point i of the match.
 * cameras is read-only here (the reference rewrites cameras[].dpix from every thread, a benign race on a temporary). */
int ssrlcv_hip_generate_bundles(const ssrlcv_multimatch* matches, const ssrlcv_keypoint* keyPoints, uint32_t numBundles,
                                const ssrlcv_camera* cameras, uint32_t numCameras, ssrlcv_bundle* bundles,
                                ssrlcv_line* lines, ssrlcv_stream_t stream);

/* generatePushbroomBundle kernel (src/PointCloudFactory.cu:4201-4283). */
int ssrlcv_hip_generate_pushbroom_bundles(const ssrlcv_multimatch* matches, const ssrlcv_keypoint* keyPoints,
                                          uint32_t numBundles, const ssrlcv_pushbroom* pushbrooms, uint32_t numCameras,
                                          ssrlcv_bundle* bundles, ssrlcv_line* lines, ssrlcv_stream_t stream);

/* computeTwoViewTriangulate x4 + voidComputeTwoViewTriangulate x2 (src/PointCloudFactory.cu:4457-4869) in one entry:
 *   points  NULL -> the void variants;  errors NULL -> no per-bundle error;  cutoff NULL -> invalid=false, else
 *   bundles[i].invalid = error > *cutoff;  errorSum (one float, must be zeroed by the caller like the reference's
 *   d_linearError) receives the sum of ||s1-s2||^2. */
int ssrlcv_hip_triangulate2(const ssrlcv_line* lines, ssrlcv_bundle* bundles, uint32_t numBundles, ssrlcv_float3* points,
                            float* errors, const float* cutoff, float* errorSum, ssrlcv_stream_t stream);

/* computeNViewTriangulate x4 (src/PointCloudFactory.cu:4880-5193).  noErrorVariant != 0 selects the first overload
 * (:4880-4930: marks bundles[i].invalid when S is singular, computes no error). */
int ssrlcv_hip_triangulateN(const ssrlcv_line* lines, ssrlcv_bundle* bundles, uint32_t numBundles, ssrlcv_float3* points,
                            float* errors, const float* cutoff, float* errorSum, int noErrorVariant,
                            ssrlcv_stream_t stream);

/* The evaluation BundleAdjustTwoView repeats 24 + 588 + 1 times per iteration (calculateImageGradient
 * src/PointCloudFactory.cu:1059-1248, calculateImageHessian :1256-1504): Image::setFloatVector (src/Image.cu:445-472)
 * + generateBundle + voidComputeTwoViewTriangulate, fused.  params holds K camera-parameter sets of
 * numCameras*6 floats {pos.xyz, rot.xyz}; errorSums[k] receives f(params_k).  One launch evaluates all K sets with
 * the matches read once.  workspace: ssrlcv_hip_ba_sweep2_workspace_bytes(numBundles, K). */
size_t ssrlcv_hip_ba_sweep2_workspace_bytes(uint32_t numBundles, uint32_t K);
int ssrlcv_hip_ba_sweep2(const ssrlcv_multimatch* matches, const ssrlcv_keypoint* keyPoints, uint32_t numBundles,
                         const ssrlcv_camera* cameras, uint32_t numCameras, const float* params, uint32_t K,
                         float* errorSums, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- pose refinement ----
 * The device part of PoseEstimator::LM_iteration (src/PoseEstimator.cu:349-393): computeResidualsAndJacobian
 * (:647-729, central differences with delta 1e-5 on roll/pitch/yaw, position columns 0), computeJTJ / computeJTf
 * (:814-844) and computeCost (:731-740) fused; the per-match residual is getResidual (:742-812).
 * out43 (device): JTJ[36] with JTJ[i + 6 j], then JTf[6], then the cost sum(|f|^2).
 * Contract (tests/test_gpu_pose_edges.py):
 *   - all 43 floats are written whatever they held; numMatches == 0 gives all +0.  Stream-ordered, no host
 *     synchronisation.  A NULL matches, pose, query, target or out43: SSRLCV_ERR_INVALID_ARG, nothing written.
 *   - JTJ is exactly symmetric (one triangle is summed, the other copied).
 *   - the position rows and columns (3..5) of JTJ and JTf[3..5] are +0 ALWAYS.  This is this library's deliberate
 *     difference: upstream (and the CPU oracle) multiply the zero position columns into the sums, so a residual that is
 *     not finite gives NaN * 0 = NaN there; the kernel never forms those products.
 *   - the per-match residual f and Jacobian J are the float32 values of the reference's expressions; the ORDER of the
 *     sums over rows and matches is unspecified.  Every returned sum lies within gamma_d * sum |terms| of the exact sum
 *     of its float32 terms (J[r][a] * J[r][b], J[r][a] * f[r], one |f|^2 per match), gamma_d = d u / (1 - d u),
 *     u = 2^-24, d the longest chain of additions of the launch (terms per thread + 6 butterfly levels + one atomic per
 *     wave: 4108 for 262 145 to 524 288 matches); with one match no order enters and the result is bit-exact.  A sum
 *     over a NaN term is NaN. */
int ssrlcv_hip_pose_lm_terms(const ssrlcv_match* matches, uint32_t numMatches, const ssrlcv_pose* pose,
                             const ssrlcv_camera* query, const ssrlcv_camera* target, float* out43,
                             ssrlcv_stream_t stream);
/* computeCost alone (:731-740), for the trial poses of the inner LM loop; cost: one device float, under the same
 * contract as out43[42] (always written, +0 for numMatches == 0, summation order unspecified within the same bound). */
int ssrlcv_hip_pose_cost(const ssrlcv_match* matches, uint32_t numMatches, const ssrlcv_pose* pose,
                         const ssrlcv_camera* query, const ssrlcv_camera* target, float* cost, ssrlcv_stream_t stream);

/* ---- fundamental-matrix RANSAC and relative pose (PoseEstimator::estimatePoseRANSAC, src/PoseEstimator.cu:92-312) ----
 * PARITY UNPINNED: the reference holds no fixture for this path; these conventions are this library's own.
 *   matches     ssrlcv_match: q = keyPoints[0].loc (query pixel), t = keyPoints[1].loc (target pixel).  A match with
 *               invalid != 0 is never an inlier; a sample that draws one yields no candidate.
 *   constraint  t~^T F q~ = 0 with q~ = (q.x, q.y, 1).  Every F is row-major float[9] in pixel coordinates, scaled to unit
 *               Frobenius norm, sign fixed so that the entry of largest magnitude is positive (lowest index on ties).
 *   inlier      Sampson distance below `threshold` px:
 *               (t~^T F q~)^2 < threshold^2 ((F q~)_0^2 + (F q~)_1^2 + (F^T t~)_0^2 + (F^T t~)_1^2); a zero denominator
 *               is not an inlier.
 *   normalise   one similarity per image: translate by the centre of that image's bounding box of the VALID match
 *               locations; one common scale s = 2 / (largest extent of either box).  Solving and scoring run in
 *               normalised coordinates with threshold s * threshold (the Sampson distance scales by s exactly).  A pixel
 *               F is taken to normalised coordinates in float64 and rescaled to unit norm before it is tested, so a
 *               candidate scores the same in the RANSAC and in ssrlcv_hip_fmatrix_score.
 *   samples     sample h (0 <= h < numSamples): for j = 0, 1, ... z = seed + (h 2^32 + j + 1) 0x9E3779B97F4A7C15 (mod 2^64),
 *               splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9; z ^= z >> 27, z *= 0x94D049BB133111EB;
 *               z ^= z >> 31), index ((z >> 32) numMatches) >> 32; duplicates skipped until 7 distinct indices, at most
 *               64 draws (else no candidate).
 *   solver      float64: null space F1, F2 of the 7x9 system A (Householder reflections from the right,
 *               A H_0 ... H_6 = [L | 0], F1 = H_0 ... H_6 e_7, F2 = H_0 ... H_6 e_8: the order of the roots depends on
 *               this basis), real roots of det(a F1 + (1 - a) F2) in
 *               ascending order (cubic through its values at a = 0, 1, -1, 2; when the leading coefficient is below
 *               1e-12 of the largest the lower-degree polynomial is solved), candidate r of sample h in slot 3 h + r,
 *               denormalised to pixels.  Empty slots: F all zero, count 0.
 *   best        largest count, lowest slot on ties (one 64-bit atomicMax of (count << 32 | ~slot)).
 *   refit       always: least-squares 8-point fit on the best candidate's inliers (9x9 float64 normal matrix from
 *               per-block partials summed in block order, Jacobi eigenvector of the smallest eigenvalue, rank 2 through
 *               the 3x3 SVD); kept when it has at least as many inliers.
 *   determinism two calls with the same inputs give bit-equal F, count, mask, candidates and counts (integer counts, no
 *               float atomics).
 * Fewer than 7 matches, fewer than 7 valid ones, or no candidate with an inlier: SSRLCV_OK, count 0, F all zero. */
/* the scratch of fmatrix_score and pose_from_fmatrix: a workspace of at least this many bytes */
#define SSRLCV_FMATRIX_AUX_WORKSPACE_BYTES 256
size_t ssrlcv_hip_fmatrix_ransac_workspace_bytes(uint32_t numMatches, uint32_t numSamples);
/* F_out: 9 floats; inlierCount_out: one uint32; inlierMask_out (NULL: none): numMatches bytes, 1 = inlier of F_out;
 * candidates_out (NULL: none): 27 numSamples floats; counts_out (NULL: none): 3 numSamples uint32.  All device memory.
 * Fully stream-ordered (no host synchronisation), so it may be captured into a graph.
 * SSRLCV_ERR_INVALID_ARG: matches, F_out, inlierCount_out or workspace NULL, numSamples 0 or above 2^26, threshold not
 * a positive finite number.  SSRLCV_ERR_WORKSPACE: workspaceBytes below the query. */
int ssrlcv_hip_fmatrix_ransac(const ssrlcv_match* matches, uint32_t numMatches, uint32_t numSamples, float threshold,
                              uint64_t seed, void* workspace, size_t workspaceBytes, float* F_out,
                              uint32_t* inlierCount_out, uint8_t* inlierMask_out, float* candidates_out,
                              uint32_t* counts_out, ssrlcv_stream_t stream);
/* The RANSAC's scoring kernel on its own: counts_out[i] = inliers of F[9 i .. 9 i + 8] (k candidates, device), with
 * the normalisation above taken from these matches.  inlierMask_out only with k == 1.  Stream-ordered. */
int ssrlcv_hip_fmatrix_score(const ssrlcv_match* matches, uint32_t numMatches, const float* F, uint32_t k, float threshold,
                             void* workspace, size_t workspaceBytes, uint32_t* counts_out, uint8_t* inlierMask_out,
                             ssrlcv_stream_t stream);
/* Relative pose from F (device, 9 floats) in the convention pose_lm_terms consumes: the target ray rotated by
 * (roll, pitch, yaw), placed at (x, y, z) in the query camera's frame.  Intrinsics of the ray model:
 * K = [[foc / dpix.x, 0, size.x / 2], [0, foc / dpix.y, size.y / 2], [0, 0, 1]], E = K_t^T F K_q projected to singular
 * values (1, 1, 0); of its four (R, C) the one with the most matches whose two ray depths are positive wins (device
 * vote, integer counts, lowest candidate on ties) over the matches with inlierMask != 0 (NULL: every valid match).
 * Angles: getAxisRotations of the rotation; position: the unit direction of C times |target.cam_pos - query.cam_pos| / 1000
 * (LM_optimize's scale).  Synchronous.  F all zero: SSRLCV_ERR_INVALID_ARG. */
int ssrlcv_hip_pose_from_fmatrix(const ssrlcv_match* matches, uint32_t numMatches, const uint8_t* inlierMask,
                                 const float* F, const ssrlcv_camera* query_host, const ssrlcv_camera* target_host,
                                 void* workspace, size_t workspaceBytes, ssrlcv_pose* pose_host, ssrlcv_stream_t stream);

/* ---- point cloud: k nearest neighbours, statistical neighbour-distance filter, normals (MeshFactory) -------------------
 * PARITY UNPINNED: the reference's Octree-based filters and normal estimation have no fixture; this contract is the
 * definition.  Points are n ssrlcv_float3 in device memory; 1 <= k <= SSRLCV_KNN_MAX_K and n >= k + 1.
 *   non-finite  a point with any NaN or +-inf coordinate is excluded: no neighbours (index UINT32_MAX, dist2 +inf), never
 *               anyone's neighbour, mean distance +inf (always removed by the filter, left out of its statistics), normal
 *               (0, 0, 0).  A finite point with fewer than k finite other points has the same empty tail.
 *   k-NN        the neighbours of i are the k points j != i smallest by the key (d2(i, j), j), in ascending key order, with
 *               dx = p[j].x - p[i].x (likewise y, z) and d2 = (dx*dx + dy*dy) + dz*dz in float32, every product and sum
 *               rounded in that order.  Duplicates (d2 = 0) are ordinary neighbours; ties go to the lower index.  The
 *               result is unique: it does not depend on the cell size, the launch shape or scheduling.  This holds for
 *               every finite input, tiny and huge scales included: where the products are subnormal or underflow to 0 the
 *               float32 key, not the distance, still decides (all d2 = 0: the k lowest indices), and where they overflow
 *               d2 = +inf with a valid index, ties by index.  The grid search relies on d2 following the true distance
 *               (to 5 2^-24 relative: difference, product, two sums) only for squared distances of 2^-100 and more, where
 *               no significant product underflows; below, every query is answered by the exact scan over all points.
 *   mean        m_i = (sqrtf(d2_1) + ... + sqrtf(d2_k)) / k: a sequential float32 sum in neighbour order, one division.
 *   filter      over the points with finite m_i: mu = sum(m_i) / n_f, std = sqrt(sum((m_i - mu)^2) / n_f) (population),
 *               both float64 through a fixed partition and a fixed tree (no float atomics: bit-identical run to run);
 *               t = mu + sigma * std; point i is kept iff m_i is finite and (double)m_i <= t.  No such point: {0, 0, 0}.
 *   normals     covariance of the k + 1 points (i and its neighbours) about their mean, float64; the unit eigenvector of
 *               the smallest eigenvalue (cyclic Jacobi, fixed sweep count), oriented so that dot(n, viewpoint - p_i) >= 0,
 *               written as float32.  Zero covariance (all k + 1 coincident) or a missing neighbour: (0, 0, 0).  A
 *               collinear neighbourhood gets some unit vector orthogonal to the line.
 * All three are stream-ordered (no host synchronisation).  SSRLCV_ERR_INVALID_ARG (before any launch): k out of range,
 * n < k + 1, a required pointer NULL.  SSRLCV_ERR_WORKSPACE: workspaceBytes below the query. */
#define SSRLCV_KNN_MAX_K 32
size_t ssrlcv_hip_knn_workspace_bytes(uint32_t numPoints, uint32_t k);
/* neighbors_out: n k uint32, row i = the neighbours of i; dist2_out (NULL: none): n k floats, their d2.
 * cellSize: the grid cell edge in the points' units (raised to the largest extent / 2^20 when smaller); 0 = automatic
 * (from the bounding box and n, re-sized once to about k points per occupied cell).  Queries still open after the grid's
 * ring cap are answered exactly by a scan over all points; farQueries (NULL: not wanted) receives their count (one
 * device uint32).  A negative or non-finite cellSize: SSRLCV_ERR_INVALID_ARG. */
int ssrlcv_hip_knn(const ssrlcv_float3* points, uint32_t numPoints, uint32_t k, float cellSize, uint32_t* neighbors_out,
                   float* dist2_out, uint32_t* farQueries, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_neighbor_filter_workspace_bytes(uint32_t numPoints, uint32_t k);
/* dist2: the n k distances of ssrlcv_hip_knn.  meanDist_out (NULL: none): n floats m_i.  stats_out: device double[3]
 * {mu, std, t}.  pointsOut / indexOut: the kept points and their input indices, in input order (capacity n);
 * normalsIn / normalsOut (both NULL or both set): n x 3 floats compacted the same way.  count_out: one device uint32.
 * sigma: any finite value.  All device memory. */
int ssrlcv_hip_neighbor_distance_filter(const ssrlcv_float3* points, uint32_t numPoints, const float* dist2, uint32_t k,
                                        float sigma, float* meanDist_out, double* stats_out, ssrlcv_float3* pointsOut,
                                        uint32_t* indexOut, const float* normalsIn, float* normalsOut, uint32_t* count_out,
                                        void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
/* neighbors: the n k indices of ssrlcv_hip_knn; normals_out: n x 3 floats (device).  viewpoint (host value, finite):
 * e.g. the mean camera position.  No workspace. */
int ssrlcv_hip_point_normals(const ssrlcv_float3* points, uint32_t numPoints, const uint32_t* neighbors, uint32_t k,
                             ssrlcv_float3 viewpoint, float* normals_out, ssrlcv_stream_t stream);

/* ============================== M: matching ======================================================= */

typedef struct {
  int mode;                 /* 0 = matchFeaturesBruteForce, 1 = matchFeaturesDoubleConstrained, 2 = matchFeaturesConstrained */
  uint32_t queryImageID;    /* Image::id of the query / target (written into the outputs) */
  uint32_t targetImageID;
  float epsilon;            /* px buffer around the epipolar segment (mode 1) / line (mode 2) */
  float delta;              /* km buffer on the earth-shell radii (mode 1) */
  float relativeThreshold;  /* used only when seedDistances != NULL */
  float absoluteThreshold;
  ssrlcv_camera queryCamera;          /* mode 1 */
  ssrlcv_float4 targetProjection[3];  /* mode 1: getProjectionMatrix(target) (src/Image.cu:498-539) */
  float fundamental[9];               /* mode 2: row-major F, epipolar line l = F (x, y, 1) (src/MatchFactory.cu:1722-1724) */
} ssrlcv_match_params;

#define SSRLCV_OUT_DMATCH 0      /* DMatch      (src/MatchFactory.cu:2073-2125, :2194-2291; ratio test vs rel^2) */
#define SSRLCV_OUT_UINT2_PAIR 1  /* uint2_pair  (src/MatchFactory.cu:2714-2760, :2824-2916; ratio test vs rel)   */
#define SSRLCV_OUT_MATCH 2       /* Match       (brute force :1462-1506, :1658-1708: ratio test vs rel; double-constrained
                                  *               :1508-1597, :1777-1873: vs rel^2; F-matrix :1599-1657, :1710-1775: vs rel) */

/* getProjectionMatrix (src/Image.cu:498-539) -- host arithmetic, exposed so shells and tests share one definition. */
void ssrlcv_projection_matrix_host(const ssrlcv_camera* camera_host, ssrlcv_float4 P_host[3]);

size_t ssrlcv_hip_match_workspace_bytes(uint32_t numQuery, uint32_t numTarget);

/* The arithmetic of the distance contraction behind every matcher entry point below (no reference counterpart: upstream's
 * distProtocol, src/Feature.cu:36-42, is a scalar fp32 loop whose sums are exact integers).  Both forms are exact and give
 * identical outputs; the setting is process-wide and takes effect at the next call.
 *   SSRLCV_MATCH_ARITH_I8  (default) v_mfma_i32_32x32x32_i8 on descriptors shifted to int8, norms in the start values
 *   SSRLCV_MATCH_ARITH_F16           v_mfma_f32_32x32x16_f16, norms as base-1024 digits in one extra K step */
#define SSRLCV_MATCH_ARITH_I8 0
#define SSRLCV_MATCH_ARITH_F16 1
int ssrlcv_hip_set_match_arithmetic(int arithmetic);
int ssrlcv_hip_get_match_arithmetic(void);

/* getSeedMatchDistances (src/MatchFactory.cu:1432-1460): out[q] = min_f distProtocol(query[q], seed[f]). */
int ssrlcv_hip_seed_distances_u8x128(const ssrlcv_sift_feature* query, uint32_t numQuery, const ssrlcv_sift_feature* seed,
                                     uint32_t numSeed, float* out, void* workspace, size_t workspaceBytes,
                                     ssrlcv_stream_t stream);

/* The 128-D brute-force contraction.  Replaces the 27 matchFeatures* kernels of src/MatchFactory.cu for T =
 * SIFT_Descriptor: winner per query = smallest (distance, f mod 32, f) among targets passing the mode's prefilter with
 * distance < absoluteThreshold -- the order the reference's 32-lane scan + lane-0 reduction produces (:2256-2271).
 * out has numQuery elements of the struct selected by outKind; seedDistances may be NULL. */
int ssrlcv_hip_match_u8x128(const ssrlcv_sift_feature* query, uint32_t numQuery, const ssrlcv_sift_feature* target,
                            uint32_t numTarget, const float* seedDistances, const ssrlcv_match_params* params_host,
                            int outKind, void* out, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- two nearest neighbours, Lowe's ratio test and the mutual check.
 * PARITY UNPINNED: upstream rejects a match by an absolute threshold or by its ratio against a seed image only; it has no
 * second neighbour and no cross check, so this contract is the library's own.
 *   order       the neighbours of query q are the two targets smallest by the key (distance, f mod 32, f) -- the key of
 *               ssrlcv_hip_match_u8x128, so neighbour 1 is that call's brute-force (mode 0) winner at an infinite
 *               threshold.  distance = the exact integer squared L2 of the descriptors (< 2^23).
 *   missing     a neighbour that does not exist (numTarget 0 or 1): index UINT32_MAX, distance +inf.
 *   ratio       passes iff (float)d1 < (ratio * ratio) * (float)d2, each product rounded to float32 in that order.  A
 *               missing second neighbour passes; ratio == 0: no test.  0 <= ratio <= 1 and finite, anything else
 *               SSRLCV_ERR_INVALID_ARG.  d1 == d2 fails for every ratio > 0 (duplicate targets are ambiguous).
 *   absolute    a match with d1 >= absoluteThreshold is rejected, as in ssrlcv_hip_match_u8x128.
 *   mutual      != 0: the match (q, j) is kept only if q is neighbour 1 of target j among ALL queries -- same key, with
 *               (q mod 32, q); no threshold and no ratio applies to that reverse pass.
 *   outputs     the structs of ssrlcv_hip_match_u8x128 (outKind), a kept or rejected entry laid out as that call writes
 *               it: distance = d1 (absoluteThreshold when there is no neighbour); a rejected uint2_pair has b = a, a rejected
 *               DMatch / Match invalid = 1 and zero key points; padding bytes are zero.  ssrlcv_hip_compact_matches[_async]
 *               and ssrlcv_hip_matchset_from_matches take them unchanged.
 *   workspace   ssrlcv_hip_match2_workspace_bytes(numQuery, numTarget) bytes.  It BEGINS with the layout of
 *               ssrlcv_hip_match_workspace_bytes(numQuery, numTarget), so the same buffer is a valid workspace for
 *               compacting the numQuery results; the partial keys of the target splits and the (numTarget, numQuery)
 *               layout of the mutual check's reverse pass follow.
 *   determinism both calls are stream-ordered without host synchronisation (kernels only, one chain on `stream`: they may
 *               be captured into a graph) and use no atomics for their results: two calls on the same inputs give
 *               bit-equal outputs.
 *   arguments   checked before any launch: query, out / index_out, workspace, params_host NULL, target NULL with
 *               numTarget > 0, outKind outside 0..2, ratio, a NaN absoluteThreshold -> SSRLCV_ERR_INVALID_ARG; then
 *               numQuery == 0 -> SSRLCV_OK; then a workspace too small -> SSRLCV_ERR_WORKSPACE.
 * The distance contraction is int8 MFMA whatever ssrlcv_hip_set_match_arithmetic says (both arithmetics are exact); the
 * reverse pass of the mutual check is the one-nearest matcher and follows that setting. */
size_t ssrlcv_hip_match2_workspace_bytes(uint32_t numQuery, uint32_t numTarget);
/* index_out: numQuery x 2 uint32; dist_out (NULL: none): numQuery x 2 float. */
int ssrlcv_hip_match_knn2_u8x128(const ssrlcv_sift_feature* query, uint32_t numQuery, const ssrlcv_sift_feature* target,
                                 uint32_t numTarget, uint32_t* index_out, float* dist_out, void* workspace,
                                 size_t workspaceBytes, ssrlcv_stream_t stream);
typedef struct {
  uint32_t queryImageID, targetImageID; /* written into the outputs */
  float ratio;
  float absoluteThreshold;
  int mutual;
} ssrlcv_ratio_params;
int ssrlcv_hip_match_ratio_u8x128(const ssrlcv_sift_feature* query, uint32_t numQuery, const ssrlcv_sift_feature* target,
                                  uint32_t numTarget, const ssrlcv_ratio_params* params_host, int outKind, void* out,
                                  void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* validateMatches (src/MatchFactory.cu:32-108): stable removal of invalid entries (thrust::remove_if).  In place;
 * *count_host receives the survivors.  Synchronous (returns after the count is on the host, like the reference).
 * A DMatch or Match is invalid when its `invalid` byte is not 0 (any value, not only 1); a uint2_pair when a.x == b.x and
 * a.y == b.y (a pair that shares one of the two is kept).  The survivors are moved whole, in input order, to the front of
 * the list; the records behind them, [count, numMatches), are left as they were, and nothing outside the list is written.
 * workspace: numMatches * sizeof(record) + 256 + 4 * (4 * ceil(numMatches / 2048) + 3) bytes are enough (a workspace of
 * ssrlcv_hip_match_workspace_bytes / _match2_workspace_bytes for the call that made the list is too); nothing is written
 * past that many bytes, one byte less is SSRLCV_ERR_WORKSPACE, and a workspace may hold anything on entry. */
int ssrlcv_hip_compact_matches(int outKind, void* matches, uint32_t numMatches, uint32_t* count_host, void* workspace,
                               size_t workspaceBytes, ssrlcv_stream_t stream);

/* The same compaction without the host round trip: asynchronous on `stream`; *count_dev (one device uint32) receives the
 * number of survivors, which are left at the front of `matches`.  For callers that queue many pairs and read all the
 * counts after one synchronisation (the per-pair D2H count of the call above was a stall per image pair).
 * outKind SSRLCV_OUT_DMATCH or SSRLCV_OUT_UINT2_PAIR; the 40-byte Match is not a multiple of the 16-byte words the
 * counted copy moves, and neither is a list that does not begin on a 16-byte boundary: with numMatches > 0 either is
 * SSRLCV_ERR_UNSUPPORTED, nothing touched (use ssrlcv_hip_compact_matches).  numMatches == 0 is answered first by both
 * calls: SSRLCV_OK, a count of 0, list and workspace untouched, whatever the kind, the alignment and workspaceBytes.
 * Rules, order, the records behind the survivors and the workspace as above. */
int ssrlcv_hip_compact_matches_async(int outKind, void* matches, uint32_t numMatches, uint32_t* count_dev, void* workspace,
                                     size_t workspaceBytes, ssrlcv_stream_t stream);

/* 2-view MatchSet assembly of doFeatureMatching (src/Pipeline.cu:198-224) as one device pass, so that the validated
 * match list never travels to the host: keyPoints[2 i], keyPoints[2 i + 1] = the end points of match i and
 * multiMatches[i] = {2, 2 i}.  inKind = SSRLCV_OUT_DMATCH or SSRLCV_OUT_MATCH (the reference slices DMatch to Match first,
 * src/MatchFactory.cu:257-280; the slice is a no-op here).  maxDistance (nullable; one device float; DMatch input only)
 * receives max(0, max_i distance_i), the figure the reference logs from a host loop (:198-203). */
int ssrlcv_hip_matchset_from_matches(int inKind, const void* matches, uint32_t numMatches, ssrlcv_keypoint* keyPoints,
                                     ssrlcv_multimatch* multiMatches, float* maxDistance, ssrlcv_stream_t stream);

/* ---- filters between triangulation and bundle adjustment, the host halves of
 * PointCloudFactory::linearCutoffFilter (src/PointCloudFactory.cu:3500-3644) and deterministicStatisticalFilter
 * (:3070-3275) on the device.  A filter = generate_bundles -> triangulate2/N with errors [-> error_sample_cutoff ->
 * triangulate2/N with that cutoff] -> filter_matchset, all queued on one stream; only the two counts come back. */
/* :3121-3156: *cutoff (DEVICE float) = sigma * sqrtf(variance) of the sample errors[0], errors[sampleJump], ... (the first
 * (numErrors - numErrors % sampleJump) / sampleJump of them), mean and variance by sequential float sums in index order
 * like the host loops upstream.  sampleJump = (int)(1 / sampleSize) is the caller's. */
int ssrlcv_hip_error_sample_cutoff(const float* errors, uint32_t numErrors, uint32_t sampleJump, float sigma, float* cutoff,
                                   ssrlcv_stream_t stream);
/* :3159-3272, :3517-3644: the MatchSet without the bundles flagged invalid, order kept: matchesOut[j] = {numLines,
 * running index}, keyPointsOut = the kept bundles' key points in order (source offset = running sum of ALL bundles'
 * numLines, i.e. the key points must lie in bundle order as every MatchSet of the reference does).  Covers the two-view
 * form ({2, 2 k_adjust}) and the N-view form.  counts: DEVICE uint32[3] = {bundles kept, key points kept, key points in}.
 * One pass (decoupled look-back scan, csrc/scan_lookback.h); workspace from ssrlcv_hip_filter_workspace_bytes. */
size_t ssrlcv_hip_filter_workspace_bytes(uint32_t numBundles);
int ssrlcv_hip_filter_matchset(const ssrlcv_bundle* bundles, const ssrlcv_keypoint* keyPoints, uint32_t numBundles,
                               ssrlcv_multimatch* matchesOut, ssrlcv_keypoint* keyPointsOut, uint32_t* counts, void* workspace,
                               size_t workspaceBytes, ssrlcv_stream_t stream);

/* The two-view bundles of image pair (imageA, imageB) of an N-view MatchSet as a two-camera MatchSet, order kept: what
 * BundleAdjustTwoView (src/PointCloudFactory.cu:1832-2262, a two-view method) is given in the N-view flows.  A multi-match
 * is taken when numKeyPoints == 2 and its key points' parentIds are imageA, imageB (the order generateMatchesExhaustive
 * writes, src/MatchFactory.cu:1007-1020); matchesOut[j] = {2, 2 j}, keyPointsOut[2 j], [2 j + 1] = the pair with parentId 0 / 1.
 * Outputs hold up to numMatches / 2 numMatches entries; *count (DEVICE uint32) = bundles selected.  One look-back pass. */
size_t ssrlcv_hip_select_pair_workspace_bytes(uint32_t numMatches);
int ssrlcv_hip_select_pair_bundles(const ssrlcv_multimatch* matches, const ssrlcv_keypoint* keyPoints, uint32_t numMatches,
                                   uint32_t numKeyPoints, int imageA, int imageB, ssrlcv_multimatch* matchesOut,
                                   ssrlcv_keypoint* keyPointsOut, uint32_t* count, void* workspace, size_t workspaceBytes,
                                   ssrlcv_stream_t stream);

/* The sort behind the spatial orders of the band-culled modes (no reference counterpart: upstream tests every pair).
 * Keys are (strip << 16 | position) words; perm[0 .. n) = 0 .. n-1 ordered by ascending (bucket, key, index) with
 * bucket = ((key >> 16) + 2048) mod 4096: bucketed by strip, bitonic-sorted per bucket in LDS (csrc/spatial_sort.hip).
 * While all strips lie in [30720, 34816) -- 2048 strips either side of the origin: frame coordinates within +-8 192 px at 4-px strips, +-32 768 px at 16 -- that IS the order by
 * (key, index); beyond, strips 4096 apart share a bucket (and stay separated inside it): still a grouping by strip, which
 * is all the matcher needs.  keys and perm are device arrays; asynchronous on `stream`. */
size_t ssrlcv_hip_sort_workspace_bytes(uint32_t n);
int ssrlcv_hip_sort_keys_u32(const uint32_t* keys, uint32_t n, uint32_t* perm, void* workspace, size_t workspaceBytes,
                             ssrlcv_stream_t stream);

/* Tail of generateMatchesExhaustive (src/MatchFactory.cu:1007-1020): KeyPoint{parentId = image, loc = that feature's
 * location} for every member {image, feature index} of the merged MatchSet, gathered on the device.  members: device
 * array of numMembers {x = image, y = feature}; features_host: HOST array of numImages device pointers.  keyPoints must
 * be 16-byte aligned (any device allocation is; a sub-array must start at an even byte offset / 16): each 16-byte element,
 * padding included (the 4 bytes behind parentId are zero), is written with one store -- SSRLCV_ERR_INVALID_ARG otherwise.
 * A member that names no image (x >= numImages), no feature of its image (y >= numFeatures_host[x]) or an image whose
 * array pointer is NULL (its count is then not read) gets parentId = x and the location (0, 0): upstream indexes its
 * arrays with such a member unchecked, so there is nothing to reproduce, and no array is read out of bounds here.
 * numMembers == 0: SSRLCV_OK, nothing touched.  One launch per 64 images over the same member list. */
int ssrlcv_hip_keypoints_from_members(const ssrlcv_uint2* members, uint32_t numMembers,
                                      const ssrlcv_sift_feature* const* features_host, const uint32_t* numFeatures_host,
                                      uint32_t numImages, ssrlcv_keypoint* keyPoints, ssrlcv_stream_t stream);

/* Host half of generateMatchesExhaustive (src/MatchFactory.cu:943-1020): pairs_host = the validated uint2_pair lists of
 * every image pair concatenated in the reference's pair order (0,1),(0,2)..(1,2)..; pairCounts_host[p] entries each.
 * Outputs are malloc'd (release with ssrlcv_host_free): MultiMatch{numKeyPoints,index} and the flattened members
 * {image, feature index}; KeyPoint{parentId = image, loc = features[image][feature].loc} is the caller's lookup.
 * Deterministic (the result is upstream's single-threaded walk's, computed on all host cores: csrc/host_merge.cpp), so
 * ranks that all-gathered the same pair arrays derive the same MatchSet. */
int ssrlcv_merge_matches_host(uint32_t numImages, const uint32_t* numFeatures_host, uint32_t numPairs,
                              const uint32_t* pairCounts_host, const ssrlcv_uint2_pair* pairs_host,
                              ssrlcv_multimatch** matches_out, ssrlcv_uint2** members_out, uint32_t* numMatches,
                              uint32_t* numMembers);
void ssrlcv_host_free(void* p);
/* Pair table of the sharded generateMatchesExhaustive (image pairs over the ranks of a node):
 * owners_out[p] = the rank that matches pair p (pairs in the order above), by longest-processing-time-first on the cost
 * numFeatures[i] x numFeatures[j]; deterministic, so every rank derives the same table.  Shared by ssrlcv_amd/dist.py and
 * host/Distributed.hpp. */
int ssrlcv_assign_pairs_host(uint32_t numImages, const uint32_t* numFeatures_host, uint32_t world, uint32_t* owners_out);
/* Test hook: the same merge with mode 1 = upstream's literal single-threaded walk (the default, mode 0, resolves the seeds
 * of an image that share no list in parallel and must give the same arrays: tests/test_merge_parallel.py). */
int ssrlcv_merge_matches_host_mode(uint32_t numImages, const uint32_t* numFeatures_host, uint32_t numPairs,
                                   const uint32_t* pairCounts_host, const ssrlcv_uint2_pair* pairs_host,
                                   ssrlcv_multimatch** matches_out, ssrlcv_uint2** members_out, uint32_t* numMatches,
                                   uint32_t* numMembers, int mode);

/* The same merge on the device (csrc/merge.hip): generateMatchesExhaustive's host half (src/MatchFactory.cu:943-1020)
 * without the D2H copy of the matches and the H2D copy of the members.  pairs: DEVICE array, the validated uint2_pair
 * arrays of every image pair concatenated in pair order as above (pairCounts_host entries each); numImages <= 32.
 * matches / members: DEVICE arrays with room for totalPairs MultiMatch and 2 x totalPairs members; counts: DEVICE
 * uint32[4] = {numMatches, numMembers, input status, rounds}.  The seeds of an image are resolved in rounds (a seed waits
 * while an unresolved lower seed could change what it reads, or reads what it would clear), which reproduces upstream's
 * sequential walk exactly.  ASYNCHRONOUS (round 4): everything is queued on `stream` -- the rounds are phases of one
 * persistent kernel (at most one block per CU) separated by a grid-wide barrier -- and nothing is read back; the caller reads `counts`
 * after synchronising the stream.  counts[2] != 0 reports malformed input (an index out of range, or two entries of one
 * list with the same partner image -- a query matched twice in one pair -- which only the host walk accepts); the two
 * counts are then 0 and the outputs untouched.  Bit 2 of the status word (value 4): the persistent walk found one of its
 * blocks not resident (CU masking, another persistent kernel on the device) -- its bounded grid barrier gave up instead of
 * hanging; the outputs are invalid.  Returns SSRLCV_ERR_INVALID_ARG / _WORKSPACE / _CAPACITY for what the
 * host can see (null pointers, 2..32 images, sizes). */
size_t ssrlcv_hip_merge_workspace_bytes(uint32_t numImages, const uint32_t* numFeatures_host, uint32_t totalPairs);
int ssrlcv_hip_merge_matches(uint32_t numImages, const uint32_t* numFeatures_host, uint32_t numPairs,
                             const uint32_t* pairCounts_host, const ssrlcv_uint2_pair* pairs, void* workspace,
                             size_t workspaceBytes, ssrlcv_multimatch* matches, ssrlcv_uint2* members, uint32_t* counts,
                             ssrlcv_stream_t stream);

/* ============================== S: SIFT =========================================================== */

/* --- kernel-level entry points (one per reference kernel / helper; all asynchronous) --- */

/* convertToBW / generateBW (src/Image.cu:665-690,1277-1296; called by generateFeatures for colour input,
 * src/SIFT_FeatureFactory.cu:26-29).  colorDepth 2 (grey + alpha), 3 (RGB) or 4 (RGBA) interleaved bytes -> one byte. */
int ssrlcv_hip_convert_to_bw(const uint8_t* colorPixels, uint32_t colorDepth, uint8_t* bw, size_t numPixels,
                             ssrlcv_stream_t stream);
/* convertToFltImage (src/Image.cu:1554-1559) */
int ssrlcv_hip_u8_to_f32(const uint8_t* pixels, float* out, size_t numPixels, ssrlcv_stream_t stream);
/* upsampleImage(float) (src/Image.cu:1393-1414): out is 2w x 2h */
int ssrlcv_hip_upsample2x(const float* in, uint32_t w, uint32_t h, float* out, ssrlcv_stream_t stream);
/* convertToFltImage + upsampleImage fused: reads the u8 image once */
int ssrlcv_hip_upsample2x_u8(const uint8_t* in, uint32_t w, uint32_t h, float* out, ssrlcv_stream_t stream);
/* binImage(float) (src/Image.cu:1380-1392): out is w/2 x h/2 */
int ssrlcv_hip_bin2x(const float* in, uint32_t w, uint32_t h, float* out, ssrlcv_stream_t stream);
/* Blur::Blur tap generation (src/FeatureFactory.cu:15-18,29-33): host arithmetic; returns odd tap count (<= 129) */
int ssrlcv_gauss_kernel_host(float sigma, float pixelWidth, float* weights_host);
/* convolveSeparable / convolveImage1D_symmetric x2 (src/Image.cu:1197-1239,1526-1546), fused H+V through LDS.
 * weights_host: `taps` floats (copied into the launch).  minmax (nullable, 2 floats, caller-initialised to
 * {FLT_MAX,-FLT_MAX}) accumulates the level's min/max that normalizeImage (src/Image.cu:631-649) finds on the host.
 * tmp: scratch of w*h floats (used only by the two-pass fallback for taps > 129; may be NULL otherwise). */
int ssrlcv_hip_gauss_sep_conv(const float* in, float* out, float* tmp, uint32_t w, uint32_t h, int taps,
                              const float* weights_host, float* minmax, ssrlcv_stream_t stream);
/* host min/max loop of normalizeImage (src/Image.cu:631-649) as a device reduction; minmax = {min,max} */
int ssrlcv_hip_minmax(const float* in, size_t n, float* minmax, ssrlcv_stream_t stream);
/* normalize kernel (src/Image.cu:1560-1565), in place, min/max read from device */
int ssrlcv_hip_normalize(float* data, size_t n, const float* minmax, ssrlcv_stream_t stream);
/* Octave::normalize + convertToDOG/subtractImages (src/FeatureFactory.cu:327-331,404-440,842-845) fused:
 * dog[b] = N(level[b+1]) - N(level[b]), b = 0..4, with N(x) = (x-min_b)/(max_b-min_b); levelMinMax = 6 x {min,max};
 * dogMinMax (nullable, 5 x {min,max}, caller-initialised to {FLT_MAX,-FLT_MAX}) accumulates the min/max that findKeyPoints'
 * second normalisation (src/FeatureFactory.cu:472) needs.  Pixels are moved four at a time: w * h % 4 != 0 returns
 * SSRLCV_ERR_INVALID_ARG (every level of a plan is a multiple of 4 pixels), and the levels must be 16-byte aligned. */
int ssrlcv_hip_dog_normalised_sub(const float* const levels_host[6], const float* levelMinMax, uint32_t w, uint32_t h,
                                  float* const dog_host[5], float* dogMinMax, ssrlcv_stream_t stream);

/* --- pipeline-level entry point: SIFT_FeatureFactory::generateFeatures, sparse branch
 *     (src/SIFT_FeatureFactory.cu:17-31,55-169) --- */
typedef struct {
  uint32_t maxOrientations;       /* generateFeatures argument (Pipeline.cu:25 passes 2) */
  float orientationThreshold;     /* 0.8 */
  float orientationContribWidth;  /* SIFT_FeatureFactory ctor, 1.5 */
  float descriptorContribWidth;   /* 6.0 */
  uint32_t maxKeyPointsPerOctave; /* capacity of the device key-point lists; 0 = default (pixels of the octave / 16) */
} ssrlcv_sift_params;

typedef struct ssrlcv_sift_plan ssrlcv_sift_plan; /* opaque host-side description of the workspace layout */

/* Host-only: lays out the scale space (4 octaves x 6 levels from a 2x upsample: SIFT_FeatureFactory.cu:56-64) for a
 * w x h u8 image.  Sizes that are not multiples of 8 get makeBinnable's zero border (src/Image.cu:966-995 as called from
 * src/FeatureFactory.cu:364-376: even sizes are padded to multiples of 8 before the upsample, sizes with an odd side
 * to multiples of 32 after it); feature locations are then in the padded frame, as upstream.  SSRLCV_ERR_UNSUPPORTED
 * for images below 64 pixels on a side (the reference's own 65-tap mirror indexes outside its smallest octave there:
 * undefined upstream), and for contribution widths beyond 30 (descriptor) / 5 (orientation), whose windows would
 * outgrow the sampling kernels' 16-bit window indexing.
 * A plan is `const` in the calls below but carries host-side bookkeeping of the (plan, workspace) pair it is run on
 * (which of an octave's two list buffers is current; its events): ONE extraction -- or one sequence of stage calls -- at
 * a time per plan, from one host thread.  Concurrent extractions take one plan each (plans are cheap: host memory only). */
int ssrlcv_sift_plan_create(uint32_t w, uint32_t h, const ssrlcv_sift_params* params, ssrlcv_sift_plan** plan);
void ssrlcv_sift_plan_destroy(ssrlcv_sift_plan* plan);
size_t ssrlcv_sift_plan_workspace_bytes(const ssrlcv_sift_plan* plan);
uint32_t ssrlcv_sift_plan_max_features(const ssrlcv_sift_plan* plan);

/* Stage 1: ScaleSpace constructor with makeDOG (src/FeatureFactory.cu:338-440): pyramid + DoG into the workspace. */
int ssrlcv_hip_sift_build_dog(const ssrlcv_sift_plan* plan, const uint8_t* pixels, void* workspace,
                              ssrlcv_stream_t stream);
/* Stage 2: findKeyPoints + checkKeyPoints + computeKeyPointOrientations + fillDescriptors
 * (src/FeatureFactory.cu:461-632, src/SIFT_FeatureFactory.cu:71-167).  features: capacity
 * ssrlcv_sift_plan_max_features(plan); numFeatures: one uint32 on the device. */
int ssrlcv_hip_sift_describe(const ssrlcv_sift_plan* plan, void* workspace, ssrlcv_sift_feature* features,
                             uint32_t* numFeatures, ssrlcv_stream_t stream);
/* Stage 2 one reference launch site at a time (asynchronous, all on `stream`), each on the state the previous one left in
 * `workspace` (after ssrlcv_hip_sift_build_dog, which ends with findExtrema's flags):
 *   0  searchForExtrema: fillExtrema + thrust::remove of what findExtrema flagged   (src/FeatureFactory.cu:86-159,883-890)
 *   1  removeNoise(noiseThreshold * 0.8) = flagNoise + discardExtrema               (:161-215,267-285,484,968-973)
 *   2  refineExtremaLocation = refineLocation + discard + stable_sort by blur + the host re-scan of the blur indices
 *                                                                                   (:217-265,892-967)
 *   3  removeNoise(noiseThreshold)                                                  (:267-285)
 *   4  removeEdges(edgeThreshold) = flagEdges + discard                             (:287-306,974-990)
 *   5  checkKeyPoints + discard                                                     (src/SIFT_FeatureFactory.cu:81-110,449-461)
 *   6  computeKeyPointOrientations = gradients, computeThetas, thrust::remove, expandKeyPoints   (src/FeatureFactory.cu:540-632,1004-1122)
 *   7  fillDescriptors                                                              (src/SIFT_FeatureFactory.cu:131-166,475-549)
 * Stages 0..7 in order give the features of ssrlcv_hip_sift_describe bit for bit (tests/test_gpu_sift.py); the fused call
 * folds stage 1 into 0 and 3-5 into one compaction.  *numFeatures (device) is updated by every call; `features` is only
 * written by stage 7 (may be NULL before).  The list of an octave after any stage: ssrlcv_sift_plan_keypoints. */
int ssrlcv_hip_sift_stage(const ssrlcv_sift_plan* plan, void* workspace, int stage, ssrlcv_sift_feature* features,
                          uint32_t* numFeatures, ssrlcv_stream_t stream);
/* Both stages back to back (asynchronous; read *numFeatures after synchronising the stream).  The fused call overlaps
 * the stages where the stand-alone calls cannot (they leave nothing in flight): octave 0's key-point list chain (flag
 * compaction, refinement, discards) starts on a side stream as soon as that octave's DoG pass is through, beside the smaller
 * octaves' convolutions; the key-point stage joins it.  Same results.  On an error return the caller's stream has been
 * ordered behind whatever the call had queued on its side streams.
 * ssrlcv_sift_plan_set_stage_event: `event` (a hipEvent_t, or NULL) is recorded by every later ssrlcv_hip_sift_extract on
 * this plan, on the caller's stream, between the scale-space stage (S1-S8) and the key-point stage (S9-S14) -- the hook
 * bench.py times the stages of the fused call with. */
int ssrlcv_sift_plan_set_stage_event(ssrlcv_sift_plan* plan, void* event);
int ssrlcv_hip_sift_extract(const ssrlcv_sift_plan* plan, const uint8_t* pixels, void* workspace,
                            ssrlcv_sift_feature* features, uint32_t* numFeatures, ssrlcv_stream_t stream);

/* ---- dense SIFT: SIFT_FeatureFactory::generateFeatures(image, dense = true, maxOrientations, orientationThreshold) -------
 * Key points on a regular grid of the image itself, all at one scale; no scale space.  The reference's sources are not
 * at hand here, so its dense branch is not restated line by line: the contract below is this project's own.  It keeps the
 * reference's signature and the arithmetic of the reference's kernels as the per-kernel entry points further down state
 * it; the result is DEFINED as this chain of them (pixelWidth = 1 throughout), and the kernels of csrc/dense.hip -- which
 * are not that chain -- are held to it bit for bit (tests/dense_ref.py, tests/test_gpu_dense.py), and both to the CPU
 * oracle's restatement of the items below (oracle_sift_dense, oracle/oracle_sift.c):
 *   1 level        L = ssrlcv_hip_u8_to_f32(pixels), normalised in place by ssrlcv_hip_minmax + ssrlcv_hip_normalize.  The
 *                  descriptor's fixed-point vote scale assumes gradient magnitudes <= 1.4143, which the normalisation gives.
 *                  A constant image (max == min) is outside the contract: its level is 0 / 0.
 *   2 gradients    G = ssrlcv_hip_pixel_gradients(L)
 *   3 grid         wo = ceilf(sigma * 3.0f * orientationContribWidth), wd = ceilf(sigma * descriptorContribWidth) (float
 *                  arithmetic, as the kernels compute their windows), margin = max(wo, wd).  Key points at the integer
 *                  locations x = margin + i stride <= w - 2 - margin, y = margin + j stride <= h - 2 - margin: nx x ny of
 *                  them in row-major order, y outer; each an SSKeyPoint {octave 0, blur 0, sigma, discard 0}.  With this
 *                  margin every one passes the window tests of compute_thetas and check_keypoints, and every descriptor
 *                  sample lies inside the image.
 *   4 orientations ssrlcv_hip_compute_thetas (lambda = orientationContribWidth), ssrlcv_hip_compact_thetas /
 *                  _compact_addresses, ssrlcv_hip_expand_keypoints: up to maxOrientations oriented key points per grid
 *                  point, strongest first, in grid order, then slot order.  An all-zero histogram contributes none.
 *   5 descriptors  ssrlcv_hip_fill_descriptors (lambda = descriptorContribWidth); parent = -1, as the sparse path writes it.
 *                  A descriptor whose window holds no gradient is outside the contract like the constant image: its votes
 *                  are all zero and its bytes 0 / 0, unspecified.  (Reachable with wo > wd beside a flat region: the
 *                  orientation window finds a gradient the descriptor window does not reach.)
 *   6 count        *numFeatures (device) = the full count; only the first min(count, capacity) records are written, in
 *                  order, and nothing behind features[capacity) is touched.
 * Decided on the host before any launch, the parameters before the buffers: SSRLCV_ERR_INVALID_ARG for params NULL, stride 0,
 * sigma or a width not finite and positive, maxOrientations outside 1..8, nx ny maxOrientations >= 2^31; SSRLCV_ERR_UNSUPPORTED
 * for wo > 32 or wd > 32; then SSRLCV_ERR_INVALID_ARG for a NULL buffer (features may be NULL with capacity 0);
 * SSRLCV_ERR_WORKSPACE for a short workspace.  An image too small for one grid point is no error: nx = ny = 0, count 0.
 * Workspace (ssrlcv_hip_sift_dense_workspace_bytes; 0 for parameters the call refuses): 13 bytes per pixel (L, the polar
 * table {magnitude, atan2}, the histogram bin) + 4 maxOrientations + 8 bytes per grid point (orientations, counts, offsets)
 * + the window's weight table and the scan's tile descriptors.  Asynchronous on `stream`; no host synchronisation. */
typedef struct {
  uint32_t stride;                  /* grid step in pixels, >= 1 */
  float sigma;                      /* scale of every key point, > 0 (host mirror default 1.6) */
  uint32_t maxOrientations;         /* 1..8 */
  float orientationThreshold;       /* 0.8 */
  float orientationContribWidth;    /* 1.5 */
  float descriptorContribWidth;     /* 6.0 */
} ssrlcv_dense_params;
/* host only, no device touched; margin / nx / ny may be NULL */
int ssrlcv_sift_dense_grid(uint32_t w, uint32_t h, const ssrlcv_dense_params* params, uint32_t* margin, uint32_t* nx, uint32_t* ny);
uint32_t ssrlcv_sift_dense_max_features(uint32_t w, uint32_t h, const ssrlcv_dense_params* params); /* nx ny maxOrientations */
size_t ssrlcv_hip_sift_dense_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_dense_params* params);
int ssrlcv_hip_sift_dense_u8(const uint8_t* pixels, uint32_t w, uint32_t h, const ssrlcv_dense_params* params, void* workspace,
                             size_t workspaceBytes, ssrlcv_sift_feature* features, uint32_t capacity, uint32_t* numFeatures,
                             ssrlcv_stream_t stream);

/* ---- dense stereo: the reference's Window_NxN descriptors + MatchFactory's disparity matchers + PointCloudFactory's
 * stereo_disparity, as SAD block matching of a rectified pair.  The reference's sources are not at hand here, so -- as for
 * dense SIFT -- the contract below is this project's own; the kernels of csrc/stereo.hip are held to a numpy restatement of
 * it bit for bit (tests/stereo_ref.py, tests/test_gpu_stereo.py).  Upstream materialises one window descriptor per pixel (up
 * to 961 bytes) and runs its generic matcher over them; here the kernel works from the two images directly and no cost
 * volume or per-pixel window exists in memory.
 *   inputs      left, right: uint8, w x h, row-major with pitch w, rectified: the partner of left pixel (x, y) at disparity d
 *               is right pixel (x - d, y).
 *   1 cost      C(x, y, d) = sum over |i| <= r, |j| <= r of |L(x + i, y + j) - R(x + i - d, y + j)|: an integer, at most
 *               961 * 255.  Defined only where both windows lie inside their image: r <= x <= w - 1 - r, r <= y <= h - 1 - r,
 *               r <= x - d <= w - 1 - r; elsewhere d is not a candidate of (x, y).  No border is replicated anywhere.
 *   2 winner    candidates are d = minDisparity + k, k = 0 .. numDisparities - 1.  d*(x, y) = the candidate of least cost C*,
 *               the smallest d among equal costs.  A pixel with no candidate is invalid.
 *   3 limit     C* > maxCost: the pixel is invalid (UINT32_MAX: no test).
 *   4 LR check  lrTolerance >= 0: the right winner dR(x', y) = the d of least C(x' + d, y, d) over the d for which that cost is
 *               defined, the smallest d among equal costs.  (x, y) stays valid only if |dR(x - d*, y) - d*| <= lrTolerance
 *               (dR(x - d*, y) always has at least the candidate d*).  lrTolerance < 0: no check.
 *   5 sub-pixel subpixel = 1: if d* - 1 and d* + 1 are both candidates of (x, y) and den = C(d* - 1) - 2 C* + C(d* + 1) != 0,
 *               off = (float)(C(d* - 1) - C(d* + 1)) / (float)(2 den): two integers below 2^24 converted exactly, one IEEE
 *               float division; otherwise off = 0.  disparity = (float)d* + off, one float addition.  |off| <= 0.5 since C*
 *               is the minimum.  Items 2 and 4 always use the integer winners.
 *   6 outputs   disparity[w h] float, an invalid pixel holds the bit pattern 0x7FC00000; cost[w h] uint32 (may be NULL) holds
 *               C*, UINT32_MAX for an invalid pixel.  Every pixel of both maps is written, the border included.
 * Decided on the host before any launch, the parameters before the buffers: SSRLCV_ERR_INVALID_ARG for params NULL, radius 0,
 * numDisparities 0, minDisparity outside -32768 .. 32767, subpixel > 1, w h >= 2^31; SSRLCV_ERR_UNSUPPORTED for radius > 15 or
 * numDisparities > 256; then SSRLCV_ERR_INVALID_ARG for a NULL buffer (cost may be NULL); SSRLCV_ERR_WORKSPACE for a short
 * workspace.  An image smaller than one window is no error: every pixel is invalid.
 * Workspace (ssrlcv_hip_stereo_workspace_bytes; host only; 0 for parameters the call refuses): two bytes per pixel, the
 * winners' k of the two views.  Asynchronous on `stream`; no host synchronisation; no atomics: bit-equal run to run.
 * Out of scope here: a uniqueness ratio, colour or NCC costs (census costs: the section "census cost" below).  Aggregating
 * these costs along paths is the next section, "semi-global matching".  (An unrectified pair of pinhole cameras is rectified
 * first: "rectification" below.) */
typedef struct {
  uint32_t radius;          /* r in 1..15; the window is (2r + 1)^2.  Upstream's five sizes: r = 1, 4, 7, 12, 15 */
  int32_t minDisparity;     /* -32768 .. 32767 */
  uint32_t numDisparities;  /* D in 1..256 */
  uint32_t maxCost;         /* a winner costlier than this is invalid; UINT32_MAX = no test */
  int32_t lrTolerance;      /* < 0 = no left-right check */
  uint32_t subpixel;        /* 0 or 1 */
} ssrlcv_stereo_params;
size_t ssrlcv_hip_stereo_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_stereo_params* params);
int ssrlcv_hip_stereo_sad_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params* params,
                             void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, ssrlcv_stream_t stream);
/* The valid pixels of a disparity map with x % step == 0 and y % step == 0, in raster order, as the sparse path's records:
 * Match{invalid = 0, {leftId, (x, y)}, {rightId, ((float)x - disparity, (float)y)}}, padding bytes zero -- what
 * ssrlcv_hip_matchset_from_matches and the triangulation take unchanged.  *count_dev (device) = the full count; only the first
 * min(count, capacity) records are written, in order, and nothing behind out[capacity) is touched (dense SIFT's item 6); out
 * may be NULL with capacity 0.  SSRLCV_ERR_INVALID_ARG for step 0 or w h >= 2^31, then for a NULL buffer; SSRLCV_ERR_WORKSPACE
 * below ssrlcv_hip_stereo_matches_workspace_bytes (host only; 0 for a refused step or size).  One ordered compaction
 * (csrc/compact.h); asynchronous on `stream`. */
size_t ssrlcv_hip_stereo_matches_workspace_bytes(uint32_t w, uint32_t h, uint32_t step);
int ssrlcv_hip_stereo_matches(const float* disparity, uint32_t w, uint32_t h, uint32_t step, int leftId, int rightId, ssrlcv_match* out,
                              uint32_t capacity, uint32_t* count_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
/* PointCloudFactory::stereo_disparity: per match d = kp0.x - kp1.x, Z = (foc * baseline) / (d + doffset),
 * X = ((kp0.x - cx) * Z) / foc, Y = ((kp0.y - cy) * Z) / foc, in float32 in exactly that order, nothing contracted.  An
 * invalid match, or one whose d + doffset is not above 0, gives (0, 0, 0): the value ssrlcv_hip_point_normals writes for a
 * missing result.  foc not finite or 0: SSRLCV_ERR_INVALID_ARG.  Asynchronous on `stream`. */
int ssrlcv_hip_stereo_points(const ssrlcv_match* matches, uint32_t n, float foc, float baseline, float doffset, float cx, float cy,
                             ssrlcv_float3* points, ssrlcv_stream_t stream);

/* ---- semi-global matching (Hirschmueller) over the SAD costs of dense stereo: instead of every pixel choosing its disparity
 * on its own, the clamped matching costs are aggregated along up to eight paths through the image with a small penalty for a
 * disparity step of one and a larger one for any other jump, and the winner is taken from the sum.  Integer arithmetic
 * throughout: the kernels of csrc/stereo.hip are held to a numpy restatement bit for bit (tests/sgm_ref.py,
 * tests/test_gpu_sgm.py).  The outputs are dense stereo's two maps, so ssrlcv_hip_stereo_mask_rectified, _stereo_matches,
 * _matches_apply_homography and _stereo_points take them unchanged.
 *   inputs      those of dense stereo.  C(x, y, d), "candidate" and the interior I = [r, w - 1 - r] x [r, h - 1 - r] are items
 *               1-2 of dense stereo, unchanged.  The disparity index is k = 0 .. D - 1 (D = numDisparities), d = minDisparity + k.
 *   1 cost      for p in I: M(p, k) = min(C(p, d), costClamp) if d is a candidate of p, else costClamp.  A non-candidate takes
 *               part in the recursion like any other entry; it can never be a winner.
 *   2 paths     bit i of `paths` selects direction i, (dx, dy) = 0: (+1, 0)  1: (-1, 0)  2: (0, +1)  3: (0, -1)  4: (+1, +1)
 *               5: (-1, +1)  6: (+1, -1)  7: (-1, -1).  The predecessor of p is q = p - (dx, dy).  0x0F is the usual 4-path
 *               form, 0xFF the 8-path form.
 *   3 path cost q not in I: L_i(p, k) = M(p, k).  Otherwise, with m = min over all k of L_i(q, k):
 *               L_i(p, k) = M(p, k) + min(L_i(q, k), L_i(q, k - 1) + P1 [k >= 1], L_i(q, k + 1) + P1 [k <= D - 2], m + P2) - m.
 *               Integers, 0 <= L_i <= costClamp + P2.
 *   4 sum       S(p, k) = sum over the selected i of L_i(p, k) <= popcount(paths) (costClamp + P2).
 *   5 winner    d*(p) = the candidate of least S, the smallest d among equal S.  A pixel with no candidate is invalid.  There
 *               is no cost limit.
 *   6 LR check  lrTolerance >= 0: item 4 of dense stereo with S in place of C: dR(x', y) = the d of least S(x' + d, y, d) over
 *               the d that are candidates of (x' + d, y), the smallest d on ties; (x, y) stays valid only if
 *               |dR(x - d*, y) - d*| <= lrTolerance.  The right view gets no aggregation of its own.
 *   7 sub-pixel subpixel = 1: item 5 of dense stereo with S in place of C: both neighbours candidates, den = S(d* - 1) - 2 S* +
 *               S(d* + 1) != 0, off = (float)(S(d* - 1) - S(d* + 1)) / (float)(2 den), disparity = (float)d* + off; every
 *               integer is below 2^24.
 *   8 outputs   item 6 of dense stereo: disparity[w h] float, 0x7FC00000 for an invalid pixel; cost[w h] uint32 (may be NULL)
 *               holds S*, UINT32_MAX for an invalid pixel.  Every pixel of both maps is written.
 * Decided on the host before any launch, the parameters before the buffers, in this order: SSRLCV_ERR_INVALID_ARG for params
 * NULL, radius 0, numDisparities 0, minDisparity outside -32768 .. 32767, subpixel > 1, P1 > P2, paths 0 or above 0xFF, w h >=
 * 2^31; SSRLCV_ERR_UNSUPPORTED for radius > 15, numDisparities > 256 or popcount(paths) (costClamp + P2) > 65535 (evaluated in
 * 64 bits; the bound that lets M, L and S live in 16 bits); then SSRLCV_ERR_INVALID_ARG for a NULL buffer (cost may be NULL);
 * SSRLCV_ERR_WORKSPACE for a short workspace.  An image smaller than one window is no error: every pixel is invalid.
 * Workspace (ssrlcv_hip_stereo_sgm_workspace_bytes; host only; 0 for parameters the call refuses; computed in size_t): with
 * K = numDisparities rounded up to 8, 16, 32, 64, 128 or 256 and a256(n) = n rounded up to 256,
 *     2 a256(w h) + 2 a256(2 w h K) + 256 bytes
 * -- the winners' k of the two views and the two uint16 volumes M and S, [y][x][k] (at 4096 x 4096, D = 64: 2 x 2.1 GB).
 * Asynchronous on `stream`; no host synchronisation; no atomics; no block waits for another: bit-equal run to run.
 * Out of scope: a uniqueness ratio, colour or NCC costs (census costs: the section "census cost" below), more than 8 paths,
 * penalties adapted to the image gradient. */
typedef struct {
  uint32_t radius;          /* 1..15 */
  int32_t minDisparity;     /* -32768 .. 32767 */
  uint32_t numDisparities;  /* 1..256 */
  uint32_t costClamp;       /* 0 is legal: everything ties */
  uint32_t P1, P2;          /* P1 <= P2 */
  uint32_t paths;           /* bit mask, 1..0xFF */
  int32_t lrTolerance;      /* < 0: no check */
  uint32_t subpixel;        /* 0 or 1 */
} ssrlcv_sgm_params;        /* 36 bytes */
size_t ssrlcv_hip_stereo_sgm_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_sgm_params* params);
int ssrlcv_hip_stereo_sgm_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_sgm_params* params,
                             void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost, ssrlcv_stream_t stream);
/* The hook tools/bench_sgm.py times the passes of one call with (process-wide, not thread-safe; not for production callers):
 * every later ssrlcv_hip_stereo_sgm_u8 records events[j] (hipEvent_t; a NULL entry is skipped) on its stream -- [0] before the
 * first launch, [1] behind the fill and the cost pass, then one behind each selected direction's pass in the order of the bits,
 * one behind the winner pass and one behind the left-right check (at most 12).  count 0 removes the hook; count > 12 or events
 * NULL with count > 0: SSRLCV_ERR_INVALID_ARG.  The caller keeps the events alive until it removes the hook. */
int ssrlcv_hip_stereo_sgm_set_pass_events(void* const* events, uint32_t count);

/* ---- census cost: the census transform of both views and the Hamming distance of the codes as the matching cost of dense
 * stereo and of semi-global matching, in place of the sum of absolute differences.  A code keeps only which neighbours are
 * darker than the centre, so the cost does not change under any strictly increasing map of either image's grey levels: two
 * exposures, two gains, the softening of a bilinear warp.  Integer arithmetic throughout: the kernels of csrc/stereo.hip are
 * held to a numpy restatement bit for bit (tests/census_ref.py, tests/test_gpu_census.py).
 *   parameters  c = censusRadius, 1, 2 or 3: the census window is (2c + 1)^2 and a code has n = 8, 24 or 48 bits.
 *               r = params->radius is the AGGREGATION radius in these calls, 0 .. 7; r = 0 is legal here: the cost of a pixel
 *               is its own Hamming distance, the usual form under semi-global matching.
 *               rho = r + c is the footprint radius, at most 10.
 *   1 census    for c <= x <= w - 1 - c and c <= y <= h - 1 - c: number the window's offsets (i, j), the centre skipped, as
 *               b = 0 .. n - 1 with j = -c .. c outer and i = -c .. c inner; bit b of T(x, y) is 1 iff I(x + i, y + j) < I(x, y),
 *               strictly.  T is a uint64 with bit b at 2^b and the upper bits zero.  Everywhere else the exported map holds 0;
 *               no cost ever reads those entries.
 *   2 Hamming   H(x, y, d) = popcount(T_L(x, y) xor T_R(x - d, y)).
 *   3 cost      C(x, y, d) = sum over |i| <= r, |j| <= r of H(x + i, y + j, d): an integer, at most n (2r + 1)^2 <= 10800.
 *               Defined only where rho <= x <= w - 1 - rho, rho <= y <= h - 1 - rho and rho <= x - d <= w - 1 - rho; elsewhere d
 *               is not a candidate of (x, y).  No border is replicated.
 *   4 the rest  is the existing text with this C, and rho wherever it says r: items 2-6 of "dense stereo" (the winner, the
 *               smallest d on ties, maxCost, the left-right check from the right view's winners over the same C, the sub-pixel
 *               parabola, both maps fully written) for ssrlcv_hip_stereo_census_u8; items 1-8 of "semi-global matching" with
 *               I = [rho, w - 1 - rho] x [rho, h - 1 - rho] and the bound popcount(paths) (costClamp + P2) <= 65535 unchanged for
 *               ssrlcv_hip_stereo_sgm_census_u8.  C fits 16 bits without a clamp: costClamp >= n (2r + 1)^2 cuts nothing.
 * Refusals keep the order of the SAD calls, the parameters before the buffers and invalid before unsupported:
 * SSRLCV_ERR_INVALID_ARG for params NULL, censusRadius 0 (it takes the place of radius 0, which is no error here), and every
 * other invalid parameter of the SAD call, w h >= 2^31 last; SSRLCV_ERR_UNSUPPORTED for censusRadius > 3 or radius > 7 (in
 * place of radius > 15), numDisparities > 256 and the 16-bit bound; then SSRLCV_ERR_INVALID_ARG for a NULL buffer (cost may be
 * NULL) and SSRLCV_ERR_WORKSPACE for a short workspace.  An image smaller than the footprint is no error: every pixel is
 * invalid.
 * Workspace (host only; 0 for parameters the call refuses; computed in size_t): the SAD call's layout plus the code maps of
 * the two views, uint64 [h][w] each:
 *     block matching         2 a256(w h) + 256 + 2 a256(8 w h) bytes
 *     semi-global matching   2 a256(w h) + 2 a256(2 w h K) + 256 + 2 a256(8 w h) bytes
 * The caller's workspace pointer is at least 8-byte aligned (any device allocation is).  Asynchronous on `stream`; no host
 * synchronisation; no atomics; no block waits for another: bit-equal run to run.
 * ssrlcv_hip_census_u8 is the per-kernel export of item 1: it writes every entry of codes[w h].  SSRLCV_ERR_INVALID_ARG for
 * censusRadius 0 or w h >= 2^31, SSRLCV_ERR_UNSUPPORTED for censusRadius > 3, then SSRLCV_ERR_INVALID_ARG for a NULL buffer.
 * The pass-events hook of ssrlcv_hip_stereo_sgm_set_pass_events applies to ssrlcv_hip_stereo_sgm_census_u8 with the same
 * marks; the two census passes count into mark [1], "behind the fill and the cost pass".
 * Still out of scope: census windows that are not square (9 x 7), the centre-symmetric and the ternary census, colour, NCC
 * costs, a uniqueness ratio. */
int ssrlcv_hip_census_u8(const uint8_t* image, uint32_t w, uint32_t h, uint32_t censusRadius, uint64_t* codes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_stereo_census_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_stereo_params* params, uint32_t censusRadius);
int ssrlcv_hip_stereo_census_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_stereo_params* params,
                                uint32_t censusRadius, void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost,
                                ssrlcv_stream_t stream);
size_t ssrlcv_hip_stereo_sgm_census_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_sgm_params* params, uint32_t censusRadius);
int ssrlcv_hip_stereo_sgm_census_u8(const uint8_t* left, const uint8_t* right, uint32_t w, uint32_t h, const ssrlcv_sgm_params* params,
                                    uint32_t censusRadius, void* workspace, size_t workspaceBytes, float* disparity, uint32_t* cost,
                                    ssrlcv_stream_t stream);

/* ---- rectification: a converging pair of Image::Camera records -> two homographies -> a rectified pair for the dense stereo
 * above, and its matches back in source pixels, where they triangulate with the original cameras into the sparse path's world
 * frame.  Like dense stereo the contract is this project's own; the kernels of csrc/rectify.hip are held to a numpy restatement
 * of it bit for bit (tests/rectify_ref.py, tests/test_gpu_rectify.py).
 *
 * Evaluating a homography.  H is 9 floats, row-major.  At a float point (x, y), in float32, every product and sum rounded on
 * its own, nothing contracted:
 *     X = (H0 x + H1 y) + H2      Y = (H3 x + H4 y) + H5      W = (H6 x + H7 y) + H8
 *     sx = X / W, sy = Y / W      two IEEE divisions
 * The point is MAPPED if W > 0 and sx, sy are finite.  It is INSIDE a sw x sh source if it is mapped and 0 <= sx <= sw - 1 and
 * 0 <= sy <= sh - 1.
 *
 * ssrlcv_hip_warp_homography_u8: dst(x, y) = src sampled bilinearly at H (x, y).  H is a HOST pointer; its 9 values travel as
 * kernel arguments.  Both images are uint8 with pitch = width.  For every output pixel (x, y), converted exactly to float:
 *   not mapped  the byte is 0.
 *   otherwise   sx is clamped to [0, srcW - 1] and sy to [0, srcH - 1];
 *               x0 = min((int)floor(sx), max(srcW - 2, 0)), x1 = min(x0 + 1, srcW - 1), fx = sx - (float)x0 (exact); y0, y1, fy
 *               the same from sy and srcH;
 *               a, b, c, d = S(x0, y0), S(x1, y0), S(x0, y1), S(x1, y1) as floats;
 *               top = a + fx (b - a), bot = c + fx (d - c), v = top + fy (bot - top): every operation rounded, no fma;
 *               the byte is (uint8)floor(v + 0.5f).  v stays in [0, 255] (each step lies between its two end values).
 * Every output pixel is written and nothing behind dst[dstW dstH); the border is replicated, never read outside; the source is
 * never written.  Decided on the host before any launch, the parameters before the buffers: SSRLCV_ERR_INVALID_ARG for H NULL,
 * a source side 0, any side above 2^24, or w h >= 2^31 of either image; a dst of 0 pixels is then SSRLCV_OK (nothing to do);
 * then SSRLCV_ERR_INVALID_ARG for a NULL buffer.  Asynchronous on `stream`, no workspace, no atomics, bit-equal run to run.
 *
 * ssrlcv_hip_stereo_mask_rectified: in place on the maps ssrlcv_hip_stereo_sad_u8 wrote for a pair warped by Hl, Hr (host
 * pointers) from srcW x srcH sources.  A pixel (x, y) whose disparity delta is not the invalid pattern stays valid only if
 *   the four points (x +- r, y +- r) are inside the left source under Hl, and
 *   the four points (xr +- (r + 0.5), y +- r), xr = (float)x - delta (one float subtraction, then one float addition or
 *   subtraction of the exact r + 0.5), are inside the right source under Hr
 * (the box is half a pixel wider than the integer winner's window because |delta - d*| <= 0.5).  Otherwise disparity <-
 * 0x7FC00000, and cost <- UINT32_MAX if a cost map is given.  The corners suffice: a homography maps lines to lines, so the
 * pre-image of the source rectangle (in the half plane W > 0) is convex, and a box whose four corners lie in a convex set lies
 * in it.  What the call does not do: the left-right check ran before it, over costs that include replicated border, so the mask
 * only removes pixels; it never rescues one.  SSRLCV_ERR_INVALID_ARG for Hl or Hr NULL, a source side 0, any side above 2^24,
 * w h >= 2^31 of the map or the source, radius outside 1..15; a map of 0 pixels is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG
 * for disparity NULL (cost may be NULL).  Asynchronous on `stream`.
 *
 * ssrlcv_hip_matches_apply_homography: in place.  For each record with invalid == 0, keyPoints[k].loc <- (sx, sy) under Hk (host
 * pointers; a NULL Hk leaves that side alone).  If either side is not mapped the record keeps both locations as they were and
 * gets invalid = 1.  Parent ids and padding bytes are untouched.  n == 0 is SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for matches
 * NULL.  With Hl, Hr of a rectification it turns ssrlcv_hip_stereo_matches' records into matches in source pixels.
 *
 * ssrlcv_rectify_cameras_host: host only, double precision, no device touched -- the one definition both binders call.
 *   1  per camera, the focal length in pixels f = foc / dpix with dpix = foc tan(fov.x / 2) / (size.x / 2), the value
 *      generateBundle recomputes (the stored dpix is ignored);
 *   2  R_i = Rz Ry Rx of cam_rot (rotatePoint's convention), double sin / cos of the float angles;
 *   3  b = pos_r - pos_l, xh = b / |b|; yh = normalise((z_l + z_r) x xh), z_i the third column of R_i; zh = xh x yh;
 *   4  the Euler angles of [xh yh zh]: y = -asin(clamp(M20)), x = atan2(M21, M22), z = atan2(M10, M00), rounded to float32 and
 *      stored as cam_rot; R_n is rebuilt from the ROUNDED angles and everything below uses that R_n;
 *   5  with a_i = R_n^T z_i: tl = rint(f_l a_l.x / a_l.z), tr = rint(f_l a_r.x / a_r.z),
 *      ty = rint(f_l (a_l.y / a_l.z + a_r.y / a_r.z) / 2)   (rint: to nearest, ties to even);
 *   6  with K(f) = [[f, 0, w/2], [0, f, h/2], [0, 0, 1]] and T(t) = [[1, 0, t], [0, 1, ty], [0, 0, 1]]:
 *      H_i = K(f_i) R_i^T R_n K(f_l)^-1 T(t_i), divided by its last entry; G_i its inverse, normalised the same way; all four
 *      rounded to float32.  H_i takes a rectified pixel to its source pixel (what the warp and the mask evaluate), G_i back;
 *   7  w, h = the left camera's size; foc = f_l, baseline = |b|, doffset = tl - tr, cx = w/2 - tl, cy = h/2 - ty: exactly
 *      ssrlcv_hip_stereo_points' parameters, so Z = foc baseline / (d + doffset) holds for the rectified pair, and both old
 *      image centres land on the rectified centre: the content overlaps at disparities near 0, whatever the convergence.
 * Refusals, in this order: SSRLCV_ERR_INVALID_ARG for a NULL; for sizes that differ or have a zero side; for foc or fov.x not
 * finite and positive; for |b| = 0; for xh . (first column of R_l) <= 0 (the caller has the cameras the wrong way round);
 * SSRLCV_ERR_UNSUPPORTED when (z_l + z_r) x xh vanishes (norm below 1e-6: float32 angles resolve no less); when a_l.z or a_r.z is below cos 45 deg; when a last
 * entry to divide by is not positive.  `out` is untouched on any error.
 *
 * Out of scope: rectifying from a fundamental matrix alone (Hartley) -- the device entry points take any homography, so it can
 * come later without touching a kernel; pushbroom cameras; lens distortion; interpolation other than bilinear; colour. */
typedef struct {
  float Hl[9], Hr[9];       /* rectified pixel -> source pixel, left and right */
  float Gl[9], Gr[9];       /* source pixel -> rectified pixel */
  uint32_t w, h;            /* size of the rectified images */
  float foc, baseline, doffset, cx, cy;  /* ssrlcv_hip_stereo_points' parameters of the rectified pair */
  float cam_rot[3];         /* Euler angles of the rectified frame R_n */
} ssrlcv_rectification;
int ssrlcv_rectify_cameras_host(const ssrlcv_camera* left, const ssrlcv_camera* right, ssrlcv_rectification* out);
int ssrlcv_hip_warp_homography_u8(const uint8_t* src, uint32_t srcW, uint32_t srcH, const float* H_host, uint8_t* dst, uint32_t dstW,
                                  uint32_t dstH, ssrlcv_stream_t stream);
int ssrlcv_hip_stereo_mask_rectified(float* disparity, uint32_t* cost, uint32_t w, uint32_t h, uint32_t radius, const float* Hl_host,
                                     const float* Hr_host, uint32_t srcW, uint32_t srcH, ssrlcv_stream_t stream);
int ssrlcv_hip_matches_apply_homography(ssrlcv_match* matches, uint32_t n, const float* H0_host, const float* H1_host,
                                        ssrlcv_stream_t stream);

/* ---- disparity post-filters: the last stage of the dense stereo chain looks at the winner map as an image.  The left-right
 * check, maxCost and the rectification mask judge one pixel at a time; what survives them are small islands of wrong disparity
 * along occlusion edges and in repeated texture, and single-pixel spikes.  The speckle filter invalidates the connected regions
 * of similar disparity that are too small to be a surface; the median filter (Hirschmueller's step behind semi-global matching)
 * removes the spikes.  Both work on the maps of every call above: float[w h], pitch w, and uint32 cost[w h].  The contract is
 * this project's own; the kernels of csrc/disparity_filter.hip are held to a numpy restatement of it bit for bit
 * (tests/speckle_ref.py, tests/test_gpu_speckle.py).
 *   validity    as everywhere in this file: a pixel is valid iff its bit pattern is not 0x7FC00000.  Any other value, other
 *               NaNs and the infinities included, is a valid pixel and follows the items below as written.
 *   1 links     two valid pixels that are 4-adjacent, (x +- 1, y) or (x, y +- 1), are linked iff fabsf(d(p) - d(q)) <= maxDiff:
 *               one IEEE float subtraction and a comparison that is false for a NaN (a NaN pixel links to nothing; inf - inf is
 *               a NaN).  Symmetric, because a - b = -(b - a) exactly.  No link across an invalid pixel, none diagonally.
 *   2 components  the connected components of the graph (valid pixels, links): the transitive closure.  A ramp that rises by
 *               maxDiff per pixel is ONE component, however far its ends are apart.  label(p) = the smallest raster index
 *               y w + x in p's component; size(p) = the number of pixels of p's component; an invalid pixel has label
 *               UINT32_MAX and size 0.  w h < 2^31, so both fit.
 *   3 speckles  in place: a valid pixel with size(p) <= maxSpeckleSize becomes invalid: its disparity becomes 0x7FC00000 and,
 *               if a cost map is given, its cost UINT32_MAX; nothing else is written.  maxSpeckleSize = 0 removes nothing and is
 *               legal.  The filter only removes pixels, and whole components at that, so no survivor's component changes: the
 *               filter is idempotent (twice with the same parameters equals once).
 *   4 median    out of place, m = radius = 1 or 2.  An invalid input pixel gives an invalid output pixel: holes are never
 *               filled.  For a valid pixel take the valid pixels of the (2m + 1)^2 window clipped to the image -- the pixel
 *               itself is among them, so there are n >= 1 -- ordered by the integer key k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF, b the
 *               bits as int32: the float order, made total, with -0 below +0.  The output is the element of rank (n - 1) / 2
 *               (integer division): the LOWER median.  It is always one of the input values: no arithmetic, no tolerance.
 *               The cost map is NOT touched by the median: it goes on describing the winner of the matching call, which
 *               the output pixel may no longer be.
 * Refusals, decided on the host before any launch, the parameters before the buffers, invalid before unsupported:
 *   components, speckles   SSRLCV_ERR_INVALID_ARG for maxDiff a NaN or negative (+inf is legal: every adjacent valid pair whose
 *               difference is no NaN links), then for w h >= 2^31; a map of 0 pixels is then SSRLCV_OK; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL disparity, labels or workspace (cost and sizes may be NULL); then
 *               SSRLCV_ERR_WORKSPACE for a short workspace.
 *   median      SSRLCV_ERR_INVALID_ARG for radius 0 or w h >= 2^31; SSRLCV_ERR_UNSUPPORTED for radius > 2; a map of 0 pixels
 *               is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL buffer or in == out.  No workspace.
 * Workspace (host only; 0 for a size the call refuses; computed in size_t), with a256(n) = n rounded up to 256:
 *     components     a256(4 w h) bytes        the tile-local component counts (needed whether sizes is given or not)
 *     speckles       2 a256(4 w h) bytes      the labels and those counts: 8 bytes per pixel, 128 MB at 4096 x 4096
 * The workspace may hold anything on entry: every entry the call reads it has written before.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another (no grid barrier, no spin: the
 * labelling is union-find in three passes -- tiles in LDS, tile seams, tile roots -- and none is repeated until nothing changes,
 * so a serpentine through every tile costs what a blob costs).  These are the first calls of the stereo chain with atomics,
 * integer ones: atomicMin on labels and atomicAdd on counts.  The result is bit-equal run to run all the same, because it is
 * a property of the component and not of the order in which unions happen: a parent is always a smaller index of the same
 * component, so whatever the order of the hooks the root of a finished tree is the component's smallest index; a size is a
 * sum of integers, which has one value in every order.  (A float atomic would not have that property; there is none.)
 * ssrlcv_hip_disparity_components is the per-kernel export of items 1-2: it writes every entry of labels[w h] and, if given,
 * of sizes[w h].
 * Out of scope: filling the holes (the next section, "hole filling"), 8-connectivity, a weighted or bilateral median, radius 3 and
 * above, a uniqueness ratio, the right view's map. */
size_t ssrlcv_hip_disparity_components_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_disparity_components(const float* disparity, uint32_t w, uint32_t h, float maxDiff, uint32_t* labels,
                                    uint32_t* sizes /* may be NULL */, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_stereo_filter_speckles_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_stereo_filter_speckles(float* disparity, uint32_t* cost /* may be NULL */, uint32_t w, uint32_t h, float maxDiff,
                                      uint32_t maxSpeckleSize, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_hip_stereo_filter_median(const float* in, float* out, uint32_t w, uint32_t h, uint32_t radius, ssrlcv_stream_t stream);

/* ---- hole filling: every stage behind the winner only removes pixels -- the left-right check, maxCost, the rectification mask
 * and the speckle filter each punch holes -- and this call closes them: a hole takes one of the measured disparities that lie
 * nearest to it along up to eight directions (Hirschmueller's step behind the peak filter).  Selection only, no arithmetic on
 * disparities: the kernels of csrc/disparity_filter.hip are held to a numpy restatement bit for bit (tests/fill_ref.py,
 * tests/test_gpu_fill.py).  Maps as in "disparity post-filters": float[w h], pitch w.
 *   validity    as everywhere in this file: a pixel is valid iff its bit pattern is not 0x7FC00000; other NaNs, the infinities
 *               and -0 are valid values.  A valid pixel of `in` is MEASURED, every other pixel is a HOLE.
 *   1 sources   bit i of `paths` selects direction i, with the (dx, dy) of "semi-global matching" item 2; direction i carries
 *               values along (dx, dy): for a hole p, hit_i(p) is the first measured pixel among p - t (dx, dy), t = 1, 2, ...,
 *               while that point is inside the image and t <= maxGap.  If the ray leaves the image or passes maxGap first, the
 *               hole has no hit in that direction.  maxGap = 0 fills nothing; UINT32_MAX is no limit.  Only `in` is looked at: a
 *               filled value is never a source, so the result does not depend on any order of evaluation.  A second call on
 *               the output may therefore fill more: the filter is NOT idempotent.
 *   2 count     n = the number of selected directions with a hit.  If n < minHits the hole stays a hole.
 *   3 value     the n hit values ordered by the integer key of the median filter ("disparity post-filters" item 4),
 *               k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF: rule 0 (MIN) takes rank 0, the smallest disparity -- the background, which
 *               is what an occlusion hides; rule 1 (MEDIAN) takes rank (n - 1) / 2, the lower median.  The output is always one
 *               of the input values: no arithmetic, no tolerance.
 *   4 outputs   out of place; every pixel of `out` and, if given, of `filled` is written and nothing behind either map.
 *               out(p) = the bits of in(p) for a measured pixel; for a hole the value of item 3, or 0x7FC00000.  filled(p) = 1
 *               for a hole that got a value, 0 everywhere else.  No cost map is touched: a filled pixel keeps the UINT32_MAX
 *               its matching call wrote, so a caller who holds a cost map can tell measured from filled by that.
 * Refusals, decided on the host before any launch, the parameters before the buffers, invalid before anything else:
 * SSRLCV_ERR_INVALID_ARG for params NULL, paths 0 or above 0xFF, minHits 0 or above popcount(paths), rule > 1, then w h >= 2^31;
 * a map of 0 pixels is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for `in`, `out` or workspace NULL, or in == out (filled may
 * be NULL); then SSRLCV_ERR_WORKSPACE for a short workspace.
 * Workspace (host only; computed in size_t; 0 for a refused parameter or size and for an empty map):
 *     popcount(paths) a256(4 w h) bytes        one hit map per selected direction
 * It may hold anything on entry: a pass stores hit_i(p) at the holes only, the invalid pattern where there is none -- the
 * natural "no hit" entry, because no measured value has it -- and the maps are read at the holes only.
 * Execution: asynchronous on `stream`; no host synchronisation; no atomics; no block waits for another: bit-equal run to run.
 * Until its pixels are written, `out` is the call's scratch for the carries that one strip of a column or diagonal hands to the
 * next.  The work per pixel and direction is O(1) whatever the gap: a carry of (last measured value, steps since it) along every row,
 * column and diagonal, never a ray walk; no loop depends on the extent of a hole or on maxGap.
 * Out of scope: interpolation that computes new values (linear, plane fits), telling occlusions from mismatches by the right
 * view's map, sources weighted by distance, more than 8 directions. */
typedef struct {
  uint32_t paths;   /* bit mask 1..0xFF, the direction numbering of semi-global matching */
  uint32_t maxGap;  /* a source further than this many steps away does not count; 0 fills nothing; UINT32_MAX = no limit */
  uint32_t minHits; /* 1 .. popcount(paths): a hole with fewer sources stays a hole */
  uint32_t rule;    /* 0 = MIN (background), 1 = MEDIAN (lower) */
} ssrlcv_fill_params; /* 16 bytes */
size_t ssrlcv_hip_stereo_fill_holes_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_fill_params* params);
int ssrlcv_hip_stereo_fill_holes(const float* in, float* out, uint8_t* filled /* may be NULL */, uint32_t w, uint32_t h,
                                 const ssrlcv_fill_params* params, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- disparity mesh: a disparity map is an organised cloud -- every point knows its neighbours -- so a triangle mesh and
 * normals need no k-NN and no viewpoint heuristic: the sampling grid gives the connectivity, a disparity jump marks a depth
 * edge, the vertex numbering is ssrlcv_hip_stereo_matches' (the faces index the clouds made from its records) and the face
 * winding orients the normals.  Everything is a selection or a fixed-order float32 expression: the kernels of csrc/mesh.hip
 * are held to a numpy restatement bit for bit (tests/mesh_ref.py, tests/test_gpu_mesh.py).
 *   grid        the nodes are the pixels with x % step == 0 and y % step == 0: gw = (w - 1) / step + 1 columns and gh =
 *               (h - 1) / step + 1 rows of them (0 for w or h 0), the grid of ssrlcv_hip_stereo_matches; node (i, j) is pixel
 *               (i step, j step) and d(i, j) its disparity.  Maps over nodes are row-major with pitch gw.
 *   validity    as everywhere in this file: a node is valid iff its disparity's bit pattern is not 0x7FC00000; other NaNs, the
 *               infinities and -0 are valid values.
 *   1 vertices  vertexIndex[gw gh] (uint32): a valid node holds its rank among the valid nodes in raster order -- the index of
 *               its record in ssrlcv_hip_stereo_matches' output for the same map and step -- and an invalid node UINT32_MAX
 *               (until the map is restricted: item 6).  *vertexCount_dev (device) = the number of valid nodes.
 *   2 joined    nodes p and q are joined iff both are valid and fabsf(d(p) - d(q)) <= maxJump: one IEEE float subtraction and
 *               a comparison that is false for a NaN ("disparity post-filters" item 1), so a NaN difference is not joined,
 *               inf - inf among them.  maxJump = +inf is legal.
 *   3 cells     cell (i, j), 0 <= i < gw - 1, 0 <= j < gh - 1, has the corners a = (i, j), b = (i + 1, j), c = (i, j + 1),
 *               d = (i + 1, j + 1).  With fewer than three valid corners the cell is empty.  With four valid corners its
 *               diagonal is b-c iff fabsf(d(b) - d(c)) < fabsf(d(a) - d(d)), otherwise a-d (ties and comparisons with a NaN
 *               included); with three, the diagonal between valid corners.  Diagonal a-d gives T0 = (a, c, d) and
 *               T1 = (a, d, b); diagonal b-c gives T0 = (a, c, b) and T1 = (b, c, d).  A triangle is emitted iff its three
 *               edges are joined.  cells[(gw - 1) (gh - 1)] (uint8, pitch gw - 1): bit 0 = T0 emitted, bit 1 = T1 emitted,
 *               bit 2 = the diagonal is b-c; the byte is 0 whenever neither triangle is emitted, so its values are 0, 1, 2, 3,
 *               5, 6, 7.  All four triangles wind the same way: with image x to the right and y down, in a camera frame with
 *               X right, Y down and Z forward (ssrlcv_hip_stereo_points') (q - p) x (r - p) of a triangle (p, q, r) has
 *               negative z: the normals face the camera.
 *   4 triangles ssrlcv_hip_mesh_triangles writes the emitted triangles as three uint32 vertex indices (vertexIndex of p, q, r)
 *               each, in cell raster order, T0 before T1.  *count_dev (device) = the full count; only the first
 *               min(count, capacity) triangles are written and nothing behind out[3 capacity) is touched; out may be NULL
 *               with capacity 0 (the truncation contract of ssrlcv_hip_stereo_matches).
 *   5 normals   ssrlcv_hip_mesh_normals: points[n] are the vertices' positions, e.g. ssrlcv_hip_stereo_points' of the records.
 *               For every node with index v < n: s = (+0, +0, +0); visit the cells (i - 1, j - 1), (i, j - 1), (i - 1, j),
 *               (i, j), in that order, where they exist, and in each T0, then T1 -- the triangle list's order; for every
 *               emitted triangle (p, q, r) that contains the node and whose three indices are all < n, with P = points,
 *               u = P[q] - P[p], v = P[r] - P[p]:
 *                 t = ((u.y v.z) - (u.z v.y), (u.z v.x) - (u.x v.z), (u.x v.y) - (u.y v.x)),   s = s + t
 *               in float32, nothing contracted.  Then len = sqrtf(((s.x s.x) + (s.y s.y)) + (s.z s.z)) and normals[v] = s / len
 *               component by component, sqrt and division correctly rounded; if len is 0 or not finite, normals[v] =
 *               (0, 0, 0), the "no result" value of ssrlcv_hip_point_normals, which a vertex without a triangle gets too.
 *               Only normals[v] of the nodes with v < n are written: an index >= n contributes nothing and writes nothing, so
 *               a map that is stale for `points` is never read or written out of bounds.
 *   6 select    ssrlcv_hip_mesh_select restricts a mesh, in place, to a subset of its vertices: keptIndex[m] holds old vertex
 *               indices, strictly ascending; old vertex keptIndex[j] becomes j and every other node UINT32_MAX (an index
 *               >= nVertices in the map included).  An entry >= nVertices is ignored.  A triangle with a removed corner has
 *               its bit cleared, a byte left without a triangle becomes 0; nothing is re-triangulated.  Two producers of
 *               keptIndex exist: the `index` output of ssrlcv_hip_neighbor_distance_filter, and the records that survive
 *               ssrlcv_hip_matches_apply_homography plus ssrlcv_hip_compact_matches: the mesh follows its cloud through both.
 * Refusals of ssrlcv_hip_disparity_mesh, decided on the host before any launch, the parameters before the buffers:
 * SSRLCV_ERR_INVALID_ARG for params NULL, step 0, maxJump negative or a NaN (!(maxJump >= 0)), then for w h >= 2^31, then for a
 * NULL vertexCount_dev; an empty map (w or h 0) then writes count 0, looks at nothing else and is SSRLCV_OK; then
 * SSRLCV_ERR_INVALID_ARG for a NULL disparity, vertexIndex or workspace, or a NULL cells that has an element (it has none when gw
 * or gh is below 2); then SSRLCV_ERR_WORKSPACE for a short workspace.  The other calls: SSRLCV_ERR_INVALID_ARG for gw gh >=
 * 2^31, then for a NULL buffer that has an element to hold (count_dev always; out unless capacity is 0; keptIndex unless m is
 * 0; the workspace unless the query gives 0), then SSRLCV_ERR_WORKSPACE.  Where there is nothing to do the call is SSRLCV_OK
 * before any other buffer is looked at: mesh_triangles on a grid without a cell writes count 0 and needs count_dev alone;
 * mesh_normals with n 0, and mesh_normals and mesh_select on a grid without a node, write nothing.
 * Workspace (host only; computed in size_t; 0 for refused input), with a256(n) = n rounded up to 256 and
 * c(N) = a256(4 (4 ceil(N / 4096) + 3)), the tables of one ordered compaction of N elements (csrc/compact.h):
 *     disparity_mesh   c(gw gh)                       mesh_select   a256(4 nVertices), the old -> new vertex table
 *     mesh_triangles   c(2 (gw - 1) (gh - 1)), c(0) when gw or gh is below 2
 * It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no atomics; no block waits for another: bit-equal run to run.
 * Out of scope: vertex welding or decimation (a height map's mesh is thinned by "surface simplification"), closing holes in the mesh, triangle-quality tests in 3-D (a sliver between a
 * near and a far surface is cut by maxJump alone), texture coordinates, Poisson or any other reconstruction from unorganised
 * clouds, merging the meshes of several pairs. */
typedef struct {
  uint32_t step;  /* >= 1: the sampling step of ssrlcv_hip_stereo_matches */
  float maxJump;  /* >= 0, +inf allowed: two nodes whose disparities differ by more are not joined */
} ssrlcv_mesh_params; /* 8 bytes */
size_t ssrlcv_hip_disparity_mesh_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_mesh_params* params);
int ssrlcv_hip_disparity_mesh(const float* disparity, uint32_t w, uint32_t h, const ssrlcv_mesh_params* params, uint32_t* vertexIndex,
                              uint8_t* cells, uint32_t* vertexCount_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_mesh_select_workspace_bytes(uint32_t nVertices);
int ssrlcv_hip_mesh_select(uint32_t* vertexIndex, uint8_t* cells, uint32_t gw, uint32_t gh, uint32_t nVertices, const uint32_t* keptIndex,
                           uint32_t m, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_mesh_triangles_workspace_bytes(uint32_t gw, uint32_t gh);
int ssrlcv_hip_mesh_triangles(const uint32_t* vertexIndex, const uint8_t* cells, uint32_t gw, uint32_t gh, uint32_t* out, uint32_t capacity,
                              uint32_t* count_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_hip_mesh_normals(const ssrlcv_float3* points, uint32_t n, const uint32_t* vertexIndex, const uint8_t* cells, uint32_t gw, uint32_t gh,
                            float* normals, ssrlcv_stream_t stream);
/* The meshes of several pairs are merged through the next section: their clouds into one height map, and that map's mesh. */

/* ---- surface model: a height map on a ground grid, fused over every pair that sees a cell.  The map has the form of a
 * disparity map -- float[w h], pitch w, invalid = 0x7FC00000 -- so ssrlcv_hip_stereo_filter_median, _filter_speckles,
 * _fill_holes and ssrlcv_hip_disparity_mesh take it unchanged: merging the meshes of several pairs is rasterising each pair's
 * world-frame cloud into the same grid, fusing per cell, and meshing the result.  Everything is a selection or a fixed-order
 * float32 expression, nothing contracted, the one division IEEE: the kernels of csrc/dsm.hip are held to a numpy restatement
 * bit for bit (tests/dsm_ref.py, tests/test_gpu_dsm.py).
 *   frame       ssrlcv_dsm_frame: cell (i, j) of the w x h grid covers origin + a ex + b ey, i cell <= a < (i + 1) cell,
 *               j cell <= b < (j + 1) cell; ez is the direction heights are measured along.  It is an affine map and is NOT
 *               checked for orthonormality.  Refused: a non-finite entry of origin, ex, ey or ez; a cell that is not finite or
 *               not above 0.
 *   validity    as everywhere in this file: a cell is valid iff its height's bit pattern is not 0x7FC00000.
 *   key         k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF of the bits b as an int32, the key of the median filter ("disparity
 *               post-filters" item 4): a total order in which -0 lies below +0.
 *   1 rasterize ssrlcv_hip_dsm_rasterize.  A point is skipped if any component is not finite, or if it is (0, 0, 0) with
 *               either sign of zero, this file's "no result" point.  Otherwise, for point p of index t, in float32 in exactly
 *               this order:
 *                 q = p - origin  (component by component)
 *                 a = ((q.x ex.x) + (q.y ex.y)) + (q.z ex.z),   b the same with ey,   z the same with ez
 *                 u = a / cell,  v = b / cell,  fi = floorf(u),  fj = floorf(v)
 *               The point lies in cell (i, j) = (fi, fj) iff fi >= 0 && fi < (float)w && fj >= 0 && fj < (float)h, compared
 *               on floats before any conversion: a NaN and a huge value are outside, -0 is inside cell 0, u == w is outside.
 *               A point whose z is not finite is skipped.  rule 0 = MAX (the top surface), 1 = MIN:
 *                 height(i, j) = the z of greatest (least) key among the cell's points
 *                 source(i, j) = that point's index; among points of equal key the smallest index
 *                 count(i, j)  = the number of points in the cell
 *               An empty cell holds 0x7FC00000, UINT32_MAX and 0.  Every entry of every given map is written and nothing
 *               behind it; source and count may be NULL.
 *   2 fuse      ssrlcv_hip_dsm_fuse: `maps` is a HOST array of m device pointers, 1 <= m <= 8, each a w x h map.  Per cell:
 *               the valid entries among the m maps, n of them, ordered by key.  If n < minViews the cell is invalid.  If
 *               !(hi - lo <= maxSpread) -- one float subtraction of the largest and the smallest entry; maxSpread = +inf is
 *               legal, a NaN difference (inf - inf) fails -- the cell is invalid.  Otherwise out takes rank 0 (rule 0, MIN),
 *               rank (n - 1) / 2 (rule 1, the lower MEDIAN) or rank n - 1 (rule 2, MAX): always one of the inputs.  views
 *               (uint8, may be NULL) holds n, whether or not the cell survives.  The same map may be passed twice.
 *   3 points    ssrlcv_hip_dsm_points writes the valid cells in raster order -- the numbering ssrlcv_hip_disparity_mesh gives
 *               the same map at step 1 (its item 1) -- each as, in float32, z its height:
 *                 a = ((float)i + 0.5f) cell,   b = ((float)j + 0.5f) cell
 *                 P = ((origin + a ex) + b ey) + z ez      (component by component, in that order)
 *               *count_dev (device) = the full count; only the first min(count, capacity) points are written and nothing
 *               behind out[capacity) is touched; out may be NULL with capacity 0 (the truncation contract of
 *               ssrlcv_hip_stereo_matches).
 *   winding     with (ex, ey, -ez) right-handed -- x east, y south, height up: the image convention with the camera above --
 *               the faces of ssrlcv_hip_disparity_mesh on the height map wind so that ssrlcv_hip_mesh_normals' normals of
 *               these points face +ez.
 * Refusals, decided on the host before any launch, the parameters before the sizes before the buffers:
 *   rasterize   SSRLCV_ERR_INVALID_ARG for a NULL or refused frame, rule > 1, w h >= 2^31, n = UINT32_MAX; then
 *               SSRLCV_ERR_UNSUPPORTED for w or h above 2^24, where (float)w stops being exact; an empty grid (w or h 0) is
 *               then SSRLCV_OK and nothing is looked at; then SSRLCV_ERR_INVALID_ARG for a NULL height or workspace, or a NULL
 *               points unless n is 0 (the maps are then all empty cells); then SSRLCV_ERR_WORKSPACE.
 *   fuse        SSRLCV_ERR_INVALID_ARG for m 0 or above 8, minViews 0 or above m, maxSpread negative or a NaN
 *               (!(maxSpread >= 0)), rule > 2, then w h >= 2^31; an empty map is then SSRLCV_OK; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL maps, maps[i] or out, or out equal to any input.
 *   points      SSRLCV_ERR_INVALID_ARG for a NULL or refused frame or w h >= 2^31; SSRLCV_ERR_UNSUPPORTED for w or h above
 *               2^24; SSRLCV_ERR_INVALID_ARG for a NULL count_dev; an empty grid then writes count 0 and is SSRLCV_OK; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL height or workspace, or a NULL out unless capacity is 0; then
 *               SSRLCV_ERR_WORKSPACE.
 * Workspace (host only; computed in size_t; 0 for a refused size), a256 and c as in "disparity mesh":
 *     dsm_rasterize   a256(8 w h), one 64-bit accumulator per cell        dsm_points   c(w h)        dsm_fuse   none
 * It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  dsm_rasterize uses global INTEGER
 * atomics only -- a 64-bit max on (key << 32) | (0xFFFFFFFF - index), the key complemented for MIN, and a 32-bit add for the
 * count, at most one of each per point: adjacent lanes of a wave that fall into one cell share theirs -- which commute: the maps
 * do not depend on the order the points arrive in and are bit-equal run to run.
 * dsm_fuse and dsm_points use no atomics.
 * Out of scope: a mean or any float accumulation per cell; a ground frame fitted to the cloud; pushbroom pairs; more than 8
 * maps.  The picture on the surface is the next section, "ortho-image". */
typedef struct {
  float origin[3];  /* the world position of the corner of cell (0, 0) */
  float ex[3];      /* the direction of growing i */
  float ey[3];      /* the direction of growing j */
  float ez[3];      /* the direction heights are measured along */
  float cell;       /* > 0 and finite: the side of a cell */
  uint32_t w, h;    /* the grid */
} ssrlcv_dsm_frame; /* 60 bytes */
size_t ssrlcv_hip_dsm_rasterize_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_rasterize(const ssrlcv_float3* points, uint32_t n, const ssrlcv_dsm_frame* frame, uint32_t rule, float* height,
                             uint32_t* source /* may be NULL */, uint32_t* count /* may be NULL */, void* workspace, size_t workspaceBytes,
                             ssrlcv_stream_t stream);
int ssrlcv_hip_dsm_fuse(const float* const* maps, uint32_t m, uint32_t w, uint32_t h, uint32_t minViews, float maxSpread, uint32_t rule,
                        float* out, uint8_t* views /* may be NULL */, ssrlcv_stream_t stream);
size_t ssrlcv_hip_dsm_points_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_points(const float* height, const ssrlcv_dsm_frame* frame, ssrlcv_float3* out, uint32_t capacity, uint32_t* count_dev,
                          void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- ortho-image: the grey of every valid cell of a height map -- the fused, filled map of "surface model", cells that the fill
 * or the median created included -- taken from up to 8 source images, each view tested for occlusion by a march over the height
 * map towards its camera.  The heights and this raster are co-registered: cell for cell the same grid.  Everything is float32,
 * every product, sum and division rounded on its own, nothing contracted: csrc/ortho.hip is held to a numpy restatement byte for
 * byte (tests/ortho_ref.py, tests/test_gpu_ortho.py).
 *   view        ssrlcv_ortho_view, made by ssrlcv_dsm_ortho_view_host from an Image::Camera record and the frame (host only, in
 *               double, no device): f = foc / dpix with dpix = foc tan(fov.x / 2) / (size.x / 2) (step 1 of "rectification"'s
 *               builder, NOT the stored dpix); R = Rz Ry Rx of cam_rot from double sin / cos of the float angles;
 *               K = [[f, 0, size.x / 2], [0, f, size.y / 2], [0, 0, 1]]; M = K R^T; pos = cam_pos, where generateBundle's rays
 *               start (ecef_offset is not added: ssrlcv_projection_matrix_host is another frame); eye = ((q . ex) / cell,
 *               (q . ey) / cell, q . ez) with q = pos - origin; all rounded to float32 at the end; w, h = size; `image` is left as
 *               it was.  SSRLCV_ERR_INVALID_ARG for a NULL, a refused frame (the rules of "surface model"), a zero side, foc or
 *               fov.x not finite and positive, or a field of view at a pole of tan; `out` is untouched on error.
 *   per cell    (i, j) of the w x h map, z its height.  If z is 0x7FC00000 or not finite: ortho = 0, seen = 0, which = 0xFF.
 *               Otherwise, for every view k in the given order:
 *     position    a = ((float)i + 0.5f) cell, b = ((float)j + 0.5f) cell, P = ((origin + a ex) + b ey) + z ez: item 3 of "surface
 *                 model", so a vertex of ssrlcv_hip_dsm_points and its colour are the same point.
 *     projection  d = P - pos; X = (M0 d.x + M1 d.y) + M2 d.z, Y with M3..5, W with M6..8; sx = X / W, sy = Y / W.  The view can
 *                 see the cell only if W > 0, sx and sy are finite, 0 <= sx <= w_k - 1 and 0 <= sy <= h_k - 1 (MAPPED and INSIDE
 *                 of "rectification").
 *     visibility  in grid coordinates: ci = (float)i + 0.5f, cj = (float)j + 0.5f; du = eye0 - ci, dv = eye1 - cj, dz = eye2 - z.
 *                 !(dz > 0): not seen (a camera at or below the cell).  L = max(|du|, |dv|); L < 1 or maxSteps == 0: visible.
 *                 Otherwise su = du / L, sv = dv / L, sz = dz / L and for s = 1 .. maxSteps, fs = (float)s:
 *                   fs > L: visible (the march has passed the camera)
 *                   u = ci + fs su, v = cj + fs sv, zr = z + fs sz (one product and one sum each); fi = floorf(u), fj = floorf(v)
 *                   !(fi >= 0 && fi < (float)w && fj >= 0 && fj < (float)h), on floats as in rasterize: visible
 *                   hh = height(fi, fj); if its pattern is not 0x7FC00000 and hh > zr + bias: OCCLUDED (+inf occludes, another
 *                   NaN never does)
 *                 Out of steps: visible.  The march is exact geometry for an orthonormal frame (pipeline.dsm_frame makes one);
 *                 for a skew frame it is still the defined result.  bias >= 0 (+inf is legal) absorbs the staircase of a
 *                 sampled slope.
 *     sample      the bilinear expression of ssrlcv_hip_warp_homography_u8 at (sx, sy), word for word (csrc/bilinear_u8.h).
 *   choice      among the views that see the cell, n of them: rule 0 FIRST, the first in the given order (the caller lists the
 *               best view first); rule 1 MEDIAN, the lower median of their bytes, rank (n - 1) / 2.  seen: bit k = view k sees
 *               the cell.  which: the smallest k among the seeing views that has the chosen byte, 0xFF when n = 0.  ortho = 0
 *               when n = 0.
 * Every entry of every given output is written and nothing behind it; seen and which may be NULL; inputs are never written;
 * views_host is a HOST array, copied into the launch.
 * Refusals, decided on the host before any launch, the parameters before the sizes before the buffers: SSRLCV_ERR_INVALID_ARG
 * for a NULL or refused frame, a NULL params or views_host, m 0 or above 8, rule > 1, !(bias >= 0), a view with a zero side, a
 * side above 2^24, w h >= 2^31 or a non-finite entry of M, pos or eye, then a grid with w h >= 2^31; then SSRLCV_ERR_UNSUPPORTED
 * for a grid side above 2^24; an empty grid is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL height, ortho, view image or
 * workspace; then SSRLCV_ERR_WORKSPACE.
 * Workspace (host only; 0 for a refused size or m): a256(4), the greatest height's order key.  It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no float atomics -- one integer atomicMax a wave for the greatest
 * height that is not a NaN, which lets a march stop, visible, once zr + bias has reached it (zr never decreases with s): the
 * outputs do not depend on it and are bit-equal run to run.
 * Out of scope, not built: colour images; a mean or blend of views; seam smoothing; pushbroom views; sampling other than
 * bilinear; more than 8 views. */
typedef struct {
  const uint8_t* image; /* DEVICE pointer, uint8, pitch = w */
  uint32_t w, h;        /* the source image */
  float M[9];           /* row-major K R^T: world direction from the camera -> homogeneous pixel */
  float pos[3];         /* the camera's position in the clouds' world frame */
  float eye[3];         /* the camera in grid coordinates: (a / cell, b / cell, height) */
} ssrlcv_ortho_view; /* 80 bytes */
typedef struct {
  uint32_t maxSteps; /* the march's length in cells of the dominant axis; 0 = no occlusion test */
  float bias;        /* >= 0: how far a height must stand above the line of sight to hide the cell */
  uint32_t rule;     /* 0 FIRST, 1 MEDIAN */
} ssrlcv_ortho_params;
int ssrlcv_dsm_ortho_view_host(const ssrlcv_camera* cam, const ssrlcv_dsm_frame* frame, ssrlcv_ortho_view* out); /* host only */
size_t ssrlcv_hip_dsm_ortho_workspace_bytes(uint32_t w, uint32_t h, uint32_t m);
int ssrlcv_hip_dsm_ortho(const float* height, const ssrlcv_dsm_frame* frame, const ssrlcv_ortho_view* views_host, uint32_t m,
                         const ssrlcv_ortho_params* params, uint8_t* ortho, uint8_t* seen /* may be NULL */, uint8_t* which /* may be NULL */,
                         void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- surface accuracy: how far a cloud lies from a reference surface, and exact robust statistics of such differences --
 * MeshFactory's calculatePerPointDifference / calculateAverageDifference upstream.  The reference is a height map in a frame of
 * "surface model", triangulated by "disparity mesh": one definition of the surface, the mesh's.  Everything is a selection or a
 * fixed-order expression, nothing contracted: csrc/accuracy.hip is held to a numpy restatement bit for bit
 * (tests/accuracy_ref.py, tests/test_gpu_accuracy.py).
 *   1 difference ssrlcv_hip_dsm_difference: `height` is the reference map of `frame` (float[w h], pitch w, invalid = 0x7FC00000).
 *               Per point of index t, in float32: the skip rules and q, a, b, z, u, v of "surface model" item 1, word for word.  A
 *               skipped point, or one whose z is not finite, gives 0x7FC00000.  Then
 *     CELL        (cells NULL): fi = floorf(u), fj = floorf(v); inside iff fi >= 0 && fi < (float)w && fj >= 0 && fj < (float)h, on
 *                 floats as in rasterize; r = height(fi, fj); an r that is 0x7FC00000 or not finite, or a point outside, gives
 *                 0x7FC00000; otherwise diff = z - r.
 *     MESH        (cells given): `cells` is what ssrlcv_hip_disparity_mesh wrote for the same map at step 1 (its item 3: bit 0 / 1 =
 *                 T0 / T1 emitted, bit 2 = the diagonal is b-c; its maxJump cuts are in it), pitch w - 1.  The mesh's vertices sit
 *                 at cell centres: uu = u - 0.5f, vv = v - 0.5f, fi = floorf(uu), fj = floorf(vv); inside iff fi >= 0 &&
 *                 fi < (float)(w - 1) && fj >= 0 && fj < (float)(h - 1) -- a grid with w or h below 2 has no inside, and a point
 *                 within half a cell of the border is inside in CELL mode and outside here.  s = uu - fi, t = vv - fj; the corners
 *                 a, b, c, d of cell (fi, fj) as in "disparity mesh" item 3, za .. zd their heights:
 *                   diagonal a-d   T0 iff t >= s:      r = za + ((t (zc - za)) + (s (zd - zc)))
 *                                  otherwise T1:       r = za + ((s (zb - za)) + (t (zd - zb)))
 *                   diagonal b-c   T0 iff s + t <= 1:  r = za + ((s (zb - za)) + (t (zc - za)))
 *                                  otherwise T1:       r = zd + (((1 - s) (zc - zd)) + ((1 - t) (zb - zd)))
 *                 A triangle whose bit is clear gives 0x7FC00000, and so does an r that is not finite; otherwise diff = z - r:
 *                 positive means above the reference along ez.  Only the corners of the chosen triangle are read.
 *               Every entry of diff[n] is written and nothing behind it; inputs are never written.
 *   2 stats     ssrlcv_hip_difference_stats over values[n], e.g. item 1's output:
 *     validity    an entry is valid iff its bits are not 0x7FC00000; `valid` counts them.
 *     value       a valid entry x becomes y = x - center, one float subtraction, and with absolute = 1 fabsf of that.
 *     selection   only entries whose y is finite take part: `finite` = m of them.
 *     min, max    the y of least and greatest key ("surface model" key: -0 below +0); 0x7FC00000 when m is 0.
 *     quantile    params.quantile[k], k < numQuantiles, is in parts per 10000; result slot k holds the y of rank
 *                 (uint64)q (m - 1) / 10000 in key order: exact, always one of the inputs; 5000 is the lower median, 0 the min,
 *                 10000 the max.  Slots k >= numQuantiles, and every slot when m is 0, hold 0x7FC00000; the parameter's entries
 *                 k >= numQuantiles are not looked at.
 *     sum, sumSq  float64 sums of (double)y and (double)y (double)y (the square is exact) in a fixed shape: tiles of 4096
 *                 consecutive entries, excluded and padding entries adding +0.0; lane l of 256 adds entries l + 256 r, r = 0 .. 15,
 *                 in that order, starting from +0.0; the 256 lane sums fold by acc[l] += acc[l + half] for l < half, half = 128,
 *                 64, .., 1; the tile sums are reduced by the same shape again until one is left.  The mean and the RMS are the
 *                 binders' business, in host float64.
 *     record      ssrlcv_diff_stats in DEVICE memory: n, valid, finite, reserved = 0, sum, sumSq, min, max, quantile[8].  The
 *                 empty record (n = 0): zeros, +0.0 sums, 0x7FC00000 in min, max and every slot.
 * Refusals, decided on the host before any launch, in this order:
 *   difference  SSRLCV_ERR_INVALID_ARG for a NULL or refused frame (the rules of "surface model"), then w h >= 2^31; then
 *               SSRLCV_ERR_UNSUPPORTED for w or h above 2^24; n = 0 is then SSRLCV_OK and nothing is looked at; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL points, height or diff.  An empty grid is legal: no point is inside it.
 *   stats       SSRLCV_ERR_INVALID_ARG for a NULL params; numQuantiles > 8, a used quantile above 10000, a center that is not
 *               finite, absolute > 1; then a NULL out_dev; n = 0 then writes the empty record and is SSRLCV_OK; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL values or workspace; then SSRLCV_ERR_WORKSPACE.
 * Workspace of stats (host only; computed in size_t; 0 for refused params), a256 as in "disparity mesh", T(n) = ceil(n / 4096):
 *     256 + 196608 + a256(16 T(n)) + a256(16 T(T(n)))
 *   the control words, 3 passes x 8 histograms x 2048 bins x 4 bytes, and the partial sums of two levels.  It may hold anything on
 *   entry.  The difference needs none.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  The difference uses no atomics.  The
 * quantiles are a radix select over the keys, digits of 11, 11 and 10 bits from the top: histograms by INTEGER atomics (LDS, then global; the
 * lanes of a wave that share the first lane's digit add once), a one-block step a pass that narrows every quantile's prefix and
 * rank, all quantiles in the same passes, equal prefixes sharing a histogram.  Counts, min and max are integer atomics, one a
 * block.  Integer atomics commute and the sums have a fixed shape: the record is bit-equal run to run and to the restatement.
 * Out of scope, not built: differences along a direction other than the frame's ez; ray casts against unorganised meshes;
 * float atomics; weighted statistics.  Registration -- a cloud that lies off in x / y shows every slope of the
 * terrain as height error -- is the next section, "surface registration"; a cloud that lies many cells off goes through the
 * section behind it, "shift search", first. */
typedef struct {
  float center;          /* finite: subtracted from every valid entry */
  uint32_t absolute;     /* 0 or 1: fabsf of the difference to center */
  uint32_t numQuantiles; /* 0 .. 8 */
  uint32_t quantile[8];  /* parts per 10000, 0 .. 10000 */
} ssrlcv_diff_stats_params; /* 44 bytes */
typedef struct {
  uint32_t n, valid, finite, reserved;
  double sum, sumSq;
  float min, max;
  float quantile[8];
} ssrlcv_diff_stats; /* 72 bytes */
int ssrlcv_hip_dsm_difference(const ssrlcv_float3* points, uint32_t n, const float* height, const ssrlcv_dsm_frame* frame,
                              const uint8_t* cells /* may be NULL */, float* diff, ssrlcv_stream_t stream);
size_t ssrlcv_hip_difference_stats_workspace_bytes(uint32_t n, const ssrlcv_diff_stats_params* params);
int ssrlcv_hip_difference_stats(const float* values, uint32_t n, const ssrlcv_diff_stats_params* params, ssrlcv_diff_stats* out_dev,
                                void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- surface registration: the point-to-plane alignment of a cloud to the reference surface of "surface accuracy" -- what
 * PointCloudFactory's scalePointCloud / translatePointCloud / rotatePointCloud do by hand upstream before
 * calculateAverageDifference.  One GPU call accumulates the normal equations of a Gauss-Newton step over seven unknowns --
 * translation, rotation, scale --, two host calls solve and compose the step, one GPU call applies a pose to a cloud; the binders
 * iterate.  Fixed-order float32 per point, nothing contracted, the divisions and the square root IEEE; products that are exact in
 * float64; float64 sums in the fixed shape of "surface accuracy"; integer atomics only: csrc/register.hip is held to a numpy
 * restatement bit for bit (tests/register_ref.py, tests/test_gpu_register.py).
 *   pose        ssrlcv_register_pose: p' = M p + T, m the 3 x 4 matrix [M | T] row-major; pivot: the point steps rotate and scale
 *               about.  The pivot only conditions the system: it changes no p'.
 *   1 terms     ssrlcv_hip_register_terms.  The reference is MESH mode only: `cells` is required, the bytes of
 *               ssrlcv_hip_disparity_mesh of `height` at step 1 with its maxJump cuts.  Per point p of index t, in float32 in
 *               exactly this order:
 *     skip        p is skipped by the rasterize rule ("surface model" item 1): a component that is not finite, or (0, 0, 0) with
 *                 either sign of zero.
 *     pose        for the rows r = 0, 1, 2:  p'.r = (((m[4r] p.x) + (m[4r+1] p.y)) + (m[4r+2] p.z)) + m[4r+3]
 *     lookup      p' goes through "surface accuracy" item 1, MESH, word for word, its own skip rules included (csrc/mesh_lookup.h
 *                 is the one definition of both): d, or no difference.  `inside` counts the points that have a d.
 *     slopes      of the chosen triangle in s and t, from the corner heights MESH mode read:
 *                   diagonal a-d   T0: rs = zd - zc, rt = zc - za        T1: rs = zb - za, rt = zd - zb
 *                   diagonal b-c   T0: rs = zb - za, rt = zc - za        T1: rs = zd - zc, rt = zd - zb
 *                 gu = rs / cell, gv = rt / cell.
 *     gradient    of d in world coordinates, for any affine frame:  G.k = (ez.k - (gu ex.k)) - (gv ey.k),
 *                 len = sqrtf(((G.x G.x) + (G.y G.y)) + (G.z G.z)),  N = G / len component by component,  e = d / len.
 *     row         L = p' - pivot;  J0..2 = N;  J3..5 = L x N as (L.y N.z) - (L.z N.y), (L.z N.x) - (L.x N.z),
 *                 (L.x N.y) - (L.y N.x);  J6 = ((L.x N.x) + (L.y N.y)) + (L.z N.z).
 *     used        iff d exists, fabsf(d - center) <= gate (one subtraction; false for a NaN) and J0..6 and e are all finite.
 *                 `used` counts these points.
 *     sums        over the used points, of exact float64 products: jtj = sum (double)Ji (double)Jj for rows i = 0..6 and within
 *                 a row j = i..6; jte = sum (double)Ji (double)e; ee = sum (double)e (double)e.  Unused and padding entries add
 *                 +0.0.  Each of the 36 sums has the shape of `sum` in "surface accuracy": tiles of 4096, lane l of 256 adds
 *                 entries l + 256 r, r = 0 .. 15, in that order from +0.0, the lanes fold by acc[l] += acc[l + half], half = 128
 *                 .. 1, and the tile sums are reduced by the same shape again until one is left.
 *     record      ssrlcv_register_terms in DEVICE memory: n, inside, used, reserved = 0, jtj[28], jte[7], ee.  The empty record
 *                 (n = 0): zeros and +0.0 sums.
 *   2 transform ssrlcv_hip_transform_points: out[t] = p' by the row expression of item 1; a point skipped by item 1's rule is
 *               copied bit for bit, so the "no result" point stays one.  out == points is legal.  Every entry of out[n] is
 *               written and nothing behind it.
 *   3 step      ssrlcv_register_step_host (host only, in double, no device): dofMask bits 0..6 = tx, ty, tz, rx, ry, rz, scale.
 *               H = jtj with H_ii <- H_ii (1 + lambda); H delta = -jte over the masked unknowns by Cholesky in its root-free form
 *               L D L^T (one masked unknown is one division); the unmasked entries of delta[7] are 0.  SSRLCV_ERR_UNSUPPORTED,
 *               not a wrong answer, when used = 0, when a pivot D_k is not above 2^-30 times the diagonal entry H_kk it started
 *               as, or when the solution is not finite.  SSRLCV_ERR_INVALID_ARG for a NULL, a mask of 0 or above 0x7F, a lambda
 *               that is negative or not finite.  delta is untouched on error.
 *   4 compose   ssrlcv_register_compose_host (host only, in double): the step is
 *                 p'' = pivot + (1 + ds) R(dw) (p' - pivot) + dt
 *               with R the exact rotation of the rotation vector dw (Rodrigues; below |dw| = 2^-26 the limits 1 and 1/2 of its two
 *               coefficients), so M <- (1 + ds) R M and T <- pivot + (1 + ds) R (T - pivot) + dt, computed in double and rounded
 *               once to float; the pivot is carried over.  out may be pose.  SSRLCV_ERR_INVALID_ARG for a NULL, a refused pose or
 *               a delta that is not finite; SSRLCV_ERR_UNSUPPORTED if an entry of the result is not a finite float; `out` is
 *               untouched on error.
 * Refusals of the device calls, decided on the host before any launch, the parameters before the sizes before the buffers:
 *   terms       SSRLCV_ERR_INVALID_ARG for a NULL or refused frame (the rules of "surface model") or w h >= 2^31; then for a
 *               NULL pose or params, an entry of m or pivot that is not finite, a center that is not finite, a gate that is
 *               negative or a NaN (+inf is legal); then SSRLCV_ERR_UNSUPPORTED for w or h above 2^24; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL out_dev; n = 0 then writes the empty record and is SSRLCV_OK; then
 *               SSRLCV_ERR_INVALID_ARG for a NULL points, height, cells or workspace; then SSRLCV_ERR_WORKSPACE.  A grid with a
 *               side below 2 is legal: no point is inside.
 *   transform   SSRLCV_ERR_INVALID_ARG for a NULL or refused pose; n = 0 is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a
 *               NULL points or out, or an out that overlaps points without being equal to it.
 * Workspace of terms (host only; computed in size_t), a256 as in "disparity mesh", T(n) = ceil(n / 4096):
 *     a256(288 T(n)) + a256(288 T(T(n)))
 *   the 36 partial sums of two levels.  It may hold anything on entry.  The transform needs none.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  The counts are INTEGER atomics, one
 * a block; the sums have a fixed shape; there are no float atomics: the record is bit-equal run to run and to the restatement.
 * The transform uses no atomics.
 * Out of scope, not built: robust weights other than the gate; cloud-to-cloud ICP; pushbroom geometry; re-running stereo.  The
 * steps converge from about a cell off: the initial pose of a cloud that lies further off comes from the next section, "shift
 * search". */
typedef struct {
  float m[12];    /* [M | T], 3 x 4 row-major: p' = M p + T */
  float pivot[3]; /* the point steps rotate and scale about */
} ssrlcv_register_pose; /* 60 bytes */
typedef struct {
  float center; /* finite: a point is used iff fabsf(d - center) <= gate */
  float gate;   /* >= 0; +inf: every point that has a difference */
} ssrlcv_register_params; /* 8 bytes */
typedef struct {
  uint32_t n, inside, used, reserved;
  double jtj[28]; /* rows i = 0..6, within a row j = i..6 */
  double jte[7];
  double ee;
} ssrlcv_register_terms; /* 304 bytes */
size_t ssrlcv_hip_register_terms_workspace_bytes(uint32_t n);
int ssrlcv_hip_register_terms(const ssrlcv_float3* points, uint32_t n, const ssrlcv_register_pose* pose, const float* height,
                              const ssrlcv_dsm_frame* frame, const uint8_t* cells, const ssrlcv_register_params* params,
                              ssrlcv_register_terms* out_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_hip_transform_points(const ssrlcv_float3* points, uint32_t n, const ssrlcv_register_pose* pose, ssrlcv_float3* out,
                                ssrlcv_stream_t stream);
int ssrlcv_register_step_host(const ssrlcv_register_terms* record, uint32_t dofMask, double lambda, double* delta /* [7] */); /* host only */
int ssrlcv_register_compose_host(const ssrlcv_register_pose* pose, const double* delta /* [7] */, ssrlcv_register_pose* out); /* host only */

/* ---- shift search: the whole-cell shift between two height maps of one grid, over every shift of a window at once -- what
 * translatePointCloud by hand does upstream before calculateAverageDifference, and what stands between "a cloud somewhere near
 * the reference" and the point-to-plane steps of "surface registration", which follow the wrong slopes from tens of cells off.
 * One GPU call fills a table with the count, the sum and the sum of squares of the height differences of every shift; one host
 * call picks the shift of least variance, which an unknown height bias does not move.  Everything is an int32 or int64
 * expression, apart from one float multiplication and one rintf a cell, so the table does not depend on the order of summation:
 * csrc/shift.hip is held to a numpy restatement byte for byte (tests/shift_ref.py, tests/test_gpu_shift.py).
 *   maps        moving[w h] and reference[w h]: float32 height maps of one grid, pitch w; a cell that is any NaN is invalid (the
 *               maps here use 0x7FC00000).  The moving map is what ssrlcv_hip_dsm_rasterize makes of the subject cloud in the
 *               reference's frame.  Neither is written.
 *   quantise    a cell of height x becomes t = x * scale, one float32 multiplication; it is valid iff fabsf(t) <= 65536.0f, which is
 *               false for a NaN; then q = (int32)rintf(t), ties to even.  A cell whose x is finite and that fails the test is
 *               CLIPPED: it counts as invalid and is counted once per map.
 *   sampling    with stride g only the cells (i g, j g) exist, i < ceil(w / g), j < ceil(h / g): the search at stride g is, by
 *               definition, the search at stride 1 on the two maps sampled that way, and every shift, centre and count below is
 *               in sampled cells.
 *   shifts      kx, ky = -S .. S, S = radius; the shift is (sx, sy) = (centerX + kx, centerY + ky); its entry has the index
 *               (ky + S) (2S + 1) + (kx + S).
 *   entry       over all sampled cells (x, y) where moving is valid, (x + sx, y + sy) lies inside the sampled grid and reference is
 *               valid there: d = qm(x, y) - qr(x + sx, y + sy), which takes part iff |d - centerQ| <= gateQ; gateQ = UINT32_MAX
 *               means no test.  ssrlcv_shift_entry: n (uint32), reserved = 0, sum = the sum of d (int64), sumSq = the sum of d d
 *               (uint64).  A shift with no such cell holds zeros.
 *   head        ssrlcv_shift_table: validMoving, validReference, clippedMoving, clippedReference, over the sampled cells.
 *   table       in DEVICE memory: the 16-byte head, then (2S + 1)^2 entries of 24 bytes; ssrlcv_shift_table_bytes gives the size
 *               (0 for a radius above 32).  Every byte of it is written, reserved words as 0, and nothing behind it.
 *   limits      S = 0 .. 32; g >= 1; |centerX|, |centerY| <= 2^24; |centerQ| <= 2^18; scale finite and > 0; at most 2^28 sampled
 *               cells, so that sumSq <= 2^34 2^28 fits.  No index wraps for any legal centre: a shift that leaves the grid
 *               altogether has an entry of zeros.
 *   pick        ssrlcv_shift_pick_host (host only, in double, no device) reads a HOST copy of the table.
 *     candidates  the entries with n >= max(minOverlap, 1).
 *     score       mean = (double)sum / (double)n;  v = (double)sumSq / (double)n - mean * mean;  every operation rounded on its own,
 *                 nothing contracted.
 *     best        the smallest v; ties go to the smaller kx^2 + ky^2, then to the smaller ky, then to the smaller kx.
 *     step        per axis, from v at the two neighbours of the best shift along it: both must be candidates inside the table,
 *                 else the step is 0.  den = (vminus - v0) + (vplus - v0); if den > 0 the step is 0.5 (vminus - vplus) / den,
 *                 clamped to -0.5 .. 0.5; else 0.
 *     record      ssrlcv_shift_result: shiftX, shiftY = g (center + k), in cells of the full grid (int64); subX, subY = the
 *                 step times (double)g; bias = mean / (double)scale; variance = v / s2 with s2 = (double)scale (double)scale;
 *                 second = the smallest v / s2 among the candidates outside the 3 x 3 around the best, +inf if there is none;
 *                 n of the best entry; candidates = how many there were.
 *     refusals    SSRLCV_ERR_INVALID_ARG for a NULL, refused params or a tableBytes that is not the size of the params' radius; then
 *                 SSRLCV_ERR_UNSUPPORTED when there is no candidate.  `out` is untouched on error.
 *   sign        a best shift s says that moving(x) shows what reference(x + s) shows: the cloud has to move by +s cells along
 *               ex, ey and by -bias along ez.
 * Refusals of the device call, decided on the host before any launch, the parameters before the sizes before the buffers:
 * SSRLCV_ERR_INVALID_ARG for a NULL params, a scale that is not finite and > 0, stride 0, radius > 32, |centerX| or |centerY|
 * > 2^24, |centerQ| > 2^18; then SSRLCV_ERR_UNSUPPORTED for w or h above 2^24 or more than 2^28 sampled cells; then
 * SSRLCV_ERR_INVALID_ARG for a table that is NULL or not 8-byte aligned; an empty grid (w h = 0) then writes the all-zero table
 * and is SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL moving, reference or workspace; then SSRLCV_ERR_WORKSPACE.
 * Workspace (host only; computed in size_t; 0 for refused params, a refused size or an empty grid), a256 as in "disparity mesh":
 *     2 a256(4 ceil(w / g) ceil(h / g))
 *   the int32 keys of both sampled maps, INT32_MIN for an invalid cell.  It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  A quantise pass, a thread a sampled
 * cell of both maps, writes the keys, so the stride is gone before the search; the head counts are INTEGER atomics, one a wave
 * and counter at most.  In the search pass lanes own shifts, not cells: a block stages a 64 x 16 tile of moving keys and the
 * reference tile with a halo of S cells in LDS, walks the tile's cells -- the moving key is one LDS word for the whole wave, and
 * an invalid one skips the cell for the whole wave -- and every lane keeps n, sum and sumSq of its shifts in registers: no
 * cross-lane reduction anywhere.  The grid is capped, blocks stride over the tiles, and each (block, shift) is flushed once by
 * 64-bit INTEGER atomics.  Integer atomics commute and there are no float atomics: the table is bit-equal run to run and to the
 * restatement.
 * Out of scope, not built: rotation or scale in the search; a sub-cell search by resampling (the step above is a parabola through
 * three scores); scores other than the variance (correlation coefficients, truncated costs); an FFT form; radii above 32 (use
 * strides); searching against the reference's mesh instead of its cells; pushbroom geometry. */
typedef struct {
  float scale;      /* finite, > 0: quanta a height unit */
  uint32_t stride;  /* g >= 1 */
  int32_t centerX;  /* in sampled cells, |centerX| <= 2^24 */
  int32_t centerY;
  uint32_t radius;  /* S = 0 .. 32 */
  int32_t centerQ;  /* in quanta, |centerQ| <= 2^18 */
  uint32_t gateQ;   /* in quanta; UINT32_MAX: no test */
} ssrlcv_shift_params; /* 28 bytes */
typedef struct {
  uint32_t n, reserved;
  int64_t sum;
  uint64_t sumSq;
} ssrlcv_shift_entry; /* 24 bytes */
typedef struct {
  uint32_t validMoving, validReference, clippedMoving, clippedReference;
} ssrlcv_shift_table; /* 16 bytes: the head; (2 radius + 1)^2 ssrlcv_shift_entry follow it */
typedef struct {
  int64_t shiftX, shiftY; /* the best shift in cells of the full grid */
  double subX, subY;      /* the sub-cell step, in cells of the full grid */
  double bias, variance, second;
  uint32_t n, candidates;
} ssrlcv_shift_result; /* 64 bytes */
size_t ssrlcv_shift_table_bytes(uint32_t radius); /* host only */
size_t ssrlcv_hip_shift_search_workspace_bytes(uint32_t w, uint32_t h, const ssrlcv_shift_params* params);
int ssrlcv_hip_shift_search(const float* moving, const float* reference, uint32_t w, uint32_t h, const ssrlcv_shift_params* params,
                            ssrlcv_shift_table* table, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_shift_pick_host(const ssrlcv_shift_table* table_host, size_t tableBytes, const ssrlcv_shift_params* params, uint32_t minOverlap,
                           ssrlcv_shift_result* out); /* host only */

/* ---- mesh render: the grid mesh drawn into a pinhole view -- a z-buffered rasterisation that gives the depth map of the model in
 * that view, the triangle under every pixel, and the vertices' greys carried into the image.  Compared with the view's own
 * pixels (item 2) it is an accuracy measure that needs no reference surface: a wrong height shifts the texture, a wrong camera
 * shifts all of it, and a view held out of the ortho-image is an independent check.  Everything is a selection, an int32
 * expression or a fixed-order float32 expression, every product, sum and division rounded on its own, nothing contracted:
 * csrc/render.hip is held to a numpy restatement byte for byte (tests/render_ref.py, tests/test_gpu_render.py).
 *   inputs      a grid mesh as ssrlcv_hip_disparity_mesh leaves it (vertexIndex[gw gh], cells[(gw - 1) (gh - 1)], after
 *               ssrlcv_hip_mesh_select too); points[n] the vertices' world positions, e.g. ssrlcv_hip_dsm_points'; grey[n] (uint8 a
 *               vertex, e.g. the ortho-image's bytes of the valid cells; NULL: every grey counts as 0); one ssrlcv_ortho_view on the
 *               HOST, of which M, pos, w and h are read -- `image` and `eye` are ignored.
 *   1 render    ssrlcv_hip_mesh_render.
 *     vertex      for vertex t, in float32, the projection of "ortho-image" word for word: d = P - pos; X = (M0 d.x + M1 d.y) +
 *                 M2 d.z, Y with M3..5, W with M6..8; sx = X / W, sy = Y / W; iw = 1.0f / W.  The vertex is USABLE iff P's
 *                 components are finite, W > 0, W <= 2^60, sx and sy are finite, fabsf(sx) <= 1048576 and fabsf(sy) <= 1048576,
 *                 and iw is finite (a W so small that 1 / W overflows is as unusable as one that is not above 0).  Its position
 *                 in 1/256 pixel is fx = (int32)rintf(sx * 256.0f), fy likewise (ties to even); pixel (x, y) has its centre at
 *                 (256 x, 256 y), the sampling convention of the ortho-image: sx = x is the centre of pixel x.
 *     triangle    every emitted triangle of `cells` (bit 0 / 1 = T0 / T1, bit 2 = the diagonal is b-c), corners (p, q, r) in the
 *                 order of "disparity mesh" item 3; its id is 2 cellIndex + t, cellIndex = cj (gw - 1) + ci.  With
 *                 E(a, b; c) = (b.x - a.x) (c.y - a.y) - (b.y - a.y) (c.x - a.x) in int32 over (fx, fy), in this order:
 *                   a corner whose vertexIndex entry is not below n (UINT32_MAX, or stale for `points`: nothing is read or
 *                   written out of bounds, as in mesh_normals), or whose vertex is not usable: skipped, counts[2]
 *                   a bounding box wider or higher than 256 maxExtent (max - min > 256 maxExtent): skipped, counts[1]; with the
 *                   box inside that bound every edge value below is under 2^29 in magnitude
 *                   A = E(p, q; r) = 0: skipped, counts[2]
 *                   x0 = max(ceil(minx / 256), 0), x1 = min(floor(maxx / 256), w - 1), y0 and y1 likewise, the divisions
 *                   rounding towards -inf and +inf for negative coordinates too; x0 > x1 or y0 > y1 -- no pixel centre of the
 *                   image inside the box, a triangle wholly off the image among them --: neither drawn nor counted
 *                   otherwise DRAWN, counts[0], whether or not a centre turns out to be covered.
 *                 There is no face culling: where A < 0 the three edge values and A are negated.
 *     coverage    the centre c of pixel (x, y), x0 <= x <= x1, y0 <= y <= y1, is covered iff Ep = E(q, r; c), Eq = E(r, p; c) and
 *                 Er = E(p, q; c) are all >= 0 (after the negation).  Edges are inclusive; a centre on a shared edge is covered
 *                 twice and the depth test decides, so there is no fill rule.
 *     per pixel   lp = (float)Ep / (float)A, lq and lr likewise; v = ((lp iwp) + (lq iwq)) + (lr iwr): the inverse depth,
 *                 interpolated in the image.  v is positive and never subnormal or a NaN (the weights are in [0, 1], one is at
 *                 least 1/3, iw >= 2^-60 and finite), so its bits order it.  The winner of a pixel is the covering triangle of
 *                 greatest v, among equal v of smallest id.
 *     outputs     each w x h of the view, pitch w; every entry of every given output is written and nothing behind it; any but
 *                 depth may be NULL.  With the pixel's winner, its weights formed again by the expressions above:
 *                   depth     float: 1.0f / v;  0x7FC00000 where nothing was drawn (the form of every map in this file)
 *                   triangle  uint32: the id;  UINT32_MAX where nothing was drawn
 *                   shade     uint8: floorf((((lp gp) + (lq gq)) + (lr gr)) + 0.5f) clamped to 0 .. 255, g the corners' greys as
 *                             floats;  0 where nothing was drawn
 *                   counts_dev[3]  uint32 (device): triangles drawn, skipped as too large, skipped for a corner or a zero area
 *   2 residual  ssrlcv_hip_image_residual: image, shade (uint8) and depth of one w x h view, pitch w.  out = (float)image -
 *               (float)shade, one subtraction, where depth's bits are not 0x7FC00000; 0x7FC00000 elsewhere: the entries that
 *               ssrlcv_hip_difference_stats ("surface accuracy" item 2, validity) leaves out, so the map goes to it as it is.
 * Refusals, decided on the host before any launch, the parameters before the sizes before the buffers:
 *   render      SSRLCV_ERR_INVALID_ARG for a NULL params, maxExtent 0 or above 64, a NULL view, a non-finite entry of its M or
 *               pos; then for a view with w h >= 2^31, then a grid with gw gh >= 2^31.  No size is unsupported.  An empty view
 *               (w or h 0) then writes three zeros to counts_dev, if given, looks at nothing else and is SSRLCV_OK.  Then
 *               SSRLCV_ERR_INVALID_ARG for a NULL depth or workspace, or -- unless n is 0 or the grid has no cell (gw or gh
 *               below 2), where nothing is drawn and every output holds its "nothing drawn" value -- a NULL points,
 *               vertexIndex or cells; then SSRLCV_ERR_WORKSPACE.
 *   residual    SSRLCV_ERR_INVALID_ARG for w h >= 2^31; an empty view is then SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL
 *               image, shade, depth or out.
 * Workspace of render (host only; computed in size_t; 0 for a view with w h >= 2^31), a256 as in "disparity mesh":
 *     256 + a256(8 w h) + a256(16 n)
 *   the counters, one 64-bit accumulator a pixel, the projected vertices.  It may hold anything on entry.  The residual needs
 *   none.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  Three passes -- a thread a vertex,
 * a thread a cell (T0, then T1, at most (maxExtent + 1)^2 pixel centres each), a thread a pixel -- and global INTEGER atomics
 * only, a 64-bit max on (bits(v) << 32) | (0xFFFFFFFF - id) a covered centre and 32-bit adds for the counts, which commute: the
 * outputs do not depend on the order the triangles arrive in and are bit-equal run to run.  The residual uses no atomics.
 * Out of scope, not built: perspective-correct shading (the greys are interpolated in the image, like v); near-plane clipping (a
 * triangle with a corner at W <= 0 is dropped whole); triangles above 64 pixels; anti-aliasing; colour; pushbroom views;
 * triangle soups that are not a grid mesh; predicted disparities. */
typedef struct {
  uint32_t maxExtent; /* 1 .. 64: a triangle whose bounding box is wider or higher than this many pixels is skipped */
} ssrlcv_render_params; /* 4 bytes */
size_t ssrlcv_hip_mesh_render_workspace_bytes(uint32_t n, uint32_t w, uint32_t h);
int ssrlcv_hip_mesh_render(const ssrlcv_float3* points, uint32_t n, const uint8_t* grey /* may be NULL */, const uint32_t* vertexIndex,
                           const uint8_t* cells, uint32_t gw, uint32_t gh, const ssrlcv_ortho_view* view, const ssrlcv_render_params* params,
                           float* depth, uint32_t* triangle /* may be NULL */, uint8_t* shade /* may be NULL */,
                           uint32_t* counts_dev /* may be NULL */, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_hip_image_residual(const uint8_t* image, const uint8_t* shade, const float* depth, uint32_t w, uint32_t h, float* out,
                              ssrlcv_stream_t stream);

/* ---- surface simplification: the grid mesh of a height map holds two triangles a cell wherever the map is valid, on a plain as on
 * a cliff.  This section selects a subset of its nodes and a conforming triangulation of them: a hierarchical right-triangle mesh
 * (RTIN / restricted quadtree, Lindstrom-Pajarola) that keeps full resolution where the map is rough and at hole boundaries and
 * collapses to large triangles where it is flat.  It is a pure selection over the existing nodes -- no vertex is created -- and its
 * only float work is one fixed-order float32 expression a node plus max, which commutes: csrc/simplify.hip is held to a numpy
 * restatement bit for bit (tests/simplify_ref.py, tests/test_gpu_simplify.py).  The error map is computed once; a mesh at any
 * tolerance is then one extraction.
 *   input       a height map height[w h], float, pitch w, the form of every map in this file: a node is valid iff its bits are
 *               not 0x7FC00000; other NaNs, the infinities and -0 are valid values.
 *   domain      L is the smallest integer with 2^L >= max(w - 1, h - 1, 1), S = 2^L; the domain is the node square [0, S]^2.  A
 *               node is PRESENT iff it lies inside the grid (x < w, y < h) and is valid.  tz(v) = the number of trailing zero bits
 *               of v, tz(0) = infinity; k(x, y) = min(tz(x), tz(y)); a node of the domain is a SPLIT NODE iff k < L: every node but
 *               the domain's four corners.  u = 2^k.
 *     D-node      tz(x) == tz(y): the centre of a block of side 2u, level t = 2 (L - k - 1).  With I = (x - u) / (2u) and
 *                 J = (y - u) / (2u) the hypotenuse is the main diagonal iff I + J is even: a = (x - u, y - u), b = (x + u, y + u),
 *                 apexes (x + u, y - u) and (x - u, y + u); otherwise a = (x + u, y - u), b = (x - u, y + u), apexes
 *                 (x - u, y - u) and (x + u, y + u).  Children: (x +- u, y) and (x, y +- u).
 *     A-node      tz(x) != tz(y): the midpoint of a block edge, level t = 2 (L - k - 1) + 1.  If tz(x) < tz(y): a = (x - u, y),
 *                 b = (x + u, y), apexes (x, y - u) and (x, y + u); otherwise a = (x, y - u), b = (x, y + u), apexes (x - u, y) and
 *                 (x + u, y).  An apex outside the domain does not exist: the edge lies on the domain's border.  Children: the
 *                 four nodes (x +- u/2, y +- u/2) that lie in the domain; none when k = 0.
 *   1 errors    ssrlcv_hip_dsm_simplify_errors.  e(m) = +inf unless m, a, b and every existing apex of m are present; otherwise,
 *               in float32 with nothing contracted, mid = (h(a) + h(b)) * 0.5f, d = fabsf(h(m) - mid), e(m) = d if d < +inf, else
 *               +inf (a NaN becomes +inf).  E(m) = max(e(m), E of m's children); a split node of the domain outside the grid has
 *               E = +inf.  error[w h] (float) holds E for every split node of the grid and +inf for the at most four corners of
 *               the domain inside the grid.  Every entry lies in [+0, +inf], never a NaN and never -0, so its bits order it.
 *               Every entry is written and nothing behind the map.
 *   2 triangles ssrlcv_hip_dsm_simplify_mesh at a `tolerance` that is a finite float; a negative one is legal and gives the
 *               full-resolution mesh.  `error` is item 1's map of the same height map.
 *     split nodes for a split node m inside the grid and an existing apex c of it, the triangle with hypotenuse a-b and apex c is
 *                 emitted iff E(m) <= tol and (t(m) == 0 or !(E(c) <= tol)).  E(m) <= tol makes c present, so E(c) is an entry of
 *                 the map.
 *     leaves      cell (i, j), 0 <= i < w - 1, 0 <= j < h - 1, has its diagonal main iff i + j is even: a = (i, j),
 *                 b = (i + 1, j + 1), apexes (i + 1, j) and (i, j + 1); otherwise a = (i + 1, j), b = (i, j + 1), apexes (i, j)
 *                 and (i + 1, j + 1).  A leaf is emitted iff a, b and c are present and (L == 0 or !(E(c) <= tol)).
 *     record      (p, q, r) = (c, a, b) if (a.x - c.x) (b.y - c.y) - (a.y - c.y) (b.x - c.x) < 0 in integers, else (c, b, a): the
 *                 winding of "disparity mesh" item 3, so on a frame with the `winding` of "surface model" the faces look along
 *                 +ez.
 *     order       ascending (2 m.y, 2 m.x), the midpoint of the hypotenuse in doubled coordinates -- a leaf of cell (i, j) has
 *                 (2j + 1, 2i + 1) --, triangles that share a midpoint by apex (c.y, c.x).
 *     output      the three uint32 of a record are the corners' new vertex indices (item 3).  *triCount_dev (device) = the full
 *                 count; only the first min(count, capacity) records are written and nothing behind out[3 capacity) is touched;
 *                 out may be NULL with capacity 0 (the truncation contract of ssrlcv_hip_mesh_triangles).
 *   3 vertices  a node is KEPT iff it is a corner of an emitted triangle, whether or not that triangle fit into `capacity`.
 *               vertexIndex[w h] (uint32) holds a kept node's rank among the kept nodes in raster order and UINT32_MAX elsewhere;
 *               *vertexCount_dev (device) = their number.  kept[min(count, keptCapacity)] holds, per new vertex in order, the
 *               node's entry of nodeIndex[w h] if nodeIndex is given, else its raster index j w + i.  With the vertexIndex that
 *               ssrlcv_hip_disparity_mesh gives the same map at step 1 as nodeIndex, `kept` is strictly ascending in the
 *               numbering of ssrlcv_hip_dsm_points -- the form of keptIndex in ssrlcv_hip_mesh_select -- and a caller gathers
 *               points, normals and greys through it.
 *   bound       for an emitted triangle of level t every node inside it is the midpoint of one of its descendants, all of which
 *               have E <= tol: refining down to the node the piecewise-linear surface moves at most tol a level, so the vertical
 *               distance of any covered node from the triangle's plane is at most (2L - t) tol in exact arithmetic; the two
 *               float32 roundings of e add at most 2^-22 max|h| a level.  This is the only accuracy promise.
 *   border      a grid whose sides are not 2^L + 1 pays full refinement along the sides that cut the domain (an apex outside the
 *               grid is not present): a plane at tolerance 0 gives 2 triangles on 33 x 33, 147 on 20 x 34 and 46 on 17 x 12.
 *               The cost is a perimeter term and is accepted.
 * Refusals, decided on the host before any launch, in this order: SSRLCV_ERR_INVALID_ARG for a tolerance that is not finite (mesh)
 * and for w h >= 2^31; SSRLCV_ERR_UNSUPPORTED for w h > 2^29 -- the candidate numbering 2 w (2h - 1) must fit 32 bits --; mesh:
 * SSRLCV_ERR_INVALID_ARG for a NULL triCount_dev or vertexCount_dev; an empty map (w or h 0) then writes both counts 0 (errors:
 * nothing), looks at nothing else and is SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL buffer that has an element to hold
 * (height and error; mesh: vertexIndex and the workspace too, out unless capacity is 0, kept unless keptCapacity is 0; nodeIndex
 * may always be NULL); then SSRLCV_ERR_WORKSPACE.
 * Workspace of mesh (host only; computed in size_t; 0 for a refused or empty size), a256 and c as in "disparity mesh":
 *     c(2 w (2h - 1)) + c(w h)
 *   the tables of the compaction over the triangle candidates and of the one over the nodes.  It may hold anything on entry.
 *   The errors need none.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another.  errors: a level is two launches, its
 * A-nodes then its D-nodes, a thread a node of the level's lattice; the levels whose lattice has at most 4096 nodes run in one
 * block: 2L launches at most.  Every entry has one writer.  mesh: two ordered compactions (csrc/compact.h); the kept marks are
 * stores of one value.  No atomics at all: bit-equal run to run.
 * Out of scope: maxJump cuts (a cliff keeps full resolution through its error instead); errors measured in 3-D or along the normal;
 * edge-collapse or quadric decimation; rendering the simplified mesh with ssrlcv_hip_mesh_render, which takes grid meshes only;
 * normals recomputed on the simplified faces (gather the full-resolution ones); texture coordinates; tiling the domain so that a
 * grid with w - 1 not a power of two avoids border refinement. */
int ssrlcv_hip_dsm_simplify_errors(const float* height, uint32_t w, uint32_t h, float* error, ssrlcv_stream_t stream);
size_t ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_simplify_mesh(const float* height, const float* error, uint32_t w, uint32_t h, float tolerance,
                                 const uint32_t* nodeIndex /* may be NULL */, uint32_t* vertexIndex, uint32_t* out, uint32_t capacity,
                                 uint32_t* triCount_dev, uint32_t* kept, uint32_t keptCapacity, uint32_t* vertexCount_dev, void* workspace,
                                 size_t workspaceBytes, ssrlcv_stream_t stream);

/* ---- terrain filter: the fused height map is a digital SURFACE model -- the top of whatever the cameras saw, buildings and trees
 * included.  This section gives the ground under it (a terrain model) and the height of what stands on the ground (the normalised
 * surface, height - terrain): grey-scale morphology of a height map, the progressive morphological filter on top of it (Zhang et
 * al. 2003: the map is opened with growing square windows, and a cell that an opening lowers by more than a threshold is an
 * object), and the map - map difference.  Erosion and dilation are selections: csrc/terrain.hip is held to a numpy restatement
 * bit for bit (tests/terrain_ref.py, tests/test_gpu_terrain.py).  Maps as everywhere in this file: float[w h], pitch w.
 *   validity    a cell is valid iff its bits are not 0x7FC00000; other NaNs, the infinities and -0 are valid values.
 *   order       values are ordered by the integer key of the median filter ("disparity post-filters" item 4),
 *               k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF: a total order on bit patterns, so -0 < +0, every NaN has a place, and equal
 *               keys are equal bits.
 *   window      W_r(p) = the cells q of the image with |q.x - p.x| <= r and |q.y - p.y| <= r: clipped at the image, never padded.
 *               The effective radius is min(radius, max(w, h) - 1), applied on the host first: UINT32_MAX is legal and means "the
 *               whole map", and no kernel forms 2r + 1 of a radius the map does not hold.  radius == 0 is refused.
 *   1 morphology  ssrlcv_hip_dsm_morphology, op = SSRLCV_MORPH_ERODE (0), _DILATE (1), _OPEN (2) or _CLOSE (3).
 *     ERODE       out(p) = the value with the smallest key among the valid cells of W_r(p), whether or not p itself is valid;
 *                 invalid iff the window holds no valid cell.
 *     DILATE      the same with the largest key.
 *     OPEN        O = DILATE(ERODE(in)), then O(p) = invalid wherever in(p) is invalid: holes stay holes.  For a valid p the result
 *                 is always valid and k(O(p)) <= k(in(p)): every window that contains p has a minimum no larger than p, and the
 *                 dilation at p takes the largest of the minima of such windows, the one centred on p among them.
 *     CLOSE       the dual: ERODE(DILATE(in)) with the same mask, valid where `in` is and k(C(p)) >= k(in(p)).
 *     outputs     out of place; every cell of `out` is written and nothing behind it; in == out is refused.  No arithmetic, no
 *                 tolerance: the output bits are input bits or the invalid pattern.
 *   2 terrain   ssrlcv_hip_dsm_terrain.  Z_0 = height; for k = 1 .. levels: O_k = OPEN(Z_{k-1}, radius[k-1]) as in item 1, and
 *               Z_k = O_k.  In float32 with nothing contracted d = Z_{k-1}(p) - O_k(p); a valid cell is FLAGGED at level k iff
 *               d > threshold[k-1].  The comparison is false for a NaN d, so inf - inf flags nothing, and no difference is ever
 *               stored: NaN bit patterns cannot leak.
 *     level       (uint8, may be NULL) 0 for a ground cell that was never flagged, k for the first level that flagged it, 255 for
 *                 an invalid input cell.
 *     terrain     the bits of height(p) where `level` would be 0, the invalid pattern everywhere else.
 *     opened      (may be NULL) Z_levels.
 *     schedule    the thresholds are the caller's: this interface knows nothing of slopes or cell sizes.  Zhang's schedule,
 *                 t_1 = initial, t_k = min(initial + slope cell 2 (r_k - r_{k-1}), maximum), is MeshFactory::terrainSchedule and
 *                 pipeline.terrain_schedule.
 *     limit       an object flat enough, or wide enough, for the largest window to fit inside it is ground: an axis-aligned
 *                 plateau of side >= 2 r_max + 1 is never flagged.  This is the method and not a defect.
 *     border      windows are clipped, so a slope is opened lower within r cells of its uphill borders and may be flagged
 *                 there.  On an exact plane every cell at least 2 (r_1 + ... + r_K) cells from every border has d = 0 at every
 *                 level and is never flagged, even at threshold 0: the plane 0.3 i - 0.2 j + 1 on 80 x 70 with radii 1, 2, 4, 8
 *                 and thresholds 0 flags 1136 cells, all of them within 7 cells of a border.
 *   3 subtract  ssrlcv_hip_dsm_subtract.  out(p) = a(p) - b(p) in float32 where both are valid; a result that is a NaN is stored
 *               as the invalid pattern (the sign and payload of inf - inf differ between hosts and the GPU and must not reach the
 *               map); out(p) is invalid where either input is.  `out` may alias `a` or `b`.  height - filled terrain is the
 *               normalised surface; the call is also the map - map sibling of ssrlcv_hip_dsm_difference, and its output goes to
 *               ssrlcv_hip_difference_stats as it is.  No workspace.
 * Refusals, decided on the host before any launch, the parameters before the buffers, in this order: SSRLCV_ERR_INVALID_ARG for
 * params NULL, levels 0 or above 8, a radius that is 0 or not above the one before it, a threshold that is negative or not finite
 * (terrain), op > 3 or radius 0 (morphology); then for w h >= 2^31; a map of 0 cells is then SSRLCV_OK and touches nothing; then
 * SSRLCV_ERR_INVALID_ARG for a NULL map or workspace (level and opened may be NULL) and for in == out; then SSRLCV_ERR_WORKSPACE.
 * Workspace (host only; computed in size_t; 0 for a refused or empty size), in whole maps of a256(4 w h) bytes:
 *     morphology  2 a256(4 w h)     the result of the row pass and the running minima of the pass at work, the first result of
 *                                   an OPEN or CLOSE waiting in `out`; at an effective radius up to 8 that result alone
 *     terrain     4 a256(4 w h)     Z_{k-1}, the erosion, the result of the row pass, the running minima
 * It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no atomics; no block waits for another: bit-equal run to run.  At
 * an effective radius up to 8 an erosion or dilation is one launch that takes the 2r + 1 taps of a row and then of a column from a
 * tile in LDS, 34 taps a cell at most; it won its A/B at every such radius.  Above 8 it is a row pass and a column pass, two
 * launches, an opening four, and the work per cell and pass is O(1) whatever the radius: running minima over segments of 2r + 1
 * cells from both ends (van Herk / Gil-Werman), never a walk over the window; no loop has a trip count per cell that grows with
 * the radius.  Until its cells are written, `out` of such an OPEN or CLOSE holds the first of its two results.
 * Out of scope: slope-adaptive or per-cell thresholds inside the kernel; discs or other windows that are not squares;
 * cloth-simulation and TIN-densification ground filters; interpolating the terrain under objects with new values (close the
 * footprints with ssrlcv_hip_stereo_fill_holes, which selects); pit removal before the filter (an opening leaves an isolated pit
 * and its neighbours alone; CLOSE and ssrlcv_hip_dsm_subtract find pits); classifying the points of a cloud instead of the cells
 * of a map; the terrain inside the surface registration. */
#define SSRLCV_MORPH_ERODE 0
#define SSRLCV_MORPH_DILATE 1
#define SSRLCV_MORPH_OPEN 2
#define SSRLCV_MORPH_CLOSE 3
typedef struct {
  uint32_t levels;       /* 1 .. 8 */
  uint32_t radius[8];    /* strictly ascending over the first `levels` entries, each >= 1; the rest ignored */
  float    threshold[8]; /* finite and >= 0 over the first `levels` entries */
} ssrlcv_terrain_params; /* 68 bytes */
size_t ssrlcv_hip_dsm_morphology_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_morphology(const float* in, float* out, uint32_t w, uint32_t h, uint32_t radius, uint32_t op, void* workspace,
                              size_t workspaceBytes, ssrlcv_stream_t stream);
size_t ssrlcv_hip_dsm_terrain_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_terrain(const float* height, uint32_t w, uint32_t h, const ssrlcv_terrain_params* params, float* terrain,
                           uint8_t* level /* may be NULL */, float* opened /* may be NULL */, void* workspace, size_t workspaceBytes,
                           ssrlcv_stream_t stream);
int ssrlcv_hip_dsm_subtract(const float* a, const float* b, uint32_t w, uint32_t h, float* out, ssrlcv_stream_t stream);

/* ---- surface objects: the `objects` map of "terrain filter" (height - terrain) says how high something stands above the ground
 * at every cell; this section says WHAT stands there: one record per object -- a connected footprint of cells at least minHeight
 * above the ground -- with its place, area, outline length, moments and height sums, and a map of the objects' numbers.  An
 * inventory of buildings and trees, without reading the map back.  Everything a record holds is an integer sum, an integer
 * minimum or maximum, or a selected bit pattern, so it does not depend on the order of summation: csrc/objects.hip is held to a
 * numpy restatement byte for byte (tests/objects_ref.py, tests/test_gpu_objects.py), and that to a plain loop over cells.
 * Maps as everywhere in this file: float[w h], pitch w, a cell invalid iff its bits are 0x7FC00000.
 *   1 members   a cell is a member iff it is valid and v >= minHeight in float32.  The comparison is false for a NaN, so no
 *               member is a NaN (a non-canonical NaN is a valid cell and never a member); +inf is a member.  minHeight = -inf
 *               takes every valid cell that is no NaN, minHeight = +inf the +inf cells alone.
 *   2 objects   the components of "disparity post-filters" items 1-2 with maxDiff, of the map that holds v at members and the
 *               invalid pattern everywhere else: 4-connectivity, and the object's `label` is that section's label, the smallest
 *               raster index y w + x of its cells.  maxDiff = +inf joins a footprint whatever its roof does; a finite value parts
 *               a roof from a tree that leans on it.  Two +inf cells do not link (inf - inf is a NaN), as that section says.
 *   3 kept      an object is kept iff cells >= minCells (minCells = 0 behaves as 1).  Kept objects are numbered 0, 1, ... in
 *               ascending label.  *count_dev = the full number kept.  Only the first min(count, capacity) records are written, in
 *               that order; nothing behind records[capacity) is touched; records may be NULL with capacity 0: the truncation
 *               contract of ssrlcv_hip_stereo_matches.
 *   4 ids       (uint32[w h], may be NULL; if given, every entry is written) a cell of a kept object holds the object's number;
 *               a non-member holds UINT32_MAX, and so does a member of a dropped object.  The numbers do not depend on
 *               capacity: an object numbered at or above it still has its number in ids.
 *   5 record    ssrlcv_object_record, over the object's cells (x, y):
 *     label, cells            as above; 1 <= cells <= w h <= 2^30.
 *     minX, minY, maxX, maxY  the bounding box, inclusive; below 65536.
 *     sumX, sumY, sumXX, sumXY, sumYY   the sums of x, y, x x, x y, y y of the integer cell coordinates: sumX, sumY <= 2^30 (2^16
 *                             - 1) < 2^46; sumXX, sumXY, sumYY <= 2^30 (2^16 - 1)^2 < 2^62.
 *     perimeter               the number of cell sides whose other side lies outside the map or is not a cell of the same object;
 *                             at most 2 cells + 2 <= 2^31 + 2 (a 4-connected set), and the 2 w + 2 h sides of the grid are below 2^18.
 *     peak, peakIndex         the bits of the value with the largest order key k(f) of the median filter ("disparity
 *                             post-filters" item 4), and the smallest raster index that holds those bits.  -0 < +0.
 *     low                     the bits of the value with the smallest key.
 *     quantise                heights are quantised exactly as "shift search" quantises: t = v * scale, one float32
 *                             multiplication; the cell takes part iff fabsf(t) <= 65536.0f; then q = (int32)rintf(t), ties to even.
 *     clipped                 the members that fail that test (+inf among them); they count in `clipped` and in nothing below.
 *     sumQ, sumQQ             the sums of q and of q q over the cells that take part: |sumQ| <= 2^30 2^16 = 2^46, sumQQ <= 2^30
 *                             2^32 = 2^62.
 *     reserved                0.
 *   6 limits    w, h <= 65536 and w h <= 2^30.  With these every sum fits its field, as the bounds above say.
 *   7 measures  ssrlcv_object_measures_host (host only, in double, no device) turns one record into lengths, areas and shapes.
 *               Only + - * / and sqrt, every operation rounded on its own, nothing contracted, no libm call; u(k) is (double)k of
 *               an integer field (a sum above 2^53 rounds to nearest even there), c = (double)frame->cell, s = (double)scale:
 *                 n = u(cells);  cc = c * c;  area = n * cc;  perimeterLength = u(perimeter) * c;
 *                 compactness = (12.566370614359172 * area) / (perimeterLength * perimeterLength)      4 pi area / perimeter^2
 *                 centroidX = u(sumX) / n;  centroidY = u(sumY) / n                                     in cells, corner (0, 0) = 0
 *                 a = (centroidX + 0.5) * c;  b = (centroidY + 0.5) * c;  world[k] = (origin[k] + a * ex[k]) + b * ey[k]
 *               -- cell centres as ssrlcv_hip_dsm_points places a cell, on the frame's plane (the object heights are relative to the
 *               terrain and say nothing about the height of the ground) --
 *                 m = u(cells - clipped);  meanQ = u(sumQ) / m;  meanHeight = meanQ / s;  volume = (u(sumQ) / s) * cc;
 *                 var = u(sumQQ) / m - meanQ * meanQ;  rmsHeight = sqrt(var < 0 ? 0 : var) / s          about the mean
 *                 mxx = u(sumXX) / n - centroidX * centroidX;  mxy = u(sumXY) / n - centroidX * centroidY;
 *                 myy = u(sumYY) / n - centroidY * centroidY                                            in cells^2
 *                 t = 0.5 * (mxx + myy);  d = 0.5 * (mxx - myy);  r = sqrt(d * d + mxy * mxy);
 *                 lambdaMajor = t + r;  l = t - r;  lambdaMinor = l < 0 ? 0 : l;
 *                 (vx, vy) = d >= 0 ? (d + r, mxy) : (mxy, r - d);  if vx < 0 both change sign;  g = sqrt(vx * vx + vy * vy);
 *                 (axisX, axisY) = g > 0 ? (vx / g, vy / g) : (1, 0)                                    the major axis, axisX >= 0
 *                 elongation = lambdaMinor > 0 ? sqrt(lambdaMajor / lambdaMinor) : lambdaMajor > 0 ? +inf : 1
 *               A record with cells - clipped = 0 has meanHeight and rmsHeight a NaN (0 / 0) and volume 0; it is not refused.
 *               Refused with SSRLCV_ERR_INVALID_ARG: a NULL record, frame or out, a refused frame ("surface model"), a scale that
 *               is not finite and > 0, cells = 0 or clipped > cells.  `out` is untouched on error.
 * Refusals of the device call, decided on the host before any launch, the parameters before the sizes before the buffers, invalid
 * before unsupported within each: SSRLCV_ERR_INVALID_ARG for params NULL, minHeight a NaN, maxDiff a NaN or negative, scale not
 * finite or not > 0; then SSRLCV_ERR_UNSUPPORTED for w or h above 65536 or w h above 2^30; then SSRLCV_ERR_INVALID_ARG for a NULL
 * count_dev; a map of 0 cells then writes *count_dev = 0 and is SSRLCV_OK; then SSRLCV_ERR_INVALID_ARG for a NULL map or workspace,
 * or for records that are NULL with capacity > 0 or not 8-byte aligned (their 64-bit sums are added in place); then
 * SSRLCV_ERR_WORKSPACE for a short workspace.
 * Workspace (host only; computed in size_t; 0 for a refused or empty size), a256 and c as in "disparity mesh":
 *     3 a256(4 w h) + c(w h)
 *   the member map, which gives its place to the objects' numbers once the labelling has read it; the labels; the component
 *   counts; the tables of the compaction.  It may hold anything on entry.
 * Execution: asynchronous on `stream`; no host synchronisation; no block waits for another; integer atomics only; bit-equal run
 * to run.  A mask pass writes the member map; the labelling is that of "disparity post-filters", called, not copied; the kept
 * roots go through one ordered compaction (csrc/compact.h), which numbers them and initialises their records; the reduction
 * walks the map in 64 x 16 tiles.  There a cell's contributions merge first inside its wave over runs of adjacent lanes of one
 * tile-local component (one ballot gives the runs, shuffles add over them, as k_cc_tile and k_dsm_scatter do), next in LDS per tile-local root,
 * and each (tile, object, field) is flushed once to the record: 64-bit atomic adds for the seven sums, a 64-bit atomic max on
 * (key << 32) | (0xFFFFFFFF - index) for the peak, 32-bit atomic min, max and add for the box, `low`, `perimeter` and `clipped`;
 * a tile-local component that is the whole object is stored without atomics.  The perimeter compares final labels, read with a
 * halo of one cell.  The same pass writes ids.  A record of an object numbered at or above capacity is never touched.  A last
 * pass, a thread a record, turns the keys back into bits and writes *count_dev.  Capped grids stride over their items.
 * Out of scope: 8-connectivity; outlines as polygons; per-object medians or other quantiles; classifying an object as building or
 * vegetation; objects of a cloud instead of a map; merging objects across tiles of a larger mosaic. */
typedef struct {
  float minHeight;   /* no NaN; -inf and +inf are legal */
  float maxDiff;     /* >= 0, +inf is legal */
  float scale;       /* finite, > 0: quanta a height unit */
  uint32_t minCells; /* 0 behaves as 1 */
} ssrlcv_object_params; /* 16 bytes */
typedef struct {
  uint32_t label, cells;           /* smallest raster index of the object; number of its cells */
  uint32_t minX, minY, maxX, maxY; /* bounding box, inclusive */
  uint32_t perimeter, clipped;
  uint32_t peakIndex;
  float peak;
  float low;
  uint32_t reserved; /* 0 */
  uint64_t sumX, sumY, sumXX, sumXY, sumYY;
  int64_t sumQ;
  uint64_t sumQQ;
} ssrlcv_object_record; /* 104 bytes */
typedef struct {
  double area, perimeterLength, compactness;
  double centroidX, centroidY; /* in cells */
  double world[3];             /* the centroid on the frame's plane */
  double meanHeight, volume, rmsHeight;
  double mxx, mxy, myy;        /* central second moments, cells^2 */
  double lambdaMajor, lambdaMinor;
  double axisX, axisY;         /* unit vector of the major axis in cells, axisX >= 0 */
  double elongation;
} ssrlcv_object_measures; /* 152 bytes */
size_t ssrlcv_hip_dsm_objects_workspace_bytes(uint32_t w, uint32_t h);
int ssrlcv_hip_dsm_objects(const float* objects, uint32_t w, uint32_t h, const ssrlcv_object_params* params, uint32_t* ids /* may be NULL */,
                           ssrlcv_object_record* records, uint32_t capacity, uint32_t* count_dev, void* workspace, size_t workspaceBytes,
                           ssrlcv_stream_t stream);
int ssrlcv_object_measures_host(const ssrlcv_object_record* record, const ssrlcv_dsm_frame* frame, float scale,
                                ssrlcv_object_measures* out); /* host only */

/* The reference's key-point lists are unbounded (thrust-sized); the plan's are sized at creation
 * (ssrlcv_sift_params.maxKeyPointsPerOctave, default: a density bound).  If a list outgrew its capacity during the last
 * extract / describe on `workspace`, that octave's list was TRUNCATED at the capacity (in the reference's order: blur 1,
 * 2, 3, raster order inside a blur) and its bit is set in *octaveMask; the call then returns SSRLCV_ERR_CAPACITY and
 * the caller should re-run with a larger capacity.  Synchronises `stream`.  Callers that need the reference's result
 * must check this after every extract (the host mirror, ssrlcv_amd.pipeline and bench.py do). */
int ssrlcv_sift_plan_overflow(const ssrlcv_sift_plan* plan, const void* workspace, uint32_t* octaveMask,
                              ssrlcv_stream_t stream);

/* Introspection for kernel-level parity tests and profiling: device pointer + geometry of a pyramid level inside the
 * workspace.  kind: 0 = DoG level b (0..4, raw as written by build_dog), 1 = gaussian level b (0..5, un-normalised;
 * valid only for the last octave processed unless the plan keeps all levels).  minmax_dev: device pointer to {min,max}. */
int ssrlcv_sift_plan_level(const ssrlcv_sift_plan* plan, void* workspace, int kind, int octave, int blur, float** data,
                           uint32_t* w, uint32_t* h, float** minmax_dev);
/* Device key-point list of an octave after ssrlcv_hip_sift_describe or any ssrlcv_hip_sift_stage call: the list and the
 * octave's state words (8 ints: extremaBlurIndices[0..4], the count n, hasExtrema, overflow).
 * Both may be WRITTEN between two stage calls (behind a synchronisation of the stream, and before the next call): the next
 * stage runs on what it finds; stage 7 books the features from the state words.  The writer keeps what the kernels rely
 * on: blur in 1..3 for every key point (the levels that have gradient tables), the list sorted by blur and the indices
 * its ordered partition (idx[0] = idx[1] = 0), n at most the list capacity (ssrlcv_sift_params.maxKeyPointsPerOctave),
 * hasExtrema = (n > 0), overflow = 0, discard = 0, sigma / pixelWidth below 8, and every key point inside checkKeyPoints'
 * window at the plan's descriptorContribWidth (src/SIFT_FeatureFactory.cu:449-461, evaluated in float32): the sampling
 * kernels do not re-check it.  A key point whose orientation window leaves the level is legal and gets no orientation.
 * tests/test_gpu_sampling.py drives the sampling kernels this way. */
int ssrlcv_sift_plan_keypoints(const ssrlcv_sift_plan* plan, void* workspace, int octave, ssrlcv_sskeypoint** list,
                               int** blurIndices_dev);
/* Debug/test control: stop the key-point stage after `stage` (0 raw extrema, 1 removeNoise(0.8 thr), 2 refine,
 * 3 removeNoise, 4 removeEdges, 5 checkKeyPoints, 6 orientations; default 6 + descriptors). */
void ssrlcv_sift_plan_set_stop_stage(ssrlcv_sift_plan* plan, int stage);


/* ---- the key-point stage one KERNEL at a time over the caller's own buffers ----------------------
 * For a maintainer who keeps upstream's ScaleSpace objects -- DoG images in Octave::blurs[b]->pixels, Unity<SSKeyPoint>
 * lists, extremaBlurIndices on the host -- and replaces launches one by one.  Each entry stands for one launch site (or
 * thrust call) of src/FeatureFactory.cu / src/SIFT_FeatureFactory.cu, takes the same arrays in the same state, is
 * asynchronous on `stream`, and gives the results of the plan path (same device functions).  Pointers are device memory.
 * Counts upstream reads back after thrust::remove are left in a device word (count_dev) for the caller to copy.        */
/* findExtrema<<<>>> (src/FeatureFactory.cu:122, kernel :847-882): extrema[i] = i or -1 for interior pixels; border
 * pixels are not written (upstream initialises the array to -1).  pixels*: three neighbouring DoG levels. */
int ssrlcv_hip_find_extrema(uint32_t w, uint32_t h, const float* pixelsUpper, const float* pixelsMiddle, const float* pixelsLower,
                            int* extrema, ssrlcv_stream_t stream);
/* thrust::remove(addr, addr + n, -1) (:128), thrust::remove(thetas, .., -FLT_MAX) (:594), thrust::remove_if(extrema, ..,
 * discard) (discardExtrema :189): in place, order kept, one pass (csrc/scan_lookback.h). */
size_t ssrlcv_hip_compact_workspace_bytes(uint32_t n);
int ssrlcv_hip_compact_addresses(int* addresses, uint32_t n, uint32_t* count_dev, void* workspace, size_t workspaceBytes,
                                 ssrlcv_stream_t stream);
int ssrlcv_hip_compact_thetas(float* thetas, uint32_t n, uint32_t* count_dev, void* workspace, size_t workspaceBytes, ssrlcv_stream_t stream);
int ssrlcv_hip_compact_keypoints(ssrlcv_sskeypoint* keyPoints, uint32_t n, uint32_t* count_dev, void* workspace, size_t workspaceBytes,
                                 ssrlcv_stream_t stream);
/* fillExtrema<<<>>> (:140, kernel :883-890) */
int ssrlcv_hip_fill_extrema(uint32_t numKeyPoints, uint32_t w, uint32_t h, int octave, int blur, float sigma, const int* extremaAddresses,
                            const float* pixels, ssrlcv_sskeypoint* keyPoints, ssrlcv_stream_t stream);
/* flagNoise<<<>>> (removeNoise :275, kernel :968-973) */
int ssrlcv_hip_flag_noise(uint32_t numKeyPoints, ssrlcv_sskeypoint* keyPoints, float threshold, ssrlcv_stream_t stream);
/* refineLocation<<<>>> (:240, kernel :892-967); pixels_dev: DEVICE array of the octave's numBlurs DoG level pointers */
int ssrlcv_hip_refine_location(uint32_t numKeyPoints, uint32_t w, uint32_t h, float sigmaMin, float blurSigmaMultiplier, uint32_t numBlurs,
                               const float* const* pixels_dev, ssrlcv_sskeypoint* keyPoints, ssrlcv_stream_t stream);
/* flagEdges<<<>>> (removeEdges :299, kernel :974-990): key points startingIndex .. + numKeyPoints on one level's pixels */
int ssrlcv_hip_flag_edges(uint32_t numKeyPoints, uint32_t startingIndex, uint32_t w, uint32_t h, ssrlcv_sskeypoint* keyPoints,
                          const float* pixels, float threshold, ssrlcv_stream_t stream);
/* checkKeyPoints<<<>>> (src/SIFT_FeatureFactory.cu:98, kernel :449-461): sets discard, never clears it */
int ssrlcv_hip_check_keypoints(uint32_t numKeyPoints, uint32_t keyPointIndex, uint32_t w, uint32_t h, float pixelWidth, float lambda,
                               ssrlcv_sskeypoint* keyPoints, ssrlcv_stream_t stream);
/* calculatePixelGradients<<<>>> (Blur::computeGradients, src/Image.cu:1583-1598) */
int ssrlcv_hip_pixel_gradients(uint32_t w, uint32_t h, const float* pixels, ssrlcv_float2* gradients, ssrlcv_stream_t stream);
/* computeThetas<<<>>> (src/FeatureFactory.cu:587, kernel :1004-1112): thetaNumbers / thetas hold numKeyPoints x
 * maxOrientations entries, -1 / -FLT_MAX = none; maxOrientations <= 8 */
int ssrlcv_hip_compute_thetas(uint32_t numKeyPoints, uint32_t keyPointIndex, uint32_t w, uint32_t h, float pixelWidth, float lambda,
                              const ssrlcv_sskeypoint* keyPoints, const ssrlcv_float2* gradients, int* thetaNumbers, uint32_t maxOrientations,
                              float orientationThreshold, float* thetas, ssrlcv_stream_t stream);
/* expandKeyPoints<<<>>> (:608, kernel :1114-1122) */
int ssrlcv_hip_expand_keypoints(uint32_t numKeyPoints, const ssrlcv_sskeypoint* keyPointsIn, ssrlcv_sskeypoint* keyPointsOut,
                                const int* thetaAddresses, const float* thetas, ssrlcv_stream_t stream);
/* fillDescriptors<<<>>> (src/SIFT_FeatureFactory.cu:150, kernel :475-549): features[i] from key point keyPointIndex + i;
 * Feature::parent is left as it is (upstream's kernel does not write it).  The 128 bin sums upstream leaves to the order
 * of its shared-memory atomics are the order-independent integer sums of DESIGN.md section 2. */
int ssrlcv_hip_fill_descriptors(uint32_t numFeatures, uint32_t keyPointIndex, uint32_t w, uint32_t h, ssrlcv_sift_feature* features,
                                float pixelWidth, float lambda, const ssrlcv_sskeypoint* keyPoints, const ssrlcv_float2* gradients,
                                ssrlcv_stream_t stream);

/* Test hook: evaluates one of the device elementary functions (ssrlcv_amd/csrc/sv_math.h: the replacements for the
 * CUDA libm calls of src/FeatureFactory.cu:942,1040,1043, src/SIFT_FeatureFactory.cu:497-508, src/matrix_util.cu:314-327,
 * src/PointCloudFactory.cu:4180) element-wise on device arrays, so that parity tests can hold them bit for bit to the
 * oracle's.  fn: 0 expf(a), 1 atan2f(a, b), 2 sinf(a), 3 cosf(a), 4 tanf(a), 5 powf(a, b), 6 expf(a) for a <= 0
 * in the branch-free form the sampling kernels use, 7 / 8 the CUDA-form sinf(a) / cosf(a) of the camera rotation
 * matrices (sv_sinf_nv / sv_cosf_nv).  b may be NULL for unary fn. */
int ssrlcv_hip_math_eval(int fn, const float* a, const float* b, float* out, size_t n, ssrlcv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
