"""Thin Python plumbing over the C ABI (include/ssrlcv_hip.h) for tests and bench.py.

torch is used only for device memory and streams; every compute call goes through libssrlcv_hip.so with raw
device pointers.  Struct arrays travel as uint8 tensors (byte-compatible with include/ssrlcv_types.h).
"""
import ctypes

import numpy as np
import torch

from . import _lib

LIB = _lib.load()

c_u32, c_f32, c_vp, c_sz, c_int = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

OUT_DMATCH, OUT_UINT2_PAIR, OUT_MATCH = 0, 1, 2
_OUT_SIZE = {OUT_DMATCH: 48, OUT_UINT2_PAIR: 16, OUT_MATCH: 40}


class SsrlcvError(RuntimeError):
    pass


class MalformedPairList(SsrlcvError):
    """the device merge's input status word: an index out of range or a query matched twice in one pair"""


def check(rc):
    if rc != 0:
        raise SsrlcvError("ssrlcv_hip status %d: %s" % (rc, LIB.ssrlcv_hip_status_string(int(rc)).decode()))


def stream_ptr():
    return c_vp(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return c_vp(0)
    assert t.is_cuda and t.is_contiguous()
    return c_vp(t.data_ptr())


def to_dev(arr):
    """numpy (possibly structured) array -> uint8 CUDA tensor holding the same bytes."""
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def to_host(t, dtype, count=None):
    a = t.detach().cpu().numpy().view(np.uint8).reshape(-1)
    dt = np.dtype(dtype)
    if count is not None:
        a = a[: count * dt.itemsize]
    return a.view(dt).copy()


def dev_bytes(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")


class CameraStruct(ctypes.Structure):
    _fields_ = [("raw", ctypes.c_uint8 * 80)]


class MatchParams(ctypes.Structure):
    _fields_ = [("mode", c_int), ("queryImageID", c_u32), ("targetImageID", c_u32), ("epsilon", c_f32),
                ("delta", c_f32), ("relativeThreshold", c_f32), ("absoluteThreshold", c_f32),
                ("pad0", c_u32),  # ssrlcv_camera is 8-byte aligned
                ("queryCamera", ctypes.c_uint8 * 80), ("targetProjection", c_f32 * 12), ("fundamental", c_f32 * 9),
                ("pad1", c_u32 * 3)]  # the float4 member makes the struct 16-byte aligned


assert ctypes.sizeof(MatchParams) == 32 + 80 + 48 + 48, ctypes.sizeof(MatchParams)


class SiftParams(ctypes.Structure):
    _fields_ = [("maxOrientations", c_u32), ("orientationThreshold", c_f32), ("orientationContribWidth", c_f32),
                ("descriptorContribWidth", c_f32), ("maxKeyPointsPerOctave", c_u32)]


# ------------------------------------------------------------------ point cloud
def generate_bundles(matches_d, keypoints_d, num_bundles, cameras_d, num_cameras, num_keypoints):
    bundles = dev_bytes(num_bundles * 12)
    lines = dev_bytes(num_keypoints * 24)
    check(LIB.ssrlcv_hip_generate_bundles(ptr(matches_d), ptr(keypoints_d), c_u32(num_bundles), ptr(cameras_d),
                                          c_u32(num_cameras), ptr(bundles), ptr(lines), stream_ptr()))
    return bundles, lines


def generate_pushbroom_bundles(matches_d, keypoints_d, num_bundles, pushbrooms_d, num_cameras, num_keypoints):
    bundles = dev_bytes(num_bundles * 12)
    lines = dev_bytes(num_keypoints * 24)
    check(LIB.ssrlcv_hip_generate_pushbroom_bundles(ptr(matches_d), ptr(keypoints_d), c_u32(num_bundles),
                                                    ptr(pushbrooms_d), c_u32(num_cameras), ptr(bundles), ptr(lines),
                                                    stream_ptr()))
    return bundles, lines


def triangulate(lines_d, bundles_d, n, nview=False, want_points=True, want_errors=False, cutoff=None,
                no_error_variant=False):
    points = torch.zeros(max(n, 1) * 3, dtype=torch.float32, device="cuda") if want_points else None
    errors = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda") if want_errors else None
    # cutoff: a float, or a 1-element float32 CUDA tensor (a cutoff computed on the device: error_sample_cutoff)
    cut = None if cutoff is None else (cutoff if torch.is_tensor(cutoff) else torch.tensor([cutoff], dtype=torch.float32, device="cuda"))
    esum = torch.zeros(1, dtype=torch.float32, device="cuda")
    if nview:
        check(LIB.ssrlcv_hip_triangulateN(ptr(lines_d), ptr(bundles_d), c_u32(n), ptr(points), ptr(errors), ptr(cut),
                                          ptr(esum), c_int(1 if no_error_variant else 0), stream_ptr()))
    else:
        check(LIB.ssrlcv_hip_triangulate2(ptr(lines_d), ptr(bundles_d), c_u32(n), ptr(points), ptr(errors), ptr(cut),
                                          ptr(esum), stream_ptr()))
    return points, errors, esum


def error_sample_cutoff(errors_d, n, sample_jump, sigma):
    """deterministicStatisticalFilter's cutoff (sigma x std of every sample_jump-th error, sequential float sums) on the
    device -> 1-element float32 CUDA tensor."""
    cut = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_error_sample_cutoff(ptr(errors_d), c_u32(n), c_u32(sample_jump), c_f32(sigma), ptr(cut), stream_ptr()))
    return cut


def filter_matchset(bundles_d, keypoints_d, num_bundles, num_keypoints):
    """The MatchSet without the bundles flagged invalid -> (MultiMatch bytes, KeyPoint bytes, counts tensor {bundles kept,
    key points kept, key points in}); asynchronous."""
    LIB.ssrlcv_hip_filter_workspace_bytes.restype = ctypes.c_size_t
    ws = dev_bytes(int(LIB.ssrlcv_hip_filter_workspace_bytes(c_u32(num_bundles))))
    mm = dev_bytes(8 * max(num_bundles, 1))
    kp = dev_bytes(16 * max(num_keypoints, 1))
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_filter_matchset(ptr(bundles_d), ptr(keypoints_d), c_u32(num_bundles), ptr(mm), ptr(kp), ptr(counts),
                                         ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return mm, kp, counts


def select_pair_bundles(matches_d, keypoints_d, num_matches, num_keypoints, image_a, image_b):
    """The two-view bundles of image pair (a, b) of a MatchSet on the device as a two-camera MatchSet
    (ssrlcv_hip_select_pair_bundles) -> (MultiMatch bytes, KeyPoint bytes, count tensor); asynchronous."""
    ws = dev_bytes(int(LIB.ssrlcv_hip_select_pair_workspace_bytes(c_u32(num_matches))))
    mm = dev_bytes(8 * max(num_matches, 1))
    kp = dev_bytes(32 * max(num_matches, 1))
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_select_pair_bundles(ptr(matches_d), ptr(keypoints_d), c_u32(num_matches), c_u32(num_keypoints),
                                             c_int(image_a), c_int(image_b), ptr(mm), ptr(kp), ptr(count), ptr(ws), c_sz(ws.numel()),
                                             stream_ptr()))
    return mm, kp, count


def ba_sweep2(matches_d, keypoints_d, num_bundles, cameras_d, num_cameras, params_d, K):
    sums = torch.zeros(K, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_ba_sweep2(ptr(matches_d), ptr(keypoints_d), c_u32(num_bundles), ptr(cameras_d),
                                   c_u32(num_cameras), ptr(params_d), c_u32(K), ptr(sums), c_vp(0), c_sz(0),
                                   stream_ptr()))
    return sums


# ------------------------------------------------------------------ pose refinement
def _host_bytes(a, n):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:n].copy()


def pose_lm_terms(matches_d, n, pose6, query_cam_np, target_cam_np):
    """-> (JTJ[6,6] with JTJ[j, i] = out[i + 6 j], JTf[6], cost) of PoseEstimator::LM_iteration at `pose6`
    (roll, pitch, yaw, x, y, z)."""
    pose = np.asarray(pose6, np.float32).copy()
    q, t = _host_bytes(query_cam_np, 80), _host_bytes(target_cam_np, 80)
    out = torch.empty(43, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_pose_lm_terms(ptr(matches_d), c_u32(n), pose.ctypes.data_as(c_vp), q.ctypes.data_as(c_vp),
                                       t.ctypes.data_as(c_vp), ptr(out), stream_ptr()))
    o = out.cpu().numpy()
    return o[:36].reshape(6, 6).copy(), o[36:42].copy(), float(o[42])


def pose_cost(matches_d, n, pose6, query_cam_np, target_cam_np):
    pose = np.asarray(pose6, np.float32).copy()
    q, t = _host_bytes(query_cam_np, 80), _host_bytes(target_cam_np, 80)
    out = torch.empty(1, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_pose_cost(ptr(matches_d), c_u32(n), pose.ctypes.data_as(c_vp), q.ctypes.data_as(c_vp),
                                   t.ctypes.data_as(c_vp), ptr(out), stream_ptr()))
    return float(out.item())


# ------------------------------------------------------------------ fundamental-matrix RANSAC / relative pose
FMATRIX_AUX_WORKSPACE_BYTES = 256  # SSRLCV_FMATRIX_AUX_WORKSPACE_BYTES


def fmatrix_ransac(matches_d, n, samples, threshold, seed=0, mask=False, candidates=False):
    """-> dict(F[3, 3] float32, count, mask (uint8[n] or None), candidates (float32[3 samples, 9] or None),
    counts (uint32[3 samples] or None)) of ssrlcv_hip_fmatrix_ransac; matches_d: MATCH records on the device."""
    ws = dev_bytes(LIB.ssrlcv_hip_fmatrix_ransac_workspace_bytes(c_u32(n), c_u32(samples)))
    F = torch.empty(9, dtype=torch.float32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    m = dev_bytes(n) if mask else None
    cand = torch.empty(27 * samples, dtype=torch.float32, device="cuda") if candidates else None
    counts = torch.empty(3 * samples, dtype=torch.int32, device="cuda") if candidates else None
    check(LIB.ssrlcv_hip_fmatrix_ransac(ptr(matches_d), c_u32(n), c_u32(samples), c_f32(threshold), ctypes.c_uint64(seed),
                                        ptr(ws), c_sz(ws.numel()), ptr(F), ptr(cnt), ptr(m), ptr(cand), ptr(counts),
                                        stream_ptr()))
    return {"F": F.cpu().numpy().reshape(3, 3), "count": int(cnt.item()),
            "mask": m.cpu().numpy()[:n].copy() if mask else None,
            "candidates": cand.cpu().numpy().reshape(-1, 9) if candidates else None,
            "counts": counts.cpu().numpy().view(np.uint32).copy() if candidates else None}


def fmatrix_score(matches_d, n, F, threshold, mask=False):
    """-> (counts uint32[k], mask uint8[n] or None): inliers of each of the k pixel F matrices (numpy [k, 9] or [3, 3])."""
    Fh = np.ascontiguousarray(np.asarray(F, np.float32).reshape(-1, 9))
    k = len(Fh)
    Fd = torch.from_numpy(Fh.reshape(-1).copy()).cuda()
    ws = dev_bytes(FMATRIX_AUX_WORKSPACE_BYTES)
    counts = torch.empty(k, dtype=torch.int32, device="cuda")
    m = dev_bytes(n) if mask else None
    check(LIB.ssrlcv_hip_fmatrix_score(ptr(matches_d), c_u32(n), ptr(Fd), c_u32(k), c_f32(threshold), ptr(ws),
                                       c_sz(ws.numel()), ptr(counts), ptr(m), stream_ptr()))
    return counts.cpu().numpy().view(np.uint32).copy(), (m.cpu().numpy()[:n].copy() if mask else None)


def pose_from_fmatrix(matches_d, n, mask_d, F, query_cam_np, target_cam_np):
    """-> pose6 float32 (roll, pitch, yaw, x, y, z) of ssrlcv_hip_pose_from_fmatrix; mask_d: uint8 device tensor or None."""
    Fd = torch.from_numpy(np.ascontiguousarray(np.asarray(F, np.float32).reshape(9))).cuda()
    q, t = _host_bytes(query_cam_np, 80), _host_bytes(target_cam_np, 80)
    ws = dev_bytes(FMATRIX_AUX_WORKSPACE_BYTES)
    pose = np.zeros(6, np.float32)
    check(LIB.ssrlcv_hip_pose_from_fmatrix(ptr(matches_d), c_u32(n), ptr(mask_d), ptr(Fd), q.ctypes.data_as(c_vp),
                                           t.ctypes.data_as(c_vp), ptr(ws), c_sz(ws.numel()), pose.ctypes.data_as(c_vp),
                                           stream_ptr()))
    return pose


# ------------------------------------------------------------------ point cloud: k-NN, neighbour-distance filter, normals
KNN_MAX_K = 32  # SSRLCV_KNN_MAX_K


class Float3(ctypes.Structure):
    _fields_ = [("x", c_f32), ("y", c_f32), ("z", c_f32)]


def _cloud(points_d):
    """(n, 3) float32 device tensor (or its flat view) -> (contiguous tensor, n)"""
    assert points_d.is_cuda and points_d.dtype == torch.float32 and points_d.numel() % 3 == 0
    p = points_d.contiguous()
    return p, p.numel() // 3


def knn(points_d, k, cell_size=0.0, dist2=True, far=False):
    """ssrlcv_hip_knn -> (neighbours int32 [n, k] (UINT32_MAX reads as -1), dist2 float32 [n, k] or None, far-path query
    count (int32 [1] device tensor) or None).  Stream-ordered: nothing here synchronises."""
    p, n = _cloud(points_d)
    ws = dev_bytes(LIB.ssrlcv_hip_knn_workspace_bytes(c_u32(n), c_u32(k)))
    nbr = torch.empty((n, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, k), dtype=torch.float32, device="cuda") if dist2 else None
    fc = torch.zeros(1, dtype=torch.int32, device="cuda") if far else None
    check(LIB.ssrlcv_hip_knn(ptr(p), c_u32(n), c_u32(k), c_f32(cell_size), ptr(nbr), ptr(d2), ptr(fc), ptr(ws),
                             c_sz(ws.numel()), stream_ptr()))
    return nbr, d2, fc


def neighbor_distance_filter(points_d, dist2_d, k, sigma, normals_d=None):
    """ssrlcv_hip_neighbor_distance_filter -> dict of device tensors: points [n, 3] and index int32 [n] (the first
    `count` rows are the kept ones), mean float32 [n], stats float64 [3] = {mu, std, t}, count int32 [1], normals [n, 3]
    or None.  Stream-ordered."""
    p, n = _cloud(points_d)
    ws = dev_bytes(LIB.ssrlcv_hip_neighbor_filter_workspace_bytes(c_u32(n), c_u32(k)))
    out = {"points": torch.empty((n, 3), dtype=torch.float32, device="cuda"),
           "index": torch.empty(n, dtype=torch.int32, device="cuda"),
           "mean": torch.empty(n, dtype=torch.float32, device="cuda"),
           "stats": torch.empty(3, dtype=torch.float64, device="cuda"),
           "count": torch.empty(1, dtype=torch.int32, device="cuda"), "normals": None}
    nin = None
    if normals_d is not None:
        nin = normals_d.contiguous()
        assert nin.dtype == torch.float32 and nin.numel() == 3 * n
        out["normals"] = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_neighbor_distance_filter(ptr(p), c_u32(n), ptr(dist2_d.contiguous()), c_u32(k), c_f32(sigma),
                                                  ptr(out["mean"]), ptr(out["stats"]), ptr(out["points"]),
                                                  ptr(out["index"]), ptr(nin), ptr(out["normals"]), ptr(out["count"]),
                                                  ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return out


def point_normals(points_d, neighbors_d, k, viewpoint):
    """ssrlcv_hip_point_normals -> float32 [n, 3] device tensor; viewpoint: three numbers (host)."""
    p, n = _cloud(points_d)
    nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    vp = Float3(*[float(v) for v in viewpoint])
    check(LIB.ssrlcv_hip_point_normals(ptr(p), c_u32(n), ptr(neighbors_d.contiguous()), c_u32(k), vp, ptr(nrm),
                                       stream_ptr()))
    return nrm


# ------------------------------------------------------------------ matching
def projection_matrix(camera_np):
    cam = np.ascontiguousarray(camera_np).view(np.uint8).reshape(-1)[:80].copy()
    out = np.zeros(12, np.float32)
    LIB.ssrlcv_projection_matrix_host(cam.ctypes.data_as(c_vp), out.ctypes.data_as(c_vp))
    return out.reshape(3, 4)


def match_workspace(nq, nt):
    return dev_bytes(LIB.ssrlcv_hip_match_workspace_bytes(c_u32(nq), c_u32(nt)))


def seed_distances(query_d, nq, seed_d, ns, workspace=None):
    ws = workspace if workspace is not None else match_workspace(nq, ns)
    out = torch.empty(max(nq, 1), dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_seed_distances_u8x128(ptr(query_d), c_u32(nq), ptr(seed_d), c_u32(ns), ptr(out), ptr(ws),
                                               c_sz(ws.numel()), stream_ptr()))
    return out


def make_match_params(mode, query_id, target_id, epsilon=0.0, delta=0.0, rel=0.0, absolute=0.0, query_camera=None,
                      target_projection=None, fundamental=None):
    p = MatchParams()
    p.mode, p.queryImageID, p.targetImageID = mode, query_id, target_id
    p.epsilon, p.delta, p.relativeThreshold, p.absoluteThreshold = epsilon, delta, rel, absolute
    if query_camera is not None:
        raw = np.ascontiguousarray(query_camera).view(np.uint8).reshape(-1)[:80]
        ctypes.memmove(p.queryCamera, raw.ctypes.data, 80)
    if target_projection is not None:
        tp = np.ascontiguousarray(target_projection, dtype=np.float32).reshape(-1)
        ctypes.memmove(p.targetProjection, tp.ctypes.data, 48)
    if fundamental is not None:
        f9 = np.ascontiguousarray(fundamental, dtype=np.float32).reshape(-1)
        ctypes.memmove(p.fundamental, f9.ctypes.data, 36)
    return p


MATCH_ARITH_I8, MATCH_ARITH_F16 = 0, 1


def set_match_arithmetic(arithmetic):
    """int8 MFMA (default) or fp16 MFMA behind every matcher call of this process: both exact, same outputs."""
    check(LIB.ssrlcv_hip_set_match_arithmetic(c_int(arithmetic)))


def get_match_arithmetic():
    return int(LIB.ssrlcv_hip_get_match_arithmetic())


def match(query_d, nq, target_d, nt, params, out_kind=OUT_DMATCH, seed_d=None, workspace=None, out=None):
    ws = workspace if workspace is not None else match_workspace(nq, nt)
    if out is None:
        out = dev_bytes(nq * _OUT_SIZE[out_kind])
    check(LIB.ssrlcv_hip_match_u8x128(ptr(query_d), c_u32(nq), ptr(target_d), c_u32(nt), ptr(seed_d),
                                      ctypes.byref(params), c_int(out_kind), ptr(out), ptr(ws), c_sz(ws.numel()),
                                      stream_ptr()))
    return out


# ------------------------------------------------------------------ two nearest neighbours, ratio test, mutual check
class RatioParams(ctypes.Structure):
    _fields_ = [("queryImageID", c_u32), ("targetImageID", c_u32), ("ratio", c_f32), ("absoluteThreshold", c_f32),
                ("mutual", c_int)]


def match2_workspace(nq, nt):
    """Workspace of match_knn2 / match_ratio; it begins with match_workspace(nq, nt)'s layout, so compact_matches takes it."""
    return dev_bytes(LIB.ssrlcv_hip_match2_workspace_bytes(c_u32(nq), c_u32(nt)))


def match_knn2(query_d, nq, target_d, nt, dist=True, workspace=None):
    """ssrlcv_hip_match_knn2_u8x128 -> (index int32 [nq, 2] (UINT32_MAX reads as -1), distance float32 [nq, 2] or None):
    the two targets smallest by (distance, f mod 32, f).  Stream-ordered."""
    ws = workspace if workspace is not None else match2_workspace(nq, nt)
    idx = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, 2), dtype=torch.float32, device="cuda") if dist else None
    check(LIB.ssrlcv_hip_match_knn2_u8x128(ptr(query_d), c_u32(nq), ptr(target_d) if nt else c_vp(0), c_u32(nt), ptr(idx), ptr(d),
                                           ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return idx, d


def make_ratio_params(query_id, target_id, ratio=0.8, absolute=3.0e9, mutual=False):
    return RatioParams(query_id, target_id, ratio, absolute, 1 if mutual else 0)


def match_ratio(query_d, nq, target_d, nt, params, out_kind=OUT_DMATCH, workspace=None, out=None):
    """ssrlcv_hip_match_ratio_u8x128: nearest neighbour kept by Lowe's ratio test, the absolute threshold and (params.mutual)
    the cross check -> nq records of out_kind, laid out as match() writes them."""
    ws = workspace if workspace is not None else match2_workspace(nq, nt)
    if out is None:
        out = dev_bytes(nq * _OUT_SIZE[out_kind])
    check(LIB.ssrlcv_hip_match_ratio_u8x128(ptr(query_d), c_u32(nq), ptr(target_d) if nt else c_vp(0), c_u32(nt),
                                            ctypes.byref(params), c_int(out_kind), ptr(out), ptr(ws), c_sz(ws.numel()),
                                            stream_ptr()))
    return out


def compact_matches(out_kind, matches_d, n, workspace):
    cnt = c_u32(0)
    check(LIB.ssrlcv_hip_compact_matches(c_int(out_kind), ptr(matches_d), c_u32(n), ctypes.byref(cnt), ptr(workspace),
                                         c_sz(workspace.numel()), stream_ptr()))
    return cnt.value


def compact_matches_async(out_kind, matches_d, n, workspace, count_d):
    """Compaction without the host round trip: count_d (1-element int32 CUDA tensor / slice) receives the survivors."""
    check(LIB.ssrlcv_hip_compact_matches_async(c_int(out_kind), ptr(matches_d), c_u32(n), ptr(count_d), ptr(workspace),
                                               c_sz(workspace.numel()), stream_ptr()))


def sort_keys(keys_d, n):
    """perm (int32 CUDA tensor of n uint32) ordering 0 .. n-1 by ascending (keys[i], i) -- the sort of the band-culled modes"""
    ws = dev_bytes(int(LIB.ssrlcv_hip_sort_workspace_bytes(c_u32(n))))
    perm = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_sort_keys_u32(ptr(keys_d), c_u32(n), ptr(perm), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return perm[:n]


def keypoints_from_members(members_d, n, feature_tensors):
    """KeyPoint{image, location} of every {image, feature} member, gathered on the device -> uint8 tensor (16 B each)."""
    V = len(feature_tensors)
    assert all(t is None or t.is_cuda for t in feature_tensors), "feature arrays must live on the device"
    ptrs = (c_vp * V)(*[t.data_ptr() if t is not None and t.numel() else 0 for t in feature_tensors])
    counts = (c_u32 * V)(*[(t.numel() // 152) if t is not None else 0 for t in feature_tensors])
    out = dev_bytes(16 * n)
    check(LIB.ssrlcv_hip_keypoints_from_members(ptr(members_d), c_u32(n), ptrs, counts, c_u32(V), ptr(out), stream_ptr()))
    return out


def merge_matches_device(num_features, pair_counts, pairs_d, workspace=None):
    """Device merge of the validated uint2_pair arrays of all image pairs (concatenated in pair order, on the device) ->
    (MultiMatch bytes, member bytes, numMatches, numMembers, rounds).  One small D2H copy of the two counts."""
    V = len(num_features)
    nf = (c_u32 * V)(*[int(x) for x in num_features])
    pc = (c_u32 * max(len(pair_counts), 1))(*[int(x) for x in pair_counts])
    total = int(sum(int(x) for x in pair_counts))
    LIB.ssrlcv_hip_merge_workspace_bytes.restype = ctypes.c_size_t
    need = int(LIB.ssrlcv_hip_merge_workspace_bytes(c_u32(V), nf, c_u32(total)))
    if need == 0:
        raise ValueError("ssrlcv_hip_merge_matches: 2..32 images")
    if workspace is None or workspace.numel() < need:
        workspace = dev_bytes(need)
    mm = dev_bytes(8 * max(total, 1))
    mem = dev_bytes(8 * 2 * max(total, 1))
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_merge_matches(c_u32(V), nf, c_u32(len(pair_counts)), pc, ptr(pairs_d) if total else None, ptr(workspace),
                                       c_sz(workspace.numel()), ptr(mm), ptr(mem), ptr(counts), stream_ptr()))
    n_mm, n_mem, bad, rounds = [int(x) for x in counts.cpu().tolist()]  # the one synchronisation of the (asynchronous) call
    if bad & 4:  # (bit 2: a block of the persistent walk was not resident and its grid barrier gave up, csrc/merge.hip)
        raise SsrlcvError("ssrlcv_hip_merge_matches: the persistent walk could not keep all its blocks resident (grid barrier timed out)")
    if bad:
        raise MalformedPairList("ssrlcv_hip_merge_matches: malformed pair list (status word %d)" % bad)
    return mm[: 8 * n_mm], mem[: 8 * n_mem], n_mm, n_mem, rounds, workspace


def matchset_from_matches(in_kind, matches_d, n, want_max=False):
    """Device M7: (KeyPoint[2n] bytes, MultiMatch[n] bytes, max distance or None) from a validated DMatch / Match array."""
    kp = dev_bytes(32 * n)
    mm = dev_bytes(8 * n)
    mx = torch.full((1,), -1.0, dtype=torch.float32, device="cuda") if want_max else None
    check(LIB.ssrlcv_hip_matchset_from_matches(c_int(in_kind), ptr(matches_d), c_u32(n), ptr(kp), ptr(mm), ptr(mx),
                                               stream_ptr()))
    return kp, mm, (float(mx.item()) if want_max else None)


# ------------------------------------------------------------------ SIFT kernel-level
def gauss_kernel(sigma, pixel_width):
    w = np.zeros(129, np.float32)
    taps = LIB.ssrlcv_gauss_kernel_host(c_f32(sigma), c_f32(pixel_width), w.ctypes.data_as(c_vp))
    return taps, w[:max(taps, 0)].copy()


def convert_to_bw(color_d, depth, n):
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    check(LIB.ssrlcv_hip_convert_to_bw(ptr(color_d), c_u32(depth), ptr(out), c_sz(n), stream_ptr()))
    return out


def upsample2x_u8(img_d, w, h):
    out = torch.empty(4 * w * h, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_upsample2x_u8(ptr(img_d), c_u32(w), c_u32(h), ptr(out), stream_ptr()))
    return out


def upsample2x(img_d, w, h):
    out = torch.empty(4 * w * h, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_upsample2x(ptr(img_d), c_u32(w), c_u32(h), ptr(out), stream_ptr()))
    return out


def u8_to_f32(img_d, n):
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_u8_to_f32(ptr(img_d), ptr(out), c_sz(n), stream_ptr()))
    return out


def bin2x(img_d, w, h):
    out = torch.empty((w // 2) * (h // 2), dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_bin2x(ptr(img_d), c_u32(w), c_u32(h), ptr(out), stream_ptr()))
    return out


def gauss_sep_conv(img_d, w, h, weights, want_minmax=True):
    out = torch.empty(w * h, dtype=torch.float32, device="cuda")
    mm = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38], dtype=torch.float32, device="cuda") \
        if want_minmax else None
    wh = np.ascontiguousarray(weights, dtype=np.float32)
    check(LIB.ssrlcv_hip_gauss_sep_conv(ptr(img_d), ptr(out), c_vp(0), c_u32(w), c_u32(h), c_int(len(wh)),
                                        wh.ctypes.data_as(c_vp), ptr(mm), stream_ptr()))
    return out, mm


def minmax(img_d, n):
    mm = torch.empty(2, dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_minmax(ptr(img_d), c_sz(n), ptr(mm), stream_ptr()))
    return mm


def normalize_(img_d, n, mm_d):
    check(LIB.ssrlcv_hip_normalize(ptr(img_d), c_sz(n), ptr(mm_d), stream_ptr()))


def math_eval(fn, a, b=None):
    """Test hook: element-wise device elementary function (0 expf, 1 atan2f(a,b), 2 sinf, 3 cosf, 4 tanf, 5 powf(a,b))."""
    a_d = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    b_d = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).cuda()
    out = torch.empty_like(a_d)
    check(LIB.ssrlcv_hip_math_eval(c_int(fn), ptr(a_d), ptr(b_d), ptr(out), c_sz(a_d.numel()), stream_ptr()))
    return out.cpu().numpy()


# ------------------------------------------------------------------ dense SIFT
class DenseParams(ctypes.Structure):
    _fields_ = [("stride", c_u32), ("sigma", c_f32), ("maxOrientations", c_u32), ("orientationThreshold", c_f32),
                ("orientationContribWidth", c_f32), ("descriptorContribWidth", c_f32)]


def dense_grid(w, h, params):
    """-> (margin, nx, ny) of the dense grid (host only); raises for parameters the library refuses."""
    m, nx, ny = c_u32(), c_u32(), c_u32()
    check(LIB.ssrlcv_sift_dense_grid(c_u32(w), c_u32(h), ctypes.byref(params), ctypes.byref(m), ctypes.byref(nx), ctypes.byref(ny)))
    return m.value, nx.value, ny.value


def dense_workspace(w, h, params):
    return dev_bytes(int(LIB.ssrlcv_hip_sift_dense_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(params))))


def sift_dense(pix_d, stride=1, sigma=1.6, max_orientations=2, orientation_threshold=0.8, orientation_contrib_width=1.5,
               descriptor_contrib_width=6.0, capacity=None, workspace=None):
    """Dense SIFT (ssrlcv_hip_sift_dense_u8) of a u8 CUDA tensor (H, W): one key point every `stride` pixels, all at scale
    `sigma`.  -> (feature bytes [min(count, capacity) * 152], count).  capacity defaults to the grid's maximum."""
    h, w = pix_d.shape
    p = DenseParams(stride, sigma, max_orientations, orientation_threshold, orientation_contrib_width, descriptor_contrib_width)
    dense_grid(w, h, p)
    cap = int(LIB.ssrlcv_sift_dense_max_features(c_u32(w), c_u32(h), ctypes.byref(p))) if capacity is None else int(capacity)
    need = int(LIB.ssrlcv_hip_sift_dense_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(p)))
    ws = workspace if workspace is not None and workspace.numel() >= need else dev_bytes(need)
    feats = dev_bytes(cap * 152)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_sift_dense_u8(ptr(pix_d), c_u32(w), c_u32(h), ctypes.byref(p), ptr(ws), c_sz(ws.numel()), ptr(feats),
                                       c_u32(cap), ptr(count), stream_ptr()))
    n = int(count.item())
    return feats[: min(n, cap) * 152], n


# ------------------------------------------------------------------ dense stereo
class StereoParams(ctypes.Structure):
    _fields_ = [("radius", c_u32), ("minDisparity", ctypes.c_int32), ("numDisparities", c_u32), ("maxCost", c_u32),
                ("lrTolerance", ctypes.c_int32), ("subpixel", c_u32)]


STEREO_NO_LIMIT = 0xFFFFFFFF  # maxCost: no test
STEREO_INVALID_BITS = 0x7FC00000  # the bit pattern of an invalid pixel of a disparity map


def stereo_workspace(w, h, params):
    return dev_bytes(int(LIB.ssrlcv_hip_stereo_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(params))))


def _stereo_call(entries, p, left_d, right_d, want_cost, workspace, census):
    """what stereo_disparity and stereo_sgm share: the call on the pair with parameters `p`, the workspace reused if it is
    large enough.  entries = ((SAD call, its workspace query), (census call, its workspace query)): census = 0 takes the first
    pair, a census radius the second, which takes the radius behind the parameters.  -> (disparity, cost or None)"""
    h, w = left_d.shape
    assert right_d.shape == left_d.shape and left_d.dtype == torch.uint8 and right_d.dtype == torch.uint8
    assert left_d.is_cuda and right_d.is_cuda and left_d.is_contiguous() and right_d.is_contiguous()  # read with pitch w
    assert isinstance(census, int) and not isinstance(census, bool) and 0 <= census <= 0xFFFFFFFF  # c_u32 would wrap or truncate it
    entry, workspace_bytes = entries[1 if census else 0]
    extra = (c_u32(census),) if census else ()
    need = int(workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(p), *extra))
    ws = workspace if workspace is not None and workspace.numel() >= max(need, 1) else dev_bytes(need)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_cost else None
    check(entry(ptr(left_d), ptr(right_d), c_u32(w), c_u32(h), ctypes.byref(p), *extra, ptr(ws), c_sz(ws.numel()), ptr(disp), ptr(cost),
                stream_ptr()))
    return disp, cost


def stereo_disparity(left_d, right_d, radius=4, min_disparity=0, num_disparities=64, max_cost=STEREO_NO_LIMIT, lr_tolerance=1,
                     subpixel=True, want_cost=True, workspace=None, census=0):
    """Block matching of two rectified u8 CUDA tensors (H, W): SAD (ssrlcv_hip_stereo_sad_u8), or with census = 1, 2 or 3 the
    census cost of that radius (ssrlcv_hip_stereo_census_u8; include/ssrlcv_hip.h "census cost"), `radius` then being the
    aggregation radius 0 .. 7.
    -> (disparity float32 (H, W), invalid pixels hold STEREO_INVALID_BITS; cost int32 (H, W) holding the uint32 bits, or
    None).  Asynchronous on the current stream."""
    p = StereoParams(radius, min_disparity, num_disparities, max_cost, lr_tolerance, 1 if subpixel else 0)
    return _stereo_call(((LIB.ssrlcv_hip_stereo_sad_u8, LIB.ssrlcv_hip_stereo_workspace_bytes),
                         (LIB.ssrlcv_hip_stereo_census_u8, LIB.ssrlcv_hip_stereo_census_workspace_bytes)), p, left_d, right_d, want_cost,
                        workspace, census)


def census(img_d, census):
    """The census codes of a u8 CUDA tensor (H, W) (ssrlcv_hip_census_u8; include/ssrlcv_hip.h "census cost" item 1), census =
    1, 2 or 3 -> int64 (H, W) holding the uint64 bits.  Asynchronous on the current stream."""
    assert img_d.dim() == 2 and img_d.dtype == torch.uint8 and img_d.is_cuda and img_d.is_contiguous()  # read with pitch w
    assert isinstance(census, int) and not isinstance(census, bool) and 0 <= census <= 0xFFFFFFFF
    h, w = img_d.shape
    codes = torch.empty((h, w), dtype=torch.int64, device="cuda")
    check(LIB.ssrlcv_hip_census_u8(ptr(img_d), c_u32(w), c_u32(h), c_u32(census), ptr(codes), stream_ptr()))
    return codes


class SgmParams(ctypes.Structure):
    _fields_ = [("radius", c_u32), ("minDisparity", ctypes.c_int32), ("numDisparities", c_u32), ("costClamp", c_u32), ("P1", c_u32),
                ("P2", c_u32), ("paths", c_u32), ("lrTolerance", ctypes.c_int32), ("subpixel", c_u32)]


def stereo_sgm(left_d, right_d, radius=2, min_disparity=0, num_disparities=64, cost_clamp=1000, p1=40, p2=400, paths=0xFF,
               lr_tolerance=1, subpixel=True, want_cost=False, workspace=None, census=0):
    """Semi-global matching over the clamped SAD costs (ssrlcv_hip_stereo_sgm_u8; include/ssrlcv_hip.h "semi-global
    matching") of two rectified u8 CUDA tensors (H, W), or with census = 1, 2 or 3 over the census costs of that radius
    (ssrlcv_hip_stereo_sgm_census_u8; "census cost"), `radius` then being the aggregation radius 0 .. 7.  -> (disparity, cost or
    None) as stereo_disparity gives them; the cost is the winner's summed path cost.  The workspace holds two uint16 volumes of
    H W num_disparities entries each.  Asynchronous on the current stream."""
    p = SgmParams(radius, min_disparity, num_disparities, cost_clamp, p1, p2, paths, lr_tolerance, 1 if subpixel else 0)
    return _stereo_call(((LIB.ssrlcv_hip_stereo_sgm_u8, LIB.ssrlcv_hip_stereo_sgm_workspace_bytes),
                         (LIB.ssrlcv_hip_stereo_sgm_census_u8, LIB.ssrlcv_hip_stereo_sgm_census_workspace_bytes)), p, left_d, right_d, want_cost,
                        workspace, census)


def stereo_sgm_set_pass_events(events):
    """torch.cuda.Events (or None to remove the hook) that every later stereo_sgm records between its passes
    (ssrlcv_hip_stereo_sgm_set_pass_events): before the first launch, behind the cost pass, behind each selected direction,
    behind the winner pass and behind the left-right check.  The caller keeps the events alive until it removes the hook."""
    if not events:
        check(LIB.ssrlcv_hip_stereo_sgm_set_pass_events(None, c_u32(0)))
        return
    for e in events:
        e.record()                   # torch creates the underlying hipEvent_t lazily, on the first record
    arr = (c_vp * len(events))(*[e.cuda_event for e in events])
    check(LIB.ssrlcv_hip_stereo_sgm_set_pass_events(arr, c_u32(len(events))))


def stereo_matches(disp_d, step=1, left_id=0, right_id=1, capacity=None):
    """The valid pixels of a disparity map on the `step` grid as Match records (ssrlcv_hip_stereo_matches), in raster order.
    -> (Match bytes [min(count, capacity) * 40], count).  capacity defaults to the grid's size."""
    h, w = disp_d.shape
    assert step >= 1 and disp_d.dtype == torch.float32 and disp_d.is_cuda and disp_d.is_contiguous()  # read with pitch w
    cap = -(-w // step) * -(-h // step) if capacity is None else int(capacity)
    need = int(LIB.ssrlcv_hip_stereo_matches_workspace_bytes(c_u32(w), c_u32(h), c_u32(step)))
    ws = dev_bytes(need)
    out = dev_bytes(cap * 40)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_stereo_matches(ptr(disp_d), c_u32(w), c_u32(h), c_u32(step), c_int(left_id), c_int(right_id), ptr(out),
                                        c_u32(cap), ptr(count), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    n = int(count.item())
    return out[: min(n, cap) * 40], n


def stereo_points(matches_d, n, foc, baseline, doffset, cx, cy):
    """upstream's stereo_disparity (ssrlcv_hip_stereo_points) -> float32 (n, 3)"""
    assert matches_d.dtype == torch.uint8 and matches_d.numel() >= 40 * n
    pts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_stereo_points(ptr(matches_d), c_u32(n), c_f32(foc), c_f32(baseline), c_f32(doffset), c_f32(cx), c_f32(cy),
                                       ptr(pts), stream_ptr()))
    return pts


# ------------------------------------------------------------------ rectification
RECTIFICATION = np.dtype([("Hl", "<f4", (9,)), ("Hr", "<f4", (9,)), ("Gl", "<f4", (9,)), ("Gr", "<f4", (9,)), ("w", "<u4"), ("h", "<u4"),
                          ("foc", "<f4"), ("baseline", "<f4"), ("doffset", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("cam_rot", "<f4", (3,))])
assert RECTIFICATION.itemsize == 184


def camera_bytes(cam):
    raw = np.ascontiguousarray(cam).view(np.uint8).reshape(-1)
    assert raw.size == 80, "one Image::Camera record (80 bytes)"
    return raw.copy()


def homography9(Hm):
    """9 floats, row-major -> a host float[9] (None passes NULL)"""
    if Hm is None:
        return None
    a = np.ascontiguousarray(Hm, np.float32).reshape(-1)
    assert a.size == 9, "a homography is 9 floats, row-major"
    return (c_f32 * 9)(*[float(v) for v in a])


def rectify_cameras(cam_l, cam_r):
    """ssrlcv_rectify_cameras_host of two Image::Camera records (host arithmetic: needs no GPU) -> a RECTIFICATION record."""
    a, b = camera_bytes(cam_l), camera_bytes(cam_r)
    out = np.zeros(1, RECTIFICATION)
    check(LIB.ssrlcv_rectify_cameras_host(a.ctypes.data_as(c_vp), b.ctypes.data_as(c_vp), out.ctypes.data_as(c_vp)))
    return out[0]


def warp_homography(src_d, Hm, out_shape=None):
    """dst(x, y) = src sampled bilinearly at H (x, y) (ssrlcv_hip_warp_homography_u8); src_d a u8 CUDA tensor (H, W), out_shape
    (rows, columns) defaults to the source's.  -> u8 CUDA tensor.  Asynchronous on the current stream."""
    assert src_d.dim() == 2 and src_d.dtype == torch.uint8 and src_d.is_cuda and src_d.is_contiguous()  # read with pitch w
    sh, sw = src_d.shape
    dh, dw = (sh, sw) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    dst = torch.empty((dh, dw), dtype=torch.uint8, device="cuda")
    check(LIB.ssrlcv_hip_warp_homography_u8(ptr(src_d), c_u32(sw), c_u32(sh), homography9(Hm), ptr(dst), c_u32(dw), c_u32(dh), stream_ptr()))
    return dst


def stereo_mask_rectified(disp_d, cost_d, radius, rect):
    """Invalidates, in place, the pixels of stereo_disparity's maps whose windows left the source images of the rectification
    `rect` (ssrlcv_hip_stereo_mask_rectified); cost_d may be None.  Asynchronous on the current stream."""
    h, w = disp_d.shape
    assert disp_d.dtype == torch.float32 and disp_d.is_cuda and disp_d.is_contiguous()  # read with pitch w
    assert cost_d is None or (cost_d.shape == disp_d.shape and cost_d.dtype == torch.int32 and cost_d.is_cuda and cost_d.is_contiguous())
    check(LIB.ssrlcv_hip_stereo_mask_rectified(ptr(disp_d), ptr(cost_d), c_u32(w), c_u32(h), c_u32(radius), homography9(rect["Hl"]), homography9(rect["Hr"]),
                                               c_u32(int(rect["w"])), c_u32(int(rect["h"])), stream_ptr()))
    return disp_d, cost_d


def matches_apply_homography(matches_d, n, H0, H1):
    """keyPoints[k].loc <- Hk loc of the first n Match records, in place (ssrlcv_hip_matches_apply_homography); a None side is
    left alone; a record that does not map gets invalid = 1.  Asynchronous on the current stream."""
    assert matches_d.dtype == torch.uint8 and matches_d.is_cuda and matches_d.is_contiguous() and matches_d.numel() >= 40 * n
    check(LIB.ssrlcv_hip_matches_apply_homography(ptr(matches_d), c_u32(n), homography9(H0), homography9(H1), stream_ptr()))
    return matches_d


# ------------------------------------------------------------------ disparity post-filters
def _disparity_map(disp_d):
    assert disp_d.dim() == 2 and disp_d.dtype == torch.float32 and disp_d.is_cuda and disp_d.is_contiguous()  # read with pitch w
    return disp_d.shape


def _filter_workspace(query, w, h, workspace):
    need = int(query(c_u32(w), c_u32(h)))
    return workspace if workspace is not None and workspace.numel() >= max(need, 1) else dev_bytes(need)


def disparity_components(disp_d, max_diff, want_sizes=True, workspace=None):
    """The connected components of a disparity map (ssrlcv_hip_disparity_components; include/ssrlcv_hip.h "disparity
    post-filters" items 1-2): 4-adjacent valid pixels whose disparities differ by at most max_diff.  -> (labels, sizes or
    None), int32 (H, W) holding the uint32 bits: the smallest raster index of the pixel's component and its pixel count;
    0xFFFFFFFF and 0 for an invalid pixel.  The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    h, w = _disparity_map(disp_d)
    ws = _filter_workspace(LIB.ssrlcv_hip_disparity_components_workspace_bytes, w, h, workspace)
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    sizes = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_sizes else None
    check(LIB.ssrlcv_hip_disparity_components(ptr(disp_d), c_u32(w), c_u32(h), c_f32(max_diff), ptr(labels), ptr(sizes), ptr(ws),
                                              c_sz(ws.numel()), stream_ptr()))
    return labels, sizes


def stereo_filter_speckles(disp_d, cost_d, max_size, max_diff, workspace=None):
    """Invalidates, in place, the components of at most max_size pixels (ssrlcv_hip_stereo_filter_speckles; item 3): their
    disparity becomes STEREO_INVALID_BITS and, with a cost map (cost_d may be None), their cost 0xFFFFFFFF.
    -> (disp_d, cost_d).  Asynchronous on the current stream."""
    h, w = _disparity_map(disp_d)
    assert cost_d is None or (cost_d.shape == disp_d.shape and cost_d.dtype == torch.int32 and cost_d.is_cuda and cost_d.is_contiguous())
    assert isinstance(max_size, int) and not isinstance(max_size, bool) and 0 <= max_size <= 0xFFFFFFFF  # c_u32 would wrap it
    ws = _filter_workspace(LIB.ssrlcv_hip_stereo_filter_speckles_workspace_bytes, w, h, workspace)
    check(LIB.ssrlcv_hip_stereo_filter_speckles(ptr(disp_d), ptr(cost_d), c_u32(w), c_u32(h), c_f32(max_diff), c_u32(max_size), ptr(ws),
                                                c_sz(ws.numel()), stream_ptr()))
    return disp_d, cost_d


def stereo_filter_median(disp_d, radius):
    """The lower median over the valid pixels of the (2 radius + 1)^2 window, radius 1 or 2, of every valid pixel
    (ssrlcv_hip_stereo_filter_median; item 4); invalid pixels stay invalid.  -> a new float32 (H, W) tensor; a cost map keeps
    describing the unfiltered winners.  Asynchronous on the current stream."""
    h, w = _disparity_map(disp_d)
    assert isinstance(radius, int) and not isinstance(radius, bool) and 0 <= radius <= 0xFFFFFFFF
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    check(LIB.ssrlcv_hip_stereo_filter_median(ptr(disp_d), ptr(out), c_u32(w), c_u32(h), c_u32(radius), stream_ptr()))
    return out


# ------------------------------------------------------------------ hole filling
class FillParams(ctypes.Structure):
    _fields_ = [("paths", c_u32), ("maxGap", c_u32), ("minHits", c_u32), ("rule", c_u32)]


FILL_MIN = 0      # rule: the smallest of the hits, the background
FILL_MEDIAN = 1   # rule: their lower median
FILL_NO_LIMIT = 0xFFFFFFFF  # max_gap: a source counts however far away it is


def stereo_fill_holes(disp_d, paths, max_gap, min_hits, rule, want_mask=False, workspace=None):
    """Fills the holes of a disparity map (ssrlcv_hip_stereo_fill_holes; include/ssrlcv_hip.h "hole filling"): a hole takes the
    smallest (rule = FILL_MIN) or the lower median (FILL_MEDIAN) of the first measured pixels within max_gap steps along the
    directions of the bit mask `paths` (semi-global matching's numbering), if at least min_hits directions have one.  Out of
    place: -> (a new float32 (H, W) tensor, mask or None); the mask is uint8 (H, W), 1 at the holes that got a value.  A cost
    map is not touched.  The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    h, w = _disparity_map(disp_d)
    for v in (paths, max_gap, min_hits, rule):
        assert isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 0xFFFFFFFF  # c_u32 would wrap it
    p = FillParams(paths, max_gap, min_hits, rule)
    need = int(LIB.ssrlcv_hip_stereo_fill_holes_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(p)))
    ws = workspace if workspace is not None and workspace.numel() >= max(need, 1) else dev_bytes(max(need, 1))
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    mask = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_mask else None
    check(LIB.ssrlcv_hip_stereo_fill_holes(ptr(disp_d), ptr(out), ptr(mask), c_u32(w), c_u32(h), ctypes.byref(p), ptr(ws), c_sz(ws.numel()),
                                           stream_ptr()))
    return out, mask


# ------------------------------------------------------------------ disparity mesh
class MeshParams(ctypes.Structure):
    _fields_ = [("step", c_u32), ("maxJump", c_f32)]


def mesh_grid(w, h, step):
    """(gw, gh): the nodes of the `step` grid of a (h, w) map, the grid of stereo_matches"""
    return ((w - 1) // step + 1 if w else 0), ((h - 1) // step + 1 if h else 0)


def _mesh_maps(vertex_index_d, cells_d):
    """the two maps of a mesh -> (gw, gh): vertex_index int32 (gh, gw) holding the uint32 bits, cells uint8 (gh - 1, gw - 1)"""
    assert vertex_index_d.dim() == 2 and vertex_index_d.dtype == torch.int32 and vertex_index_d.is_cuda and vertex_index_d.is_contiguous()
    gh, gw = vertex_index_d.shape
    assert cells_d.dtype == torch.uint8 and cells_d.is_cuda and cells_d.is_contiguous()
    assert tuple(cells_d.shape) == (max(gh - 1, 0), max(gw - 1, 0))
    return gw, gh


def disparity_mesh(disp_d, step, max_jump):
    """The triangle mesh of a disparity map over the `step` grid (ssrlcv_hip_disparity_mesh; include/ssrlcv_hip.h "disparity
    mesh" items 1-3).  -> (vertex_index int32 (gh, gw) holding the uint32 bits: a valid node's record index in stereo_matches'
    output, -1 (UINT32_MAX) for an invalid one; cells uint8 (gh - 1, gw - 1); count int32 [1] device tensor: the number of
    vertices).  Asynchronous on the current stream."""
    h, w = _disparity_map(disp_d)
    assert isinstance(step, int) and not isinstance(step, bool) and 0 <= step <= 0xFFFFFFFF  # c_u32 would wrap it
    p = MeshParams(step, float(max_jump))
    gw, gh = mesh_grid(w, h, step) if step else (0, 0)
    ws = dev_bytes(int(LIB.ssrlcv_hip_disparity_mesh_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(p))))
    vertex_index = torch.empty((gh, gw), dtype=torch.int32, device="cuda")
    cells = torch.empty((max(gh - 1, 0), max(gw - 1, 0)), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_disparity_mesh(ptr(disp_d), c_u32(w), c_u32(h), ctypes.byref(p), ptr(vertex_index), ptr(cells), ptr(count), ptr(ws),
                                        c_sz(ws.numel()), stream_ptr()))
    return vertex_index, cells, count


def mesh_select(vertex_index_d, cells_d, n_vertices, kept_index_d):
    """Restricts a mesh, IN PLACE, to the vertices kept_index_d names (ssrlcv_hip_mesh_select; item 6): int32 device tensor of old
    vertex indices, strictly ascending; old vertex kept_index[j] becomes j, every other node -1, and a triangle that loses a
    corner goes.  -> (vertex_index_d, cells_d).  Asynchronous on the current stream."""
    gw, gh = _mesh_maps(vertex_index_d, cells_d)
    assert kept_index_d.dim() == 1 and kept_index_d.dtype == torch.int32 and kept_index_d.is_cuda and kept_index_d.is_contiguous()
    ws = dev_bytes(int(LIB.ssrlcv_hip_mesh_select_workspace_bytes(c_u32(n_vertices))))
    check(LIB.ssrlcv_hip_mesh_select(ptr(vertex_index_d), ptr(cells_d), c_u32(gw), c_u32(gh), c_u32(n_vertices), ptr(kept_index_d),
                                     c_u32(kept_index_d.numel()), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return vertex_index_d, cells_d


def mesh_triangles(vertex_index_d, cells_d, capacity=None):
    """The emitted triangles of a mesh as vertex index triples, in cell raster order, T0 before T1 (ssrlcv_hip_mesh_triangles;
    item 4).  -> (faces int32 (min(count, capacity), 3), count).  capacity defaults to two triangles a cell.  One
    synchronisation (the count)."""
    gw, gh = _mesh_maps(vertex_index_d, cells_d)
    cap = 2 * cells_d.numel() if capacity is None else int(capacity)
    ws = dev_bytes(int(LIB.ssrlcv_hip_mesh_triangles_workspace_bytes(c_u32(gw), c_u32(gh))))
    out = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_mesh_triangles(ptr(vertex_index_d), ptr(cells_d), c_u32(gw), c_u32(gh), ptr(out) if cap else c_vp(0), c_u32(cap),
                                        ptr(count), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    n = int(count.item())
    return out[: min(n, cap)], n


def mesh_normals(points_d, vertex_index_d, cells_d, out=None):
    """Unit normals of a mesh's vertices from the triangles around them, facing the camera (ssrlcv_hip_mesh_normals; item 5).
    points_d: (n, 3) float32 device tensor.  -> float32 (n, 3): zeros first, then the vertices of the map with an index below n;
    into `out` (which is not cleared) when given.  Asynchronous on the current stream."""
    gw, gh = _mesh_maps(vertex_index_d, cells_d)
    p, n = _cloud(points_d)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device="cuda") if out is None else out
    assert nrm.dtype == torch.float32 and nrm.is_cuda and nrm.is_contiguous() and nrm.numel() >= 3 * n
    check(LIB.ssrlcv_hip_mesh_normals(ptr(p), c_u32(n), ptr(vertex_index_d), ptr(cells_d), c_u32(gw), c_u32(gh), ptr(nrm), stream_ptr()))
    return nrm


# ------------------------------------------------------------------ surface model
class DsmFrame(ctypes.Structure):
    """ssrlcv_dsm_frame: cell (i, j) covers origin + a ex + b ey, i cell <= a < (i + 1) cell, j cell <= b < (j + 1) cell; heights
    are measured along ez"""
    _fields_ = [("origin", c_f32 * 3), ("ex", c_f32 * 3), ("ey", c_f32 * 3), ("ez", c_f32 * 3), ("cell", c_f32), ("w", c_u32), ("h", c_u32)]

    @classmethod
    def make(cls, origin, ex, ey, ez, cell, w, h):
        vec = lambda v: (c_f32 * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])  # noqa: E731
        return cls(vec(origin), vec(ex), vec(ey), vec(ez), float(np.float32(cell)), int(w), int(h))


assert ctypes.sizeof(DsmFrame) == 60

DSM_MAX, DSM_MIN = 0, 1                          # dsm_rasterize's rule
DSM_FUSE_MIN, DSM_FUSE_MEDIAN, DSM_FUSE_MAX = 0, 1, 2   # dsm_fuse's rule


def dsm_rasterize(points_d, frame, rule=DSM_MAX, want_source=True, want_count=True, workspace=None):
    """A cloud into the height map of `frame` (ssrlcv_hip_dsm_rasterize; include/ssrlcv_hip.h "surface model" item 1): per cell
    the greatest (rule DSM_MAX) or least (DSM_MIN) height of its points.  points_d: (n, 3) float32 device tensor.
    -> (height float32 (h, w), 0x7FC00000 for an empty cell; source int32 (h, w) holding the uint32 bits: the winner's index, -1
    for an empty cell; count int32 (h, w)); source and count are None unless asked for.  The workspace is reused if it is large
    enough.  Asynchronous on the current stream."""
    p, n = _cloud(points_d)
    w, h = int(frame.w), int(frame.h)
    ws = _filter_workspace(LIB.ssrlcv_hip_dsm_rasterize_workspace_bytes, w, h, workspace)
    height = torch.empty((h, w), dtype=torch.float32, device="cuda")
    source = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_source else None
    count = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_count else None
    check(LIB.ssrlcv_hip_dsm_rasterize(ptr(p) if n else c_vp(0), c_u32(n), ctypes.byref(frame), c_u32(rule), ptr(height), ptr(source), ptr(count),
                                       ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return height, source, count


def dsm_fuse(maps, min_views=1, max_spread=float("inf"), rule=DSM_FUSE_MEDIAN, want_views=True):
    """Up to 8 height maps of one grid fused per cell (ssrlcv_hip_dsm_fuse; item 2): a cell with at least min_views valid entries
    whose largest and smallest differ by at most max_spread takes the smallest (DSM_FUSE_MIN), the lower median
    (DSM_FUSE_MEDIAN) or the largest (DSM_FUSE_MAX) of them.  -> (a new float32 (h, w) tensor, views uint8 (h, w) or None: the
    number of valid entries).  Asynchronous on the current stream."""
    maps = list(maps)
    assert maps, "at least one map"
    h, w = _disparity_map(maps[0])
    for m in maps:
        assert _disparity_map(m) == (h, w), "the maps share one grid"
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    views = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_views else None
    arr = (c_vp * len(maps))(*[m.data_ptr() for m in maps])
    check(LIB.ssrlcv_hip_dsm_fuse(arr, c_u32(len(maps)), c_u32(w), c_u32(h), c_u32(min_views), c_f32(max_spread), c_u32(rule), ptr(out), ptr(views),
                                  stream_ptr()))
    return out, views


def dsm_points(height_d, frame, capacity=None):
    """The valid cells of a height map as world-frame points, in raster order: the vertex numbering disparity_mesh gives the same
    map at step 1 (ssrlcv_hip_dsm_points; item 3).  -> (points float32 (min(count, capacity), 3), count).  capacity defaults to
    the grid's size.  One synchronisation (the count)."""
    h, w = _disparity_map(height_d)
    assert (h, w) == (int(frame.h), int(frame.w)), "the map has the frame's grid"
    cap = w * h if capacity is None else int(capacity)
    ws = dev_bytes(int(LIB.ssrlcv_hip_dsm_points_workspace_bytes(c_u32(w), c_u32(h))))
    out = torch.empty((cap, 3), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_dsm_points(ptr(height_d), ctypes.byref(frame), ptr(out) if cap else c_vp(0), c_u32(cap), ptr(count), ptr(ws),
                                    c_sz(ws.numel()), stream_ptr()))
    n = int(count.item())
    return out[: min(n, cap)], n


# ------------------------------------------------------------------ ortho-image
class OrthoView(ctypes.Structure):
    """ssrlcv_ortho_view: a source image and its camera as the ortho-image reads it (made by dsm_ortho_view)"""
    _fields_ = [("image", c_vp), ("w", c_u32), ("h", c_u32), ("M", c_f32 * 9), ("pos", c_f32 * 3), ("eye", c_f32 * 3)]


class OrthoParams(ctypes.Structure):
    _fields_ = [("maxSteps", c_u32), ("bias", c_f32), ("rule", c_u32)]


assert ctypes.sizeof(OrthoView) == 80 and ctypes.sizeof(OrthoParams) == 12

ORTHO_FIRST, ORTHO_MEDIAN = 0, 1   # dsm_ortho's rule
ORTHO_NO_VIEW = 0xFF               # which: no view sees the cell


def dsm_ortho_view(cam, frame):
    """ssrlcv_dsm_ortho_view_host of one Image::Camera record over the grid of `frame` (host arithmetic: needs no GPU) -> an
    OrthoView whose image pointer is NULL."""
    raw = camera_bytes(cam)
    out = OrthoView()
    check(LIB.ssrlcv_dsm_ortho_view_host(raw.ctypes.data_as(c_vp), ctypes.byref(frame), ctypes.byref(out)))
    return out


def dsm_ortho(height_d, frame, views, images, max_steps, bias, rule, want_seen=True, want_which=True, workspace=None):
    """The ortho-image of a height map (ssrlcv_hip_dsm_ortho; include/ssrlcv_hip.h "ortho-image"): every valid cell's grey from the
    first (ORTHO_FIRST) of `views` that sees it, or the lower median (ORTHO_MEDIAN) of those that do, a view seeing a cell if the
    cell projects into its image and no height within max_steps cells towards the camera stands more than `bias` above the line
    of sight.  views: 1 to 8 OrthoView; images: their uint8 (h, w) device tensors.  -> (ortho uint8 (h, w); seen uint8 (h, w), bit
    k = view k sees the cell; which uint8 (h, w), the view the grey came from, ORTHO_NO_VIEW for none); seen and which are None
    unless asked for.  The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    h, w = _disparity_map(height_d)
    assert (h, w) == (int(frame.h), int(frame.w)), "the map has the frame's grid"
    views, images = list(views), list(images)
    assert len(views) == len(images), "one image a view"
    arr = (OrthoView * max(len(views), 1))()
    for k, (v, img) in enumerate(zip(views, images)):
        assert img.dim() == 2 and img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous()   # read with pitch w
        assert tuple(img.shape) == (int(v.h), int(v.w)), "the image has the view's size"
        ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(v), ctypes.sizeof(OrthoView))
        arr[k].image = img.data_ptr()
    need = int(LIB.ssrlcv_hip_dsm_ortho_workspace_bytes(c_u32(w), c_u32(h), c_u32(len(views))))
    ws = workspace if workspace is not None and workspace.numel() >= need else dev_bytes(need)
    params = OrthoParams(int(max_steps), float(bias), int(rule))
    ortho = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    seen = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_seen else None
    which = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_which else None
    check(LIB.ssrlcv_hip_dsm_ortho(ptr(height_d), ctypes.byref(frame), arr, c_u32(len(views)), ctypes.byref(params), ptr(ortho), ptr(seen), ptr(which),
                                   ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return ortho, seen, which


# ------------------------------------------------------------------ surface accuracy
class DiffStatsParams(ctypes.Structure):
    """ssrlcv_diff_stats_params: y = x - center (fabsf of it with absolute), quantiles in parts per 10000"""
    _fields_ = [("center", c_f32), ("absolute", c_u32), ("numQuantiles", c_u32), ("quantile", c_u32 * 8)]


class DiffStats(ctypes.Structure):
    """ssrlcv_diff_stats: the record ssrlcv_hip_difference_stats writes"""
    _fields_ = [("n", c_u32), ("valid", c_u32), ("finite", c_u32), ("reserved", c_u32), ("sum", ctypes.c_double), ("sumSq", ctypes.c_double),
                ("min", c_f32), ("max", c_f32), ("quantile", c_f32 * 8)]


assert ctypes.sizeof(DiffStatsParams) == 44 and ctypes.sizeof(DiffStats) == 72


def dsm_difference(points_d, height_d, frame, cells_d=None, out=None):
    """The signed height difference of every point of a cloud to a reference height map (ssrlcv_hip_dsm_difference;
    include/ssrlcv_hip.h "surface accuracy" item 1): to the height of the cell under the point (cells_d None), or to the triangle
    of the reference's mesh under it (cells_d: disparity_mesh's `cells` of height_d at step 1).  points_d: (n, 3) float32 device
    tensor.  -> float32 (n,), 0x7FC00000 where there is no difference; into `out` when given.  Asynchronous on the current
    stream."""
    p, n = _cloud(points_d)
    h, w = _disparity_map(height_d)
    assert (h, w) == (int(frame.h), int(frame.w)), "the map has the frame's grid"
    if cells_d is not None:
        assert cells_d.dtype == torch.uint8 and cells_d.is_cuda and cells_d.is_contiguous()
        assert tuple(cells_d.shape) == (max(h - 1, 0), max(w - 1, 0)), "the cells of the same map at step 1"
        if cells_d.numel() == 0:
            cells_d = dev_bytes(1)   # a grid without a cell is still MESH mode (no point is inside): the pointer must not be NULL
    diff = torch.empty((n,), dtype=torch.float32, device="cuda") if out is None else out
    assert diff.dtype == torch.float32 and diff.is_cuda and diff.is_contiguous() and diff.numel() >= n
    check(LIB.ssrlcv_hip_dsm_difference(ptr(p) if n else c_vp(0), c_u32(n), ptr(height_d), ctypes.byref(frame), ptr(cells_d), ptr(diff), stream_ptr()))
    return diff


def difference_stats(values_d, center=0.0, absolute=False, quantiles=(), workspace=None):
    """Exact statistics of a float32 device tensor of differences (ssrlcv_hip_difference_stats; "surface accuracy" item 2): the
    valid entries (bits not 0x7FC00000) become y = x - center, |y| with `absolute`; over the finite y: count, float64 sum and sum of
    squares, min, max and up to 8 quantiles (parts per 10000, each one of the inputs).  -> a DiffStats record on the host.  The
    workspace is reused if it is large enough.  One synchronisation (the record)."""
    assert values_d.dtype == torch.float32 and values_d.is_cuda and values_d.is_contiguous()
    n = values_d.numel()
    quantiles = [int(q) for q in quantiles]
    assert len(quantiles) <= 8 and all(0 <= q <= 0xFFFFFFFF for q in quantiles)   # c_u32 would wrap them
    params = DiffStatsParams(float(center), int(bool(absolute)), len(quantiles), (c_u32 * 8)(*quantiles))
    need = int(LIB.ssrlcv_hip_difference_stats_workspace_bytes(c_u32(n), ctypes.byref(params)))
    ws = workspace if workspace is not None and workspace.numel() >= need else dev_bytes(need)
    out = torch.empty(ctypes.sizeof(DiffStats), dtype=torch.uint8, device="cuda")
    check(LIB.ssrlcv_hip_difference_stats(ptr(values_d) if n else c_vp(0), c_u32(n), ctypes.byref(params), ptr(out), ptr(ws), c_sz(ws.numel()),
                                          stream_ptr()))
    return DiffStats.from_buffer_copy(out.cpu().numpy().tobytes())


# ------------------------------------------------------------------ surface registration
class RegisterPose(ctypes.Structure):
    """ssrlcv_register_pose: p' = M p + T, m = [M | T] 3 x 4 row-major; pivot: the point steps rotate and scale about"""
    _fields_ = [("m", c_f32 * 12), ("pivot", c_f32 * 3)]

    @classmethod
    def make(cls, matrix=None, translation=(0, 0, 0), pivot=(0, 0, 0)):
        m = np.zeros((3, 4), np.float32)
        m[:, :3] = np.eye(3) if matrix is None else np.asarray(matrix, np.float64).reshape(3, 3)
        m[:, 3] = np.asarray(translation, np.float64).reshape(3)
        return cls((c_f32 * 12)(*m.reshape(12).tolist()), (c_f32 * 3)(*[float(np.float32(x)) for x in pivot]))


class RegisterParams(ctypes.Structure):
    """ssrlcv_register_params: a point is used iff fabsf(d - center) <= gate"""
    _fields_ = [("center", c_f32), ("gate", c_f32)]


class RegisterTerms(ctypes.Structure):
    """ssrlcv_register_terms: the record ssrlcv_hip_register_terms writes"""
    _fields_ = [("n", c_u32), ("inside", c_u32), ("used", c_u32), ("reserved", c_u32), ("jtj", ctypes.c_double * 28), ("jte", ctypes.c_double * 7),
                ("ee", ctypes.c_double)]


assert ctypes.sizeof(RegisterPose) == 60 and ctypes.sizeof(RegisterParams) == 8 and ctypes.sizeof(RegisterTerms) == 304

REGISTER_SHIFT, REGISTER_RIGID, REGISTER_SIMILARITY = 0x07, 0x3F, 0x7F   # register_step's dof masks: bits tx, ty, tz, rx, ry, rz, scale


def register_terms(points_d, pose, height_d, frame, cells_d, center=0.0, gate=float("inf"), workspace=None):
    """The normal equations of one point-to-plane step of a cloud under `pose` towards a reference height map
    (ssrlcv_hip_register_terms; include/ssrlcv_hip.h "surface registration" item 1).  points_d: (n, 3) float32 device tensor;
    cells_d: disparity_mesh's `cells` of height_d at step 1 (required: the reference is its mesh); a point takes part iff it has
    a difference d to the mesh and |d - center| <= gate.  -> a RegisterTerms record on the host.  The workspace is reused if it
    is large enough.  One synchronisation (the record)."""
    p, n = _cloud(points_d)
    h, w = _disparity_map(height_d)
    assert (h, w) == (int(frame.h), int(frame.w)), "the map has the frame's grid"
    assert cells_d is not None and cells_d.dtype == torch.uint8 and cells_d.is_cuda and cells_d.is_contiguous()
    assert tuple(cells_d.shape) == (max(h - 1, 0), max(w - 1, 0)), "the cells of the same map at step 1"
    if cells_d.numel() == 0:
        cells_d = dev_bytes(1)   # a grid without a cell: no point is inside, and the pointer must not be NULL
    params = RegisterParams(float(center), float(gate))
    need = int(LIB.ssrlcv_hip_register_terms_workspace_bytes(c_u32(n)))
    ws = workspace if workspace is not None and workspace.numel() >= max(need, 1) else dev_bytes(max(need, 1))
    out = torch.empty(ctypes.sizeof(RegisterTerms), dtype=torch.uint8, device="cuda")
    check(LIB.ssrlcv_hip_register_terms(ptr(p) if n else c_vp(0), c_u32(n), ctypes.byref(pose), ptr(height_d), ctypes.byref(frame), ptr(cells_d),
                                        ctypes.byref(params), ptr(out), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return RegisterTerms.from_buffer_copy(out.cpu().numpy().tobytes())


def transform_points(points_d, pose, out=None):
    """A pose applied to a cloud (ssrlcv_hip_transform_points; "surface registration" item 2): p' = M p + T; a "no result" point
    ((0, 0, 0) or a non-finite component) is copied bit for bit.  -> float32 (n, 3); into `out` when given, which may be
    points_d itself.  Asynchronous on the current stream."""
    p, n = _cloud(points_d)
    res = torch.empty((n, 3), dtype=torch.float32, device="cuda") if out is None else out
    assert res.dtype == torch.float32 and res.is_cuda and res.is_contiguous() and res.numel() >= 3 * n
    check(LIB.ssrlcv_hip_transform_points(ptr(p) if n else c_vp(0), c_u32(n), ctypes.byref(pose), ptr(res) if n else c_vp(0), stream_ptr()))
    return res


def register_step(terms, dof_mask=REGISTER_RIGID, damping=0.0):
    """ssrlcv_register_step_host (host arithmetic: needs no GPU): H delta = -jte over the masked unknowns, H = jtj with its
    diagonal times (1 + damping).  -> delta, float64 (7,) (tx, ty, tz, rx, ry, rz, scale; 0 where unmasked), or None where the
    system has no answer (no point used, or a direction the points do not hold)."""
    delta = (ctypes.c_double * 7)()
    rc = LIB.ssrlcv_register_step_host(ctypes.byref(terms), c_u32(int(dof_mask)), ctypes.c_double(float(damping)), delta)
    if rc == -4:   # SSRLCV_ERR_UNSUPPORTED
        return None
    check(rc)
    return np.array(list(delta), np.float64)


def register_compose(pose, delta):
    """ssrlcv_register_compose_host (host arithmetic): the pose after the step p'' = pivot + (1 + ds) R(dw) (p' - pivot) + dt.
    -> a new RegisterPose with the same pivot."""
    d = (ctypes.c_double * 7)(*[float(x) for x in delta])
    out = RegisterPose()
    check(LIB.ssrlcv_register_compose_host(ctypes.byref(pose), d, ctypes.byref(out)))
    return out


# ------------------------------------------------------------------ mesh render
class RenderParams(ctypes.Structure):
    """ssrlcv_render_params: a triangle whose bounding box is wider or higher than maxExtent pixels is skipped"""
    _fields_ = [("maxExtent", c_u32)]


assert ctypes.sizeof(RenderParams) == 4

RENDER_NO_TRIANGLE = 0xFFFFFFFF   # triangle: nothing was drawn at the pixel


def mesh_render(points_d, vertex_index_d, cells_d, view, grey_d=None, max_extent=8, want_triangle=True, want_shade=True, workspace=None):
    """A grid mesh drawn into a pinhole view (ssrlcv_hip_mesh_render; include/ssrlcv_hip.h "mesh render" item 1).  points_d: (n, 3)
    float32 device tensor, the vertices' world positions; vertex_index_d, cells_d: the maps of disparity_mesh (after mesh_select
    too); view: an OrthoView (dsm_ortho_view's), of which M, pos, w and h are read; grey_d: uint8 (n,) device tensor, one grey a
    vertex, or None (every grey 0).  -> (depth float32 (h, w), 0x7FC00000 where nothing was drawn; triangle int32 (h, w) holding
    the uint32 bits: 2 cell + t, -1 (RENDER_NO_TRIANGLE) for none; shade uint8 (h, w); counts int32 [3] device tensor: triangles
    drawn, skipped as larger than max_extent pixels, skipped for an unusable corner or a zero area); triangle and shade are None
    unless asked for.  The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    gw, gh = _mesh_maps(vertex_index_d, cells_d)
    p, n = _cloud(points_d)
    if grey_d is not None:
        assert grey_d.dtype == torch.uint8 and grey_d.is_cuda and grey_d.is_contiguous() and grey_d.numel() == n, "one grey a vertex"
    assert isinstance(max_extent, int) and not isinstance(max_extent, bool) and 0 <= max_extent <= 0xFFFFFFFF   # c_u32 would wrap it
    w, h = int(view.w), int(view.h)
    need = int(LIB.ssrlcv_hip_mesh_render_workspace_bytes(c_u32(n), c_u32(w), c_u32(h)))
    ws = workspace if workspace is not None and workspace.numel() >= max(need, 1) else dev_bytes(need)
    params = RenderParams(max_extent)
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    triangle = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_triangle else None
    shade = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_shade else None
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_mesh_render(ptr(p) if n else c_vp(0), c_u32(n), ptr(grey_d) if n else c_vp(0), ptr(vertex_index_d) if gw * gh else c_vp(0),
                                     ptr(cells_d) if cells_d.numel() else c_vp(0), c_u32(gw), c_u32(gh), ctypes.byref(view), ctypes.byref(params),
                                     ptr(depth), ptr(triangle), ptr(shade), ptr(counts), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return depth, triangle, shade, counts


def image_residual(image_d, shade_d, depth_d, out=None):
    """A view's own pixels minus the rendered ones (ssrlcv_hip_image_residual; "mesh render" item 2): float32 (h, w),
    (float)image - (float)shade where depth is valid and 0x7FC00000 elsewhere -- the form difference_stats takes.  image_d,
    shade_d: uint8 (h, w) device tensors; depth_d: mesh_render's.  Into `out` when given.  Asynchronous on the current stream."""
    h, w = _disparity_map(depth_d)
    for t in (image_d, shade_d):
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (h, w), "the image, the shade and the depth share one view"
    res = torch.empty((h, w), dtype=torch.float32, device="cuda") if out is None else out
    assert res.dtype == torch.float32 and res.is_cuda and res.is_contiguous() and res.numel() >= w * h
    check(LIB.ssrlcv_hip_image_residual(ptr(image_d), ptr(shade_d), ptr(depth_d), c_u32(w), c_u32(h), ptr(res), stream_ptr()))
    return res


# ------------------------------------------------------------------ surface simplification
def dsm_simplify_errors(height_d, out=None):
    """The error map of a height map's right-triangle hierarchy (ssrlcv_hip_dsm_simplify_errors; include/ssrlcv_hip.h "surface
    simplification" item 1): float32 (h, w), per split node the largest midpoint error in its subtree, +inf where a triangle
    cannot be formed.  Computed once; dsm_simplify_mesh extracts a mesh at any tolerance from it.  Into `out` when given.
    Asynchronous on the current stream."""
    h, w = _disparity_map(height_d)
    err = torch.empty((h, w), dtype=torch.float32, device="cuda") if out is None else out
    assert err.dtype == torch.float32 and err.is_cuda and err.is_contiguous() and err.numel() >= w * h
    check(LIB.ssrlcv_hip_dsm_simplify_errors(ptr(height_d), c_u32(w), c_u32(h), ptr(err), stream_ptr()))
    return err


def dsm_simplify_mesh(height_d, error_d, tolerance, node_index_d=None, capacity=None, kept_capacity=None, workspace=None):
    """The simplified mesh of a height map at `tolerance` (ssrlcv_hip_dsm_simplify_mesh; items 2 and 3).  error_d:
    dsm_simplify_errors' map of height_d.  node_index_d: int32 (h, w) or None; `kept` then holds raster indices.
    -> (faces int32 (min(count, capacity), 3): new vertex indices; n_faces; kept int32 (min(n_vertices, kept_capacity),): per new
    vertex its node's entry of node_index_d; n_vertices; vertex_index int32 (h, w) holding the uint32 bits: a kept node's new index,
    -1 elsewhere).  capacity defaults to the full-resolution mesh, kept_capacity to the grid.  One synchronisation (the counts)."""
    h, w = _disparity_map(height_d)
    assert _disparity_map(error_d) == (h, w), "the error map has the height map's grid"
    if node_index_d is not None:
        assert node_index_d.dtype == torch.int32 and node_index_d.is_cuda and node_index_d.is_contiguous() and tuple(node_index_d.shape) == (h, w)
    cap = 2 * max(w - 1, 0) * max(h - 1, 0) if capacity is None else int(capacity)
    kcap = w * h if kept_capacity is None else int(kept_capacity)
    ws = _filter_workspace(LIB.ssrlcv_hip_dsm_simplify_mesh_workspace_bytes, w, h, workspace)
    faces = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    kept = torch.empty(kcap, dtype=torch.int32, device="cuda")
    vertex_index = torch.empty((h, w), dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    check(LIB.ssrlcv_hip_dsm_simplify_mesh(ptr(height_d), ptr(error_d), c_u32(w), c_u32(h), c_f32(tolerance), ptr(node_index_d), ptr(vertex_index),
                                           ptr(faces) if cap else c_vp(0), c_u32(cap), c_vp(counts.data_ptr()), ptr(kept) if kcap else c_vp(0),
                                           c_u32(kcap), c_vp(counts.data_ptr() + 4), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    nt, nv = (int(c) for c in counts.cpu().tolist())
    return faces[: min(nt, cap)], nt, kept[: min(nv, kcap)], nv, vertex_index


# ------------------------------------------------------------------ terrain filter
class TerrainParams(ctypes.Structure):
    _fields_ = [("levels", c_u32), ("radius", c_u32 * 8), ("threshold", c_f32 * 8)]


MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3
MORPH_WHOLE_MAP = 0xFFFFFFFF  # radius: the window is the whole map


def dsm_morphology(height_d, radius, op, out=None, workspace=None):
    """Grey-scale morphology of a height map with the clipped square window of `radius` cells (ssrlcv_hip_dsm_morphology;
    include/ssrlcv_hip.h "terrain filter" item 1): MORPH_ERODE takes the smallest valid value of the window, MORPH_DILATE the
    largest, MORPH_OPEN the dilation of the erosion and MORPH_CLOSE the erosion of the dilation, both with the holes of the input
    kept.  Selection only: every output is an input value or 0x7FC00000.  Out of place: -> a new float32 (h, w) tensor, or `out`.
    The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    h, w = _disparity_map(height_d)
    assert isinstance(radius, int) and not isinstance(radius, bool) and 0 <= radius <= 0xFFFFFFFF  # c_u32 would wrap it
    assert isinstance(op, int) and not isinstance(op, bool) and 0 <= op <= 0xFFFFFFFF
    ws = _filter_workspace(LIB.ssrlcv_hip_dsm_morphology_workspace_bytes, w, h, workspace)
    res = torch.empty((h, w), dtype=torch.float32, device="cuda") if out is None else out
    assert _disparity_map(res) == (h, w)
    check(LIB.ssrlcv_hip_dsm_morphology(ptr(height_d), ptr(res), c_u32(w), c_u32(h), c_u32(radius), c_u32(op), ptr(ws), c_sz(ws.numel()), stream_ptr()))
    return res


def dsm_terrain(height_d, radii, thresholds, want_level=True, want_opened=False, workspace=None):
    """The progressive morphological ground filter (ssrlcv_hip_dsm_terrain; item 2): the map is opened with the windows of
    `radii` (1 to 8 of them, strictly ascending) in turn, and a valid cell that level k's opening lowers by more than
    thresholds[k - 1] is an object.  -> (terrain float32 (h, w): the height's bits at the ground cells, 0x7FC00000 elsewhere;
    level uint8 (h, w) or None: 0 ground, k the first level that flagged the cell, 255 an invalid input cell; opened float32 (h, w)
    or None: the last opening).  The workspace is reused if it is large enough.  Asynchronous on the current stream."""
    h, w = _disparity_map(height_d)
    radii, thresholds = [int(r) for r in radii], [float(t) for t in thresholds]
    assert len(radii) == len(thresholds) <= 8 and all(0 <= r <= 0xFFFFFFFF for r in radii)
    p = TerrainParams(len(radii), (c_u32 * 8)(*radii), (c_f32 * 8)(*thresholds))
    ws = _filter_workspace(LIB.ssrlcv_hip_dsm_terrain_workspace_bytes, w, h, workspace)
    terrain = torch.empty((h, w), dtype=torch.float32, device="cuda")
    level = torch.empty((h, w), dtype=torch.uint8, device="cuda") if want_level else None
    opened = torch.empty((h, w), dtype=torch.float32, device="cuda") if want_opened else None
    check(LIB.ssrlcv_hip_dsm_terrain(ptr(height_d), c_u32(w), c_u32(h), ctypes.byref(p), ptr(terrain), ptr(level), ptr(opened), ptr(ws),
                                     c_sz(ws.numel()), stream_ptr()))
    return terrain, level, opened


def dsm_subtract(a_d, b_d, out=None):
    """a - b of two maps of one grid in float32 (ssrlcv_hip_dsm_subtract; item 3): 0x7FC00000 where either is invalid or the
    difference is a NaN.  height - filled terrain is the normalised surface; the result is the form difference_stats takes.
    `out` may be a_d or b_d.  Asynchronous on the current stream."""
    h, w = _disparity_map(a_d)
    assert _disparity_map(b_d) == (h, w), "both maps have one grid"
    res = torch.empty((h, w), dtype=torch.float32, device="cuda") if out is None else out
    assert _disparity_map(res) == (h, w)
    check(LIB.ssrlcv_hip_dsm_subtract(ptr(a_d), ptr(b_d), c_u32(w), c_u32(h), ptr(res), stream_ptr()))
    return res


# ------------------------------------------------------------------ surface objects
class ObjectParams(ctypes.Structure):
    """ssrlcv_object_params: a cell is a member iff it is valid and v >= minHeight; members link as disparity_components links with
    maxDiff; q = rint(v x scale); an object of fewer than minCells cells is dropped (0 behaves as 1)"""
    _fields_ = [("minHeight", c_f32), ("maxDiff", c_f32), ("scale", c_f32), ("minCells", c_u32)]


class ObjectRecord(ctypes.Structure):
    """ssrlcv_object_record: one kept object"""
    _fields_ = [("label", c_u32), ("cells", c_u32), ("minX", c_u32), ("minY", c_u32), ("maxX", c_u32), ("maxY", c_u32), ("perimeter", c_u32),
                ("clipped", c_u32), ("peakIndex", c_u32), ("peak", c_f32), ("low", c_f32), ("reserved", c_u32), ("sumX", ctypes.c_uint64),
                ("sumY", ctypes.c_uint64), ("sumXX", ctypes.c_uint64), ("sumXY", ctypes.c_uint64), ("sumYY", ctypes.c_uint64),
                ("sumQ", ctypes.c_int64), ("sumQQ", ctypes.c_uint64)]


class ObjectMeasures(ctypes.Structure):
    """ssrlcv_object_measures: what ssrlcv_object_measures_host makes of a record"""
    _fields_ = [(name, ctypes.c_double) for name in ("area", "perimeterLength", "compactness", "centroidX", "centroidY")] + \
               [("world", ctypes.c_double * 3)] + \
               [(name, ctypes.c_double) for name in ("meanHeight", "volume", "rmsHeight", "mxx", "mxy", "myy", "lambdaMajor", "lambdaMinor",
                                                     "axisX", "axisY", "elongation")]


OBJECT_RECORD = np.dtype([("label", "<u4"), ("cells", "<u4"), ("minX", "<u4"), ("minY", "<u4"), ("maxX", "<u4"), ("maxY", "<u4"),
                          ("perimeter", "<u4"), ("clipped", "<u4"), ("peakIndex", "<u4"), ("peak", "<f4"), ("low", "<f4"), ("reserved", "<u4"),
                          ("sumX", "<u8"), ("sumY", "<u8"), ("sumXX", "<u8"), ("sumXY", "<u8"), ("sumYY", "<u8"), ("sumQ", "<i8"), ("sumQQ", "<u8")])
assert ctypes.sizeof(ObjectParams) == 16 and ctypes.sizeof(ObjectRecord) == 104 == OBJECT_RECORD.itemsize and ctypes.sizeof(ObjectMeasures) == 152


def dsm_objects(objects_d, min_height, max_diff=float("inf"), min_cells=1, scale=256.0, capacity=None, want_ids=True, workspace=None):
    """The objects of an object-height map (ssrlcv_hip_dsm_objects; include/ssrlcv_hip.h "surface objects"): the 4-connected
    components of the cells that are valid and >= min_height, linked where they differ by at most max_diff; those of at least
    min_cells cells are numbered in raster order of their first cells.  capacity None: a first call with capacity 0 counts them and
    a second one writes every record; a number: one call, at most that many records.
    -> (count: the full number kept; ids int32 (h, w) holding the uint32 bits: the object's number, -1 for a cell of none, or None;
    records: an OBJECT_RECORD array of min(count, capacity)).  The workspace is reused if it is large enough.  One
    synchronisation a call (the count)."""
    h, w = _disparity_map(objects_d)
    assert isinstance(min_cells, int) and not isinstance(min_cells, bool) and 0 <= min_cells <= 0xFFFFFFFF  # c_u32 would wrap it
    assert capacity is None or (isinstance(capacity, int) and not isinstance(capacity, bool) and 0 <= capacity <= 0xFFFFFFFF)
    p = ObjectParams(float(min_height), float(max_diff), float(scale), min_cells)
    ws = _filter_workspace(LIB.ssrlcv_hip_dsm_objects_workspace_bytes, w, h, workspace)
    ids = torch.empty((h, w), dtype=torch.int32, device="cuda") if want_ids else None
    count_d = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(cap, want):
        records = torch.empty(max(cap * 13, 1), dtype=torch.int64, device="cuda")  # 104 bytes a record, 8-byte aligned
        check(LIB.ssrlcv_hip_dsm_objects(ptr(objects_d) if w * h else c_vp(0), c_u32(w), c_u32(h), ctypes.byref(p), ptr(ids) if want else c_vp(0),
                                         ptr(records) if cap else c_vp(0), c_u32(cap), ptr(count_d), ptr(ws), c_sz(ws.numel()), stream_ptr()))
        return int(count_d.cpu().numpy().view(np.uint32)[0]), records

    if capacity is None:
        capacity = call(0, False)[0]
    count, records = call(capacity, want_ids)
    got = min(count, capacity)
    return count, ids, records.cpu().numpy().view(np.uint8)[:got * 104].view(OBJECT_RECORD).copy()


def object_measures(record, frame, scale=256.0):
    """ssrlcv_object_measures_host (host arithmetic: needs no GPU): area, perimeter length, compactness, centroid in cells and on the
    frame's plane in the world, mean height, volume and RMS height, the central second moments, their eigenvalues, the major
    axis and the elongation of one record (a row of an OBJECT_RECORD array or an ObjectRecord).  -> an ObjectMeasures."""
    if not isinstance(record, ObjectRecord):
        raw = np.asarray(record, OBJECT_RECORD).reshape(1).tobytes()
        record = ObjectRecord.from_buffer_copy(raw)
    out = ObjectMeasures()
    check(LIB.ssrlcv_object_measures_host(ctypes.byref(record), ctypes.byref(frame), c_f32(float(scale)), ctypes.byref(out)))
    return out


# ------------------------------------------------------------------ shift search
class ShiftParams(ctypes.Structure):
    """ssrlcv_shift_params: q = rint(height x scale); shifts (centerX + kx, centerY + ky), kx, ky = -radius .. radius, in cells of
    the grid sampled at `stride`; a difference d takes part iff |d - centerQ| <= gateQ (SHIFT_NO_GATE: always)"""
    _fields_ = [("scale", c_f32), ("stride", c_u32), ("centerX", ctypes.c_int32), ("centerY", ctypes.c_int32), ("radius", c_u32),
                ("centerQ", ctypes.c_int32), ("gateQ", c_u32)]


class ShiftResult(ctypes.Structure):
    """ssrlcv_shift_result: the record ssrlcv_shift_pick_host writes"""
    _fields_ = [("shiftX", ctypes.c_int64), ("shiftY", ctypes.c_int64), ("subX", ctypes.c_double), ("subY", ctypes.c_double),
                ("bias", ctypes.c_double), ("variance", ctypes.c_double), ("second", ctypes.c_double), ("n", c_u32), ("candidates", c_u32)]


assert ctypes.sizeof(ShiftParams) == 28 and ctypes.sizeof(ShiftResult) == 64

SHIFT_NO_GATE = 0xFFFFFFFF
SHIFT_MAX_RADIUS = 32
SHIFT_HEAD = np.dtype([("validMoving", "<u4"), ("validReference", "<u4"), ("clippedMoving", "<u4"), ("clippedReference", "<u4")])
SHIFT_ENTRY = np.dtype([("n", "<u4"), ("reserved", "<u4"), ("sum", "<i8"), ("sumSq", "<u8")])
assert SHIFT_HEAD.itemsize == 16 and SHIFT_ENTRY.itemsize == 24


def shift_search(moving, reference, scale, stride=1, center=(0, 0), radius=8, center_q=0, gate_q=None, ws=None):
    """The differences of two height maps of one grid at every whole-cell shift of a window (ssrlcv_hip_shift_search;
    include/ssrlcv_hip.h "shift search").  moving, reference: float32 (h, w) device tensors, any NaN an invalid cell; heights are
    quantised to rint(height x scale); with `stride` g only the cells (i g, j g) take part, and center and radius are in cells
    of that sampled grid; gate_q None: no gate.  -> dict(params: the ShiftParams; head: the four counts as a SHIFT_HEAD record;
    entries: a SHIFT_ENTRY array (2 radius + 1, 2 radius + 1), [ky + radius, kx + radius] the shift center + (kx, ky); bytes: the
    table as the device wrote it).  The workspace is reused if it is large enough.  One synchronisation (the table)."""
    h, w = _disparity_map(moving)
    assert _disparity_map(reference) == (h, w), "both maps have one grid"
    ints = [int(stride), int(center[0]), int(center[1]), int(radius), int(center_q), SHIFT_NO_GATE if gate_q is None else int(gate_q)]
    assert 0 <= ints[0] <= 0xFFFFFFFF and 0 <= ints[3] <= 0xFFFFFFFF and 0 <= ints[5] <= 0xFFFFFFFF   # c_u32 would wrap them
    assert all(-(1 << 31) <= v < (1 << 31) for v in (ints[1], ints[2], ints[4]))
    params = ShiftParams(float(scale), *ints)
    size = int(LIB.ssrlcv_shift_table_bytes(c_u32(ints[3])))
    need = int(LIB.ssrlcv_hip_shift_search_workspace_bytes(c_u32(w), c_u32(h), ctypes.byref(params)))
    work = ws if ws is not None and ws.numel() >= max(need, 1) else dev_bytes(need)
    table = torch.empty(max(size, 8) // 8, dtype=torch.int64, device="cuda")       # 8-byte aligned
    check(LIB.ssrlcv_hip_shift_search(ptr(moving) if w * h else c_vp(0), ptr(reference) if w * h else c_vp(0), c_u32(w), c_u32(h), ctypes.byref(params),
                                      ptr(table), ptr(work), c_sz(work.numel()), stream_ptr()))
    raw = table.cpu().numpy().view(np.uint8)[:size].copy()
    side = 2 * ints[3] + 1
    return {"params": params, "head": raw[:16].view(SHIFT_HEAD)[0], "entries": raw[16:].view(SHIFT_ENTRY).reshape(side, side), "bytes": raw}


def shift_pick(table, params, min_overlap):
    """ssrlcv_shift_pick_host (host arithmetic: needs no GPU): among the entries with n >= max(min_overlap, 1) the shift of least
    variance of the differences, the sub-cell step from its neighbours' variances, the height bias and the runner-up outside its
    3 x 3.  table: shift_search's dictionary, or the table's bytes as a uint8 array.  -> a ShiftResult, or None when no entry
    has that many cells."""
    raw = np.ascontiguousarray(table["bytes"] if isinstance(table, dict) else table, dtype=np.uint8)
    assert 0 <= int(min_overlap) <= 0xFFFFFFFF
    out = ShiftResult()
    rc = LIB.ssrlcv_shift_pick_host(raw.ctypes.data_as(c_vp), c_sz(raw.size), ctypes.byref(params), c_u32(int(min_overlap)), ctypes.byref(out))
    if rc == -4:   # SSRLCV_ERR_UNSUPPORTED
        return None
    check(rc)
    return out


# ------------------------------------------------------------------ SIFT pipeline
class SiftPlan:
    """Owns an ssrlcv_sift_plan and (optionally) the workspace tensor for one W x H image slot."""

    def __init__(self, w, h, max_orientations=2, orientation_threshold=0.8, orientation_contrib_width=1.5,
                 descriptor_contrib_width=6.0, max_keypoints_per_octave=0, alloc=True):
        self.w, self.h = w, h
        p = SiftParams(max_orientations, orientation_threshold, orientation_contrib_width, descriptor_contrib_width,
                       max_keypoints_per_octave)
        self.handle = c_vp()
        check(LIB.ssrlcv_sift_plan_create(c_u32(w), c_u32(h), ctypes.byref(p), ctypes.byref(self.handle)))
        self.workspace_bytes = LIB.ssrlcv_sift_plan_workspace_bytes(self.handle)
        self.max_features = LIB.ssrlcv_sift_plan_max_features(self.handle)
        self.workspace = dev_bytes(self.workspace_bytes) if alloc else None
        self.features = dev_bytes(self.max_features * 152) if alloc else None
        self.num_features = torch.zeros(1, dtype=torch.int32, device="cuda") if alloc else None

    def __del__(self):
        if getattr(self, "handle", None) and LIB is not None:  # (module globals are gone at interpreter shutdown)
            LIB.ssrlcv_sift_plan_destroy(self.handle)
            self.handle = None

    def set_stop_stage(self, stage):
        LIB.ssrlcv_sift_plan_set_stop_stage(self.handle, c_int(stage))

    def set_stage_event(self, event):
        """A torch.cuda.Event (or None) that extract() records on the launching stream between the scale-space stage and the
        key-point stage (ssrlcv_sift_plan_set_stage_event): how a caller times the stages of the fused call."""
        handle = None
        if event is not None:
            event.record()           # torch creates the underlying hipEvent_t lazily, on the first record
            handle = event.cuda_event
        self._stage_event = event    # (kept alive as long as the plan refers to it)
        check(LIB.ssrlcv_sift_plan_set_stage_event(self.handle, c_vp(handle) if handle is not None else None))

    def build_dog(self, pixels_d):
        check(LIB.ssrlcv_hip_sift_build_dog(self.handle, ptr(pixels_d), ptr(self.workspace), stream_ptr()))

    def describe(self):
        check(LIB.ssrlcv_hip_sift_describe(self.handle, ptr(self.workspace), ptr(self.features),
                                           ptr(self.num_features), stream_ptr()))

    def stage(self, stage):
        """One reference launch site of the key-point stage (ssrlcv_hip_sift_stage), on the state the previous one left."""
        check(LIB.ssrlcv_hip_sift_stage(self.handle, ptr(self.workspace), c_int(stage), ptr(self.features),
                                        ptr(self.num_features), stream_ptr()))

    def extract(self, pixels_d):
        check(LIB.ssrlcv_hip_sift_extract(self.handle, ptr(pixels_d), ptr(self.workspace), ptr(self.features),
                                          ptr(self.num_features), stream_ptr()))

    def count(self):
        """Feature count of the last extract; raises when a key-point list outgrew its capacity (the list was truncated:
        not the reference's result -- re-run with a larger max_keypoints_per_octave)."""
        mask = c_u32(0)
        rc = LIB.ssrlcv_sift_plan_overflow(self.handle, ptr(self.workspace), ctypes.byref(mask), stream_ptr())
        if mask.value:
            raise SsrlcvError("key-point capacity exceeded in octaves %s" % [o for o in range(4) if mask.value >> o & 1])
        check(rc)
        return int(self.num_features.item())

    def overflow_mask(self):
        mask = c_u32(0)
        LIB.ssrlcv_sift_plan_overflow(self.handle, ptr(self.workspace), ctypes.byref(mask), stream_ptr())
        return mask.value

    def level(self, kind, octave, blur):
        """-> (numpy level copy, (min, max)); kind 0 = raw DoG, 1 = gaussian (last octave built)."""
        data, mm = c_vp(), c_vp()
        w, h = c_u32(), c_u32()
        check(LIB.ssrlcv_sift_plan_level(self.handle, ptr(self.workspace), c_int(kind), c_int(octave), c_int(blur),
                                         ctypes.byref(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(mm)))
        torch.cuda.synchronize()
        base = self.workspace.data_ptr()
        off = data.value - base
        n = w.value * h.value
        lvl = self.workspace[off: off + 4 * n].view(torch.float32).cpu().numpy().reshape(h.value, w.value).copy()
        moff = mm.value - base
        mmv = self.workspace[moff: moff + 8].view(torch.float32).cpu().numpy().copy()
        return lvl, (float(mmv[0]), float(mmv[1]))

    def keypoints(self, octave, dtype):
        """-> (SSKeyPoint numpy array of the octave, blur indices [6])"""
        lst, idx = c_vp(), c_vp()
        check(LIB.ssrlcv_sift_plan_keypoints(self.handle, ptr(self.workspace), c_int(octave), ctypes.byref(lst),
                                             ctypes.byref(idx)))
        torch.cuda.synchronize()
        base = self.workspace.data_ptr()
        ioff = idx.value - base
        state = self.workspace[ioff: ioff + 32].view(torch.int32).cpu().numpy().copy()
        n = int(state[5]) if int(state[6]) else 0
        loff = lst.value - base
        kps = to_host(self.workspace[loff: loff + 32 * max(n, 1)], dtype, n)
        return kps, state[:6].copy(), int(state[7])

    def features_host(self, dtype):
        n = self.count()
        return to_host(self.features[: 152 * max(n, 1)], dtype, n)
