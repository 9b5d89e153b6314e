"""Fundamental-matrix RANSAC without a GPU: the C ABI exports it, sizes its workspace and refuses bad arguments before any
device work; the float64 restatement the GPU tests hold it to (tests/ransac_ref.py) recovers a synthetic two-view
geometry (parity unpinned: the reference has no fixture for this path)."""
import ctypes

import numpy as np

import ransac_ref as R

NEW = ("ssrlcv_hip_fmatrix_ransac_workspace_bytes", "ssrlcv_hip_fmatrix_ransac", "ssrlcv_hip_fmatrix_score",
       "ssrlcv_hip_pose_from_fmatrix")
INVALID_ARG, WORKSPACE = -1, -3


def _lib():
    from ssrlcv_amd import _lib
    return _lib.load()


def test_ransac_symbols_are_exported():
    from ssrlcv_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.ssrlcv_hip_abi_version() == 4


def test_workspace_grows_with_samples():
    ws = _lib().ssrlcv_hip_fmatrix_ransac_workspace_bytes
    sizes = [ws(ctypes.c_uint32(13534), ctypes.c_uint32(s)) for s in (1, 1024, 4096, 16384)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[2] >= 4096 * (27 * 4 + 3 * 4)  # candidates and their counts


def _ransac(lib, matches, n, samples, thr, ws, wsb, F, cnt):
    v = ctypes.c_void_p
    return lib.ssrlcv_hip_fmatrix_ransac(v(matches), ctypes.c_uint32(n), ctypes.c_uint32(samples), ctypes.c_float(thr),
                                         ctypes.c_uint64(0), v(ws), ctypes.c_size_t(wsb), v(F), v(cnt), v(0), v(0),
                                         v(0), v(0))


def test_argument_checks_come_before_device_work():
    """Bogus (never dereferenced) pointers: every check below must return before the first HIP call."""
    lib = _lib()
    P = 1 << 20  # not a valid device pointer: a call that got past its checks would fault, not return a status
    need = lib.ssrlcv_hip_fmatrix_ransac_workspace_bytes(ctypes.c_uint32(100), ctypes.c_uint32(64))
    assert _ransac(lib, 0, 100, 64, 1.0, P, need, P, P) == INVALID_ARG      # matches NULL
    assert _ransac(lib, P, 100, 64, 1.0, P, need, 0, P) == INVALID_ARG      # F_out NULL
    assert _ransac(lib, P, 100, 64, 1.0, P, need, P, 0) == INVALID_ARG      # count NULL
    assert _ransac(lib, P, 100, 0, 1.0, P, need, P, P) == INVALID_ARG       # numSamples == 0
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert _ransac(lib, P, 100, 64, thr, P, need, P, P) == INVALID_ARG, thr
    assert _ransac(lib, P, 100, 64, 1.0, P, need - 1, P, P) == WORKSPACE
    v = ctypes.c_void_p
    score = lib.ssrlcv_hip_fmatrix_score
    assert score(v(0), ctypes.c_uint32(10), v(P), ctypes.c_uint32(1), ctypes.c_float(1.0), v(P), ctypes.c_size_t(256),
                 v(P), v(0), v(0)) == INVALID_ARG
    assert score(v(P), ctypes.c_uint32(10), v(P), ctypes.c_uint32(2), ctypes.c_float(1.0), v(P), ctypes.c_size_t(256),
                 v(P), v(P), v(0)) == INVALID_ARG  # a mask only for k == 1
    assert score(v(P), ctypes.c_uint32(10), v(P), ctypes.c_uint32(1), ctypes.c_float(1.0), v(P), ctypes.c_size_t(255),
                 v(P), v(0), v(0)) == WORKSPACE
    cam = np.zeros(80, np.uint8)
    pose = np.zeros(6, np.float32)
    assert lib.ssrlcv_hip_pose_from_fmatrix(v(P), ctypes.c_uint32(10), v(0), v(0), cam.ctypes.data_as(v),
                                            cam.ctypes.data_as(v), v(P), ctypes.c_size_t(256), pose.ctypes.data_as(v),
                                            v(0)) == INVALID_ARG


def test_sample_hash_is_splitmix64():
    """Sample 0, seed 0, draw 0 is splitmix64's first output; the indices are distinct and in range."""
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
    z ^= z >> 31
    assert z == 0xE220A8397B1DCDAF  # splitmix64(seed 0), first value
    idx = R.sample_indices(0, 0, 1000)
    assert idx[0] == ((z >> 32) * 1000) >> 32 and len(set(idx)) == 7 and max(idx) < 1000
    assert R.sample_indices(0, 0, 7) is None or sorted(R.sample_indices(0, 0, 7)) == list(range(7))


def test_reference_recovers_synthetic_geometry():
    matches, cams, truth = R.synthetic(2000, seed=3)
    F, mask = R.ransac(matches, 1024, 2.0)
    inl = truth["inlier"]
    recall = (mask & inl).sum() / inl.sum()
    precision = (mask & inl).sum() / mask.sum()
    assert recall >= 0.98 and precision >= 0.98, (recall, precision)
    q, t, _ = R.split(matches)
    Rp, C = R.pose_from_F(F, q, t, mask, R.K_of(cams[0:1]), R.K_of(cams[1:2]))
    assert R.rotation_error_deg(Rp, truth["Rp"]) <= 0.5
    assert R.angle_deg(C, truth["C"]) <= 2.0
    # the true F passes the same inliers (the scene is what the tests think it is)
    Ft = R.F_of_pose(truth["Rp"], truth["C"], R.K_of(cams[0:1]), R.K_of(cams[1:2]))
    assert (R.inliers(Ft, q, t, matches["invalid"] == 0, 2.0) & inl).sum() >= 0.99 * inl.sum()
