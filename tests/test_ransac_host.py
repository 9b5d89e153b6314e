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


def test_refit_eigh_matches_svd():
    """refit() (eigenvector of the normal matrix, the contract's form) and ransac()'s SVD of the rows give one F."""
    matches, _, truth = R.synthetic(2000, seed=3)
    q, t, valid = R.split(matches)
    cq, ct, s = R.normalisation(q, t, valid)
    mask = truth["inlier"]
    _, _, vt = np.linalg.svd(R.rows((q[mask] - cq) * s, (t[mask] - ct) * s))
    F_svd = R.to_pixel(R.rank2(vt[8].reshape(3, 3)), cq, ct, s)
    F_eigh = R.refit(matches, mask)
    assert np.abs(F_svd - F_eigh).max() < 1e-9
    assert R.sampson_gap(F_svd, F_eigh, q[mask], t[mask]) < 1e-9


def test_best_slot_is_lowest_of_the_largest():
    assert R.best_slot([0, 5, 3, 5, 5]) == (1, 5)
    assert R.best_slot([7]) == (0, 7)
    assert R.best_slot([0, 0, 0]) == (None, 0)


def test_axis_rotations_invert_rot():
    rng = np.random.default_rng(4)
    a = np.stack([rng.uniform(-np.pi, np.pi, 200), rng.uniform(-1.39, 1.39, 200), rng.uniform(-np.pi, np.pi, 200)], 1)
    for x in np.concatenate([a, [[0.0, 0.0, 0.0], [0.1, -0.6, 2.5], [-3.0, 1.39, -3.1]]]):
        assert np.abs(R.axis_rotations(R.rot(x)) - x).max() < 1e-12, x


def test_draws_needed_matches_sample_indices():
    """the vectorised hash of the 64-draw cap search agrees with sample_indices, sample by sample"""
    d = R.draws_needed(0, 65536, 7)
    assert (d == 64).any() and (d == 65).any()  # seed 0 at n = 7 reaches both sides of the cap
    for h in list(range(64)) + list(np.flatnonzero((d >= 63) & (d <= 66))):
        idx = R.sample_indices(0, int(h), 7)
        assert (idx is not None) == (1 <= d[h] <= 64), (h, d[h])
    d2 = R.draws_needed(2 ** 64 - 1, 256, 50)
    for h in range(256):
        assert (R.sample_indices(2 ** 64 - 1, h, 50) is not None) == (1 <= d2[h] <= 64)


def test_pose6_recovers_exact_poses():
    """pose6 of the exact F of each pose gives back its angles and its scaled baseline direction (float64)."""
    for name, (angles, C) in R.POSES.items():
        matches, cams, truth = R.synthetic(2000, seed=11, outliers=0.0, angles=angles, C=C)
        F = R.F_of_pose(truth["Rp"], truth["C"], R.K_of(cams[0:1]), R.K_of(cams[1:2]))
        p = R.pose6(F, matches, None, cams)
        assert np.abs(p[:3] - np.asarray(angles)).max() < 1e-12, (name, p)
        length = np.linalg.norm(cams["cam_pos"][1].astype(np.float64) - cams["cam_pos"][0]) / 1000.0
        assert np.abs(p[3:] - truth["C"] / np.linalg.norm(truth["C"]) * length).max() < 1e-12 * length, (name, p)


def test_householder_null_space():
    """householder_null spans the 7x9 system's null space with an orthonormal pair, and solve7 finds the same F in
    either basis (only the parameter, and so the order of the roots, depends on it)."""
    matches, _, truth = R.synthetic(500, seed=5)
    q, t, valid = R.split(matches)
    cq, ct, s = R.normalisation(q, t, valid)
    for h in range(50):
        idx = R.sample_indices(0, h, 500)
        qn, tn = (q[idx] - cq) * s, (t[idx] - ct) * s
        F1, F2 = R.householder_null(R.rows(qn, tn))
        N = np.stack([F1.reshape(-1), F2.reshape(-1)])
        assert np.abs(R.rows(qn, tn) @ N.T).max() < 1e-12 and np.abs(N @ N.T - np.eye(2)).max() < 1e-12
        a, near_a = R.solve7(qn, tn)
        b, near_b = R.solve7(qn, tn, householder=True)
        assert len(a) == len(b) or near_a or near_b
        if len(a) == len(b):
            ua = [F.reshape(-1) / np.linalg.norm(F) for F in a]
            for F in b:
                f = F.reshape(-1) / np.linalg.norm(F)
                assert min(min(np.linalg.norm(f - g), np.linalg.norm(f + g)) for g in ua) < 1e-6
