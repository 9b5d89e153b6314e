"""Fundamental-matrix RANSAC on the MI355X (ssrlcv_hip_fmatrix_ransac / _score / pose_from_fmatrix, csrc/ransac.hip),
held to the float64 restatement of tests/ransac_ref.py and to synthetic ground truth (parity unpinned)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import ransac_ref as R

pytestmark = pytest.mark.gpu
THR = 2.0


@pytest.fixture(scope="module")
def scenes():
    return {n: R.synthetic(n, seed=n % 97 + 1) for n in (500, 20000, 300000)}


def _run(capi, matches, samples=1024, seed=0, thr=THR):
    md = capi.to_dev(matches)
    return md, capi.fmatrix_ransac(md, len(matches), samples, thr, seed, mask=True, candidates=True)


@pytest.mark.parametrize("n", [500, 20000])
def test_samples_and_minimal_solver(capi, scenes, n):
    matches, _, _ = scenes[n]
    _, out = _run(capi, matches)
    q, t, valid = R.split(matches)
    cq, ct, s = R.normalisation(q, t, valid)
    cand, counts = out["candidates"].reshape(-1, 3, 9), out["counts"].reshape(-1, 3)
    mismatched, near_count, far, total = 0, 0, 0, 0
    for h in range(len(cand)):
        idx = R.sample_indices(0, h, n)
        filled = np.abs(cand[h]).sum(1) > 0
        assert np.all(counts[h][~filled] == 0)
        assert np.all(filled[: filled.sum()])  # slots fill from r = 0
        ref, near = R.solve7((q[idx] - cq) * s, (t[idx] - ct) * s)
        near_count += near
        if filled.sum() != len(ref):
            assert near, (h, filled.sum(), len(ref))
            mismatched += 1
        for F in cand[h][filled]:
            d = np.sqrt(R.sampson_d2(F, q[idx], t[idx]).max())
            assert d < 5e-2  # the float32 rounding of a pixel F of a near-degenerate sample: measured up to 1.25e-2 px
            far += d >= 1e-2
            total += 1
            assert abs(np.linalg.det(R.to_normalised(F, cq, ct, s))) < 1e-4
            f = F.reshape(-1)
            assert f[np.argmax(np.abs(f))] > 0 and abs(np.linalg.norm(f.astype(np.float64)) - 1) < 1e-5
    assert near_count <= 0.005 * len(cand), near_count
    assert far <= 0.01 * total, (far, total)


@pytest.mark.parametrize("n", [500, 20000, 300000])
def test_scoring_matches_float64(capi, scenes, n):
    matches, _, _ = scenes[n]
    md, out = _run(capi, matches)
    q, t, valid = R.split(matches)
    cand, counts = out["candidates"], out["counts"]
    filled = np.flatnonzero(np.abs(cand).sum(1) > 0)
    pick = filled[:: max(1, len(filled) // 200)]  # every candidate at the small sizes, ~200 of them at 3e5
    for i in pick:
        d2 = R.sampson_d2(cand[i], q, t)
        ref = int(np.sum((d2 < THR * THR) & valid))
        # t~^T F q~ cancels in float32: near the threshold it is ~s thr = 1e-3 of its terms, so d^2 carries ~2e-4
        # relative error (measured: one match of one candidate at 3e5 outside a 1e-4 band)
        band = int(np.sum(np.abs(d2 - THR * THR) <= 1e-3 * THR * THR))
        assert abs(int(counts[i]) - ref) <= band, (i, counts[i], ref, band)
    again, _ = capi.fmatrix_score(md, n, cand, THR)
    assert np.array_equal(again, counts)
    c1, m1 = capi.fmatrix_score(md, n, out["F"], THR, mask=True)
    assert c1[0] == out["count"] == int(out["mask"].sum()) and np.array_equal(m1, out["mask"])


@pytest.mark.parametrize("n", [500, 20000, 300000])
def test_recovers_synthetic_geometry(capi, scenes, n):
    matches, cams, truth = scenes[n]
    md, out = _run(capi, matches)
    mask = out["mask"].astype(bool)
    inl = truth["inlier"]
    recall, precision = (mask & inl).sum() / inl.sum(), (mask & inl).sum() / max(1, mask.sum())
    assert recall >= 0.98 and precision >= 0.98, (recall, precision)
    best = out["counts"].max()
    assert out["count"] >= best  # the refit is kept only when it does at least as well
    f = out["F"].reshape(-1)
    assert f[np.argmax(np.abs(f))] > 0 and abs(np.linalg.norm(f.astype(np.float64)) - 1) < 1e-5
    mask_d = capi.to_dev(out["mask"])
    pose = capi.pose_from_fmatrix(md, n, mask_d, out["F"], cams[0:1], cams[1:2])
    Rp = R.rot(pose[:3].astype(np.float64))
    assert R.rotation_error_deg(Rp, truth["Rp"]) <= 0.5, pose
    assert R.angle_deg(pose[3:].astype(np.float64), truth["C"]) <= 2.0, pose
    assert abs(np.linalg.norm(pose[3:]) - np.linalg.norm(truth["C"])) <= 1e-4 * np.linalg.norm(truth["C"])


def test_bit_equal_across_calls(capi, scenes):
    matches, _, _ = scenes[20000]
    _, a = _run(capi, matches, seed=7)
    _, b = _run(capi, matches, seed=7)
    for k in ("F", "mask", "candidates", "counts"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["count"] == b["count"]


def test_edge_cases(capi):
    matches, _, _ = R.synthetic(7, seed=5, outliers=0.0)
    for n in (0, 1, 6):
        md = capi.to_dev(matches[:n]) if n else capi.dev_bytes(40)
        out = capi.fmatrix_ransac(md, n, 64, THR, mask=n > 0, candidates=True)
        assert out["count"] == 0 and not out["F"].any() and not out["counts"].any() and not out["candidates"].any()
    bad = R.synthetic(500, seed=6)[0]
    bad["invalid"] = 1
    out = capi.fmatrix_ransac(capi.to_dev(bad), 500, 256, THR, mask=True, candidates=True)
    assert out["count"] == 0 and not out["F"].any() and not out["mask"].any() and not out["counts"].any()
    out = capi.fmatrix_ransac(capi.to_dev(matches), 7, 64, THR, mask=True, candidates=True)
    assert out["counts"].max() == 7 and out["count"] == 7 and out["mask"].all()
    # invalid matches are never inliers and never sampled
    some = R.synthetic(2000, seed=8)[0]
    some["invalid"][::3] = 1
    out = capi.fmatrix_ransac(capi.to_dev(some), 2000, 512, THR, mask=True, candidates=True)
    assert out["count"] > 0 and not out["mask"][::3].any()
    for h in range(512):
        idx = R.sample_indices(0, h, 2000)
        if idx is not None and some["invalid"][idx].any():
            assert not out["candidates"][3 * h:3 * h + 3].any()


def test_real_tie_points():
    """The reference's Pipeline2View stage-0 tie points: RANSAC finds at least 95 % of the consensus of the F the
    cameras themselves imply (narrow-FOV satellite geometry is near-affine: no pose assertion)."""
    from ssrlcv_amd import capi
    v = H.load_view("Pipeline2View")
    m = H.matches_from_matchset(v["kp0"])
    md = capi.to_dev(m)
    Fc = R.F_of_cameras(v["cameras"])
    Fc = (Fc / np.linalg.norm(Fc)).astype(np.float32)
    c_cam = int(capi.fmatrix_score(md, len(m), Fc, THR)[0][0])
    out = capi.fmatrix_ransac(md, len(m), 4096, THR)
    assert c_cam > 0 and out["count"] >= 0.95 * c_cam, (out["count"], c_cam, len(m))


def test_pose_estimator_ransac_through_class_api(tmp_path, scenes):
    """PoseEstimator::estimatePoseRANSAC (tests/cpp/pose_ransac_test.cpp) on the synthetic pair, then LM_optimize from
    that pose: angles within the bound of the recovery test, LM does not raise the cost."""
    matches, cams, truth = scenes[20000]
    path = str(tmp_path / "pair.bin")
    with open(path, "wb") as f:
        f.write(np.uint64(len(matches)).tobytes() + cams.tobytes() + matches.tobytes())
    exe = os.path.join(H.ROOT, "ssrlcv_amd", "host", "_build", "pose_ransac_test")
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "csrc"), "release"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "host"), "_build/pose_ransac_test"])
    out = subprocess.check_output([exe, path]).decode()
    vals = {}
    for line in out.splitlines():
        if line.startswith("ransac ") or line.startswith("lm "):
            key, *nums = line.split()
            vals[key] = np.array([float(x) for x in nums])
    assert "ok" in out.splitlines()[-1], out
    inliers, pose = vals["ransac"][0], vals["ransac"][1:]
    assert inliers >= 0.98 * truth["inlier"].sum()
    assert R.rotation_error_deg(R.rot(pose[:3]), truth["Rp"]) <= 0.5, pose
    assert R.angle_deg(pose[3:], truth["C"]) <= 2.0, pose
    cost_start, cost_end = vals["lm"]
    assert cost_end <= cost_start, (cost_start, cost_end)
