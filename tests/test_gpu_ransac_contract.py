"""Fundamental-matrix RANSAC and pose from F (csrc/ransac.hip) held clause by clause to the contract of include/ssrlcv_hip.h
("fundamental-matrix RANSAC and relative pose"): slot order, the 64-bit sample hash and its 64-draw cap, the best pick and
the refit rule, the valid-only normalisation, degenerate input, the scoring kernel's tile edges and the pose, each
against the float64 restatement of tests/ransac_ref.py (parity unpinned: the contract is the definition)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import ransac_ref as R

pytestmark = pytest.mark.gpu
THR = 2.0

# Measured on the MI355X (the largest value seen over every case of the test that uses it):
SLOT_TOL = 2e-6       # slot r against reference root r, unit normalised F, Frobenius: 2.3e-7
REFIT_TOL = 5e-4      # refit against the float64 refit, max |Sampson distance difference| over the inliers, px: 7.6e-5
ANGLE_TOL = 4e-7      # pose angles against pose6, rad: 4.0e-8
DIR_TOL = 3e-7        # pose direction against pose6, rad: 2.6e-8
TIE_ANGLE_TOL = 1e-7  # Pipeline2View pose against the cameras' relative pose, rad: 2.7e-10 (a few float32 ulps of 0.17)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _unit(F, ref=None):
    """F (any shape of 9) as a unit vector; with `ref`, the sign that points it along ref"""
    f = np.asarray(F, np.float64).reshape(-1)
    f = f / np.linalg.norm(f)
    return f if ref is None or np.dot(f, ref) >= 0 else -f


# ---------------------------------------------------------------------------------------------- a. slot order, solver
SEEDS = (0, 7, 2 ** 32 + 5, 2 ** 64 - 1)


def slot_distances(capi, n, seed):
    """-> (distance of every filled slot r to reference root r, slots checked for order, near samples) after the checks
    of test_slot_order_and_solver at one (n, seed)"""
    matches = R.synthetic(n, seed=n % 97 + 1)[0]
    md = capi.to_dev(matches)
    q, t, valid = R.split(matches)
    cq, ct, s = R.normalisation(q, t, valid)
    full = capi.fmatrix_ransac(md, n, 1000, THR, seed, candidates=True)
    for S in (1, 63, 64, 65):  # sample h does not depend on numSamples
        part = capi.fmatrix_ransac(md, n, S, THR, seed, candidates=True)
        assert _bits(part["candidates"]) == _bits(full["candidates"][:3 * S]), (seed, S)
        assert np.array_equal(part["counts"], full["counts"][:3 * S]), (seed, S)
    cand = full["candidates"].reshape(-1, 3, 9)
    dist, ordered, near_samples = [], 0, 0
    for h in range(len(cand)):
        filled = np.abs(cand[h]).sum(1) > 0
        assert np.all(filled[: filled.sum()]), h  # slots fill from r = 0
        idx = R.sample_indices(seed, h, n)
        if idx is None:
            assert not filled.any(), h
            continue
        ref, near = R.solve7((q[idx] - cq) * s, (t[idx] - ct) * s, householder=True)
        near_samples += near
        if filled.sum() != len(ref):
            assert near, (seed, h, filled.sum(), len(ref))
            continue
        refs = [_unit(F) for F in ref]
        for r in range(len(ref)):
            g = _unit(R.to_normalised(cand[h][r], cq, ct, s))
            d = [np.linalg.norm(_unit(x, g) - g) for x in refs]
            dist.append(d[r])
            if not near:
                assert int(np.argmin(d)) == r, (seed, h, r, d)  # ascending roots: slot r is root r
                ordered += 1
    return np.array(dist), ordered, near_samples


@pytest.mark.parametrize("n", [500, 20000])
def test_slot_order_and_solver(capi, n):
    """samples + solver: sample h of a 64-bit seed draws sample_indices(seed, h), whatever numSamples is; its real roots
    fill slots 3h + r in ascending order, each within SLOT_TOL of the float64 root (near-double roots: no order check)."""
    for seed in SEEDS:
        dist, ordered, near = slot_distances(capi, n, seed)
        assert ordered >= 1000 and near <= 10, (seed, ordered, near)
        assert dist.max() <= SLOT_TOL, (seed, dist.max())


# ---------------------------------------------------------------------------------------------- b. the 64-draw cap
CAP_SAMPLES = 65536  # at n = 7 about (6/7)^63 ~ 6e-5 of the samples need exactly 64 draws


def cap_seed():
    """-> (seed, draws) of the first seed at n = 7 with a sample complete on draw 64 and one that would be on draw 65
    (at n = 8 and 9 neither occurs within 65536 samples)"""
    for seed in range(64):
        d = R.draws_needed(seed, CAP_SAMPLES, 7)
        if (d == 64).any() and (d == 65).any():
            return seed, d
    raise AssertionError("no seed reaches both sides of the cap")


def test_64_draw_cap(capi):
    """samples: 7 distinct indices within 64 draws, else no candidate.  Seven matches, so every sample that completes
    solves the same system: its slots are filled exactly when the reference completes it within 64 draws."""
    seed, d = cap_seed()
    matches = R.synthetic(7, seed=5, outliers=0.0)[0]
    out = capi.fmatrix_ransac(capi.to_dev(matches), 7, CAP_SAMPLES, THR, seed, candidates=True)
    filled = np.abs(out["candidates"].reshape(CAP_SAMPLES, 27)).sum(1) > 0
    expect = (d >= 1) & (d <= 64)
    assert np.array_equal(filled, expect), np.flatnonzero(filled != expect)[:10]
    assert not filled[d == 65].any() and filled[d == 64].all()


# ---------------------------------------------------------------------------------------------- c. best pick and refit
def _scene(name):
    if name == "normal":
        return R.synthetic(20000, seed=20000 % 97 + 1)[0], THR
    if name == "clean":  # every good candidate and the refit pass all matches: the refit ties the best
        return R.synthetic(500, seed=13, outliers=0.0, noise=0.05)[0], THR
    return R.synthetic(60, seed=15, noise=0.5)[0], 0.02  # "ties": most candidates pass just their own 7 matches


def best_and_refit(capi, matches, thr, samples=1024):
    """-> dict of the RANSAC run, its best slot b, b's inlier mask, the float64 refit on it, and which branch held"""
    n = len(matches)
    md = capi.to_dev(matches)
    out = capi.fmatrix_ransac(md, n, samples, thr, 0, mask=True, candidates=True)
    counts, cand = out["counts"], out["candidates"]
    b, cb = R.best_slot(counts)
    assert b is not None
    cnt_b, mask_b = capi.fmatrix_score(md, n, cand[b], thr, mask=True)
    assert cnt_b[0] == cb
    Fr = R.refit(matches, mask_b)
    q, t, _ = R.split(matches)
    inl = mask_b.astype(bool)
    F = out["F"].reshape(-1)
    res = dict(out=out, md=md, b=b, cb=cb, mask_b=inl, Fr=Fr, kept_candidate=_bits(F) == _bits(cand[b]),
               gap=R.sampson_gap(F, Fr, q[inl], t[inl]))
    c1, m1 = capi.fmatrix_score(md, n, F, thr, mask=True)  # count and mask are those of F_out
    assert c1[0] == out["count"] == int(out["mask"].sum()) and np.array_equal(m1, out["mask"])
    return res


@pytest.mark.parametrize("scene", ["normal", "clean", "ties"])
def test_best_pick_and_refit_rule(capi, scene):
    """best + refit: b = the lowest slot with the largest count.  Either F_out is candidate b bit for bit and the refit
    on b's inliers scores below counts[b] (the float64 refit, up to the matches its REFIT_TOL gap and the 1e-3 scoring
    band can move across the threshold), or F_out is that refit (within REFIT_TOL) with count >= counts[b]."""
    matches, thr = _scene(scene)
    r = best_and_refit(capi, matches, thr)
    out, cb = r["out"], r["cb"]
    q, t, valid = R.split(matches)
    if r["kept_candidate"]:
        Fr32 = r["Fr"].astype(np.float32)
        cr = int(capi.fmatrix_score(r["md"], len(matches), Fr32, thr)[0][0])
        d = np.sqrt(R.sampson_d2(Fr32, q, t))
        band = int(np.sum(valid & (np.abs(d - thr) <= REFIT_TOL + 1e-3 * thr)))
        assert cr < cb + band, (cr, cb, band)
        assert out["count"] == cb
    else:
        assert r["gap"] <= REFIT_TOL and out["count"] >= cb, (r["gap"], out["count"], cb)
    counts = out["counts"]
    if scene == "ties":  # the lowest-slot rule decides F_out
        assert r["kept_candidate"] and int(np.sum(counts == cb)) >= 2, np.sum(counts == cb)
    if scene == "clean":  # the `>=` of the refit rule decides F_out
        assert not r["kept_candidate"] and out["count"] == cb == len(matches), (out["count"], cb)
    if scene == "normal":
        assert not r["kept_candidate"] and out["count"] >= cb


# ---------------------------------------------------------------------------------------------- d. refit vs float64
def refit_gaps(capi, n):
    """-> (GPU refit vs float64 refit, runner-up refit vs float64 refit): max Sampson-distance gaps over b's inliers"""
    matches = R.synthetic(n, seed=n % 97 + 1)[0]
    r = best_and_refit(capi, matches, THR)
    assert not r["kept_candidate"], n  # the refit is kept on this scene
    q, t, _ = R.split(matches)
    cand, counts = r["out"]["candidates"], r["out"]["counts"]
    for c in np.argsort(-counts.astype(np.int64), kind="stable")[1:]:  # the runner-up: the next slot with other inliers
        m2 = capi.fmatrix_score(r["md"], n, cand[c], THR, mask=True)[1].astype(bool)
        if not np.array_equal(m2, r["mask_b"]):
            break
    inl = r["mask_b"]
    return r["gap"], R.sampson_gap(R.refit(matches, m2), r["Fr"], q[inl], t[inl])


@pytest.mark.parametrize("n", [500, 20000, 300000])
def test_refit_matches_float64(capi, n):
    """refit: the least-squares 8-point fit on the best candidate's inliers, against the float64 eigh refit of the
    same mask; REFIT_TOL is at least 10x below the gap to the refit on the runner-up candidate's inliers."""
    gap, runner_up = refit_gaps(capi, n)
    assert gap <= REFIT_TOL and 10 * REFIT_TOL <= runner_up, (gap, runner_up)


# ---------------------------------------------------------------------------------------------- e. only valid matches
def test_only_valid_matches_count(capi):
    """normalise + inlier: the boxes come from the valid matches only and an invalid match is never an inlier or a sample,
    so moving the invalid matches to NaN, +-1e30 and negative locations changes no output bit."""
    matches = R.synthetic(3000, seed=21)[0]
    matches["invalid"][1::3] = 1
    moved = matches.copy()
    inv = np.flatnonzero(matches["invalid"])
    junk = np.array([[np.nan, np.nan], [1e30, -1e30], [-1e30, 1e30], [-250.0, -4000.0], [1e30, 1e30], [-3.0, np.nan]],
                    np.float32)
    moved["kp0_loc"][inv] = junk[np.arange(len(inv)) % len(junk)]
    moved["kp1_loc"][inv] = junk[(np.arange(len(inv)) + 2) % len(junk)]
    a = capi.fmatrix_ransac(capi.to_dev(matches), 3000, 1024, THR, 3, mask=True, candidates=True)
    b = capi.fmatrix_ransac(capi.to_dev(moved), 3000, 1024, THR, 3, mask=True, candidates=True)
    assert a["count"] > 0 and a["count"] == b["count"]
    for k in ("F", "mask", "candidates", "counts"):
        assert _bits(a[k]) == _bits(b[k]), k
    Fs = np.concatenate([a["F"].reshape(1, 9), a["candidates"][:300]])
    for k in (1, len(Fs)):
        ca, ma = capi.fmatrix_score(capi.to_dev(matches), 3000, Fs[:k], THR, mask=k == 1)
        cb, mb = capi.fmatrix_score(capi.to_dev(moved), 3000, Fs[:k], THR, mask=k == 1)
        assert np.array_equal(ca, cb) and (k > 1 or np.array_equal(ma, mb))


# ---------------------------------------------------------------------------------------------- f. pose vs float64
def _pose_case(name, n=2000):
    angles, C = R.POSES[name]
    matches, cams, truth = R.synthetic(n, seed=11, outliers=0.0, angles=angles, C=C)
    F = R.F_of_pose(truth["Rp"], truth["C"], R.K_of(cams[0:1]), R.K_of(cams[1:2]))
    return matches, cams, R.to_pixel(F, np.zeros(2), np.zeros(2), 1.0).astype(np.float32)


def pose_errors(capi, name):
    """-> (max angle error, direction error in rad, relative length error) of pose_from_fmatrix against pose6"""
    matches, cams, F32 = _pose_case(name)
    pose = capi.pose_from_fmatrix(capi.to_dev(matches), len(matches), None, F32, cams[0:1], cams[1:2]).astype(np.float64)
    ref = R.pose6(F32.astype(np.float64), matches, None, cams)
    length = np.linalg.norm(cams["cam_pos"][1].astype(np.float64) - cams["cam_pos"][0]) / 1000.0
    return (np.abs(pose[:3] - ref[:3]).max(), np.radians(R.angle_deg(pose[3:], ref[3:])),
            abs(np.linalg.norm(pose[3:]) - length) / length)


@pytest.mark.parametrize("name", list(R.POSES))
def test_pose_matches_float64(capi, name):
    """pose: the vote winner among the four (R, C), getAxisRotations of its rotation, unit C times |dcam_pos| / 1000;
    the exact F of each pose (rounded to float32) against pose6 of the same F."""
    da, dc, dl = pose_errors(capi, name)
    assert da <= ANGLE_TOL and dc <= DIR_TOL and dl <= 1e-6, (da, dc, dl)


def test_pose_input_conventions(capi):
    """pose: mask NULL = every valid match (= an all-ones mask); invalid matches take no part in the vote; F and -F are
    one pose; F all zero is SSRLCV_ERR_INVALID_ARG."""
    matches, cams, F32 = _pose_case("default")
    n = len(matches)
    md = capi.to_dev(matches)
    ref = capi.pose_from_fmatrix(md, n, None, F32, cams[0:1], cams[1:2])
    ones = capi.to_dev(np.ones(n, np.uint8))
    assert _bits(capi.pose_from_fmatrix(md, n, ones, F32, cams[0:1], cams[1:2])) == _bits(ref)
    assert _bits(capi.pose_from_fmatrix(md, n, None, -F32, cams[0:1], cams[1:2])) == _bits(ref)
    # invalid matches of points behind both cameras, three times as many as the valid ones: counted, they would hand
    # the vote to the (R, -C) decomposition
    angles, C = R.POSES["default"]
    rng = np.random.default_rng(2)
    z = -rng.uniform(10.0, 30.0, 3 * n)
    X = np.stack([rng.uniform(-1, 1, 3 * n) * z * 0.4, rng.uniform(-1, 1, 3 * n) * z * 0.4, z], 1)
    qh, th = X @ R.K_of(cams[0:1]).T, ((X - np.asarray(C)) @ R.rot(angles)) @ R.K_of(cams[1:2]).T
    junk = np.zeros(3 * n, H.MATCH)
    junk["invalid"] = 1
    junk["kp0_loc"], junk["kp1_loc"] = qh[:, :2] / qh[:, 2:], th[:, :2] / th[:, 2:]
    both = np.concatenate([matches, junk])[rng.permutation(4 * n)]
    counted = both.copy()
    counted["invalid"] = 0
    assert np.abs(R.pose6(F32.astype(np.float64), counted, None, cams)[3:]
                  + R.pose6(F32.astype(np.float64), matches, None, cams)[3:]).max() < 1e-6  # the junk flips C
    bd = capi.to_dev(both)
    assert _bits(capi.pose_from_fmatrix(bd, 4 * n, None, F32, cams[0:1], cams[1:2])) == _bits(ref)
    all_ones = capi.to_dev(np.ones(4 * n, np.uint8))
    assert _bits(capi.pose_from_fmatrix(bd, 4 * n, all_ones, F32, cams[0:1], cams[1:2])) == _bits(ref)
    with pytest.raises(capi.SsrlcvError, match="status -1"):
        capi.pose_from_fmatrix(md, n, None, np.zeros(9, np.float32), cams[0:1], cams[1:2])


def tie_point_pose_error(capi):
    v = H.load_view("Pipeline2View")
    m = H.matches_from_matchset(v["kp0"])
    Fc = R.F_of_cameras(v["cameras"])
    Fc = (Fc / np.linalg.norm(Fc)).astype(np.float32)
    pose = capi.pose_from_fmatrix(capi.to_dev(m), len(m), None, Fc, v["cameras"][0:1], v["cameras"][1:2])
    rel = H.relative_pose(v["cameras"]).astype(np.float64)
    length = np.linalg.norm(rel[3:])
    return np.abs(pose[:3] - rel[:3]).max(), np.radians(R.angle_deg(pose[3:], rel[3:])), \
        abs(np.linalg.norm(pose[3:]) - length) / length


def test_real_tie_points_pose(capi):
    """pose on the reference's Pipeline2View stage-0 tie points: the F the cameras imply gives back the cameras'
    relative pose (H.relative_pose; a float64 emulation of the vote splits 13534 / 0 / 0 / 0)."""
    da, dc, dl = tie_point_pose_error(capi)
    assert da <= TIE_ANGLE_TOL and dc <= TIE_ANGLE_TOL and dl <= 1e-6, (da, dc, dl)


# ---------------------------------------------------------------------------------------------- g. degenerate input
def _degenerate(name):
    m = R.synthetic(500, seed=31)[0]
    rng = np.random.default_rng(32)
    if name == "six_valid":
        m["invalid"] = 1
        m["invalid"][[3, 50, 100, 200, 300, 499]] = 0
    elif name == "one_point_pair":  # the valid matches share one location pair; the invalid ones spread
        m["invalid"][::3] = 1
        ok = m["invalid"] == 0
        m["kp0_loc"][ok], m["kp1_loc"][ok] = (1000.5, 2000.25), (1500.0, 700.0)
    elif name == "one_query_point":
        m["kp0_loc"] = (1234.5, 987.25)
    elif name == "collinear":
        x = rng.uniform(0, 4000, 500)
        m["kp0_loc"] = np.stack([x, 0.5 * x + 100], 1)
        m["kp1_loc"] = np.stack([0.8 * x + 10, 3000 - 0.6 * x + rng.normal(0, 0.5, 500)], 1)
    elif name == "planar":  # points on one plane: every sample's 7x9 system has a 3-dimensional null space
        cams = R.synthetic_cameras()
        Kq, Kt, Rp = R.K_of(cams[0:1]), R.K_of(cams[1:2]), R.rot(R.TRUE_ANGLES)
        u = rng.uniform(-0.3, 0.3, (500, 2))
        X = np.stack([u[:, 0] * 20, u[:, 1] * 20, 20 + 4 * u[:, 0]], 1)
        qh, th = X @ Kq.T, ((X - R.TRUE_C) @ Rp) @ Kt.T
        m["kp0_loc"], m["kp1_loc"] = qh[:, :2] / qh[:, 2:], th[:, :2] / th[:, 2:]
    return m


@pytest.mark.parametrize("name", ["six_valid", "one_point_pair", "one_query_point", "collinear", "planar"])
def test_degenerate_input(capi, name):
    """fewer than 7 valid matches or a zero extent: count 0, F zero; otherwise degenerate geometry still gives finite
    outputs, unit-norm sign-fixed candidates, and a count and mask that are F_out's own."""
    m = _degenerate(name)
    n = len(m)
    md = capi.to_dev(m)
    out = capi.fmatrix_ransac(md, n, 512, THR, 0, mask=True, candidates=True)
    cand = out["candidates"]
    assert np.isfinite(out["F"]).all() and np.isfinite(cand).all()
    filled = np.abs(cand).sum(1) > 0
    for f in cand[filled]:
        assert abs(np.linalg.norm(f.astype(np.float64)) - 1) < 1e-5 and f[np.argmax(np.abs(f))] > 0
    assert not out["counts"][~filled].any()
    c1, m1 = capi.fmatrix_score(md, n, out["F"], THR, mask=True)
    assert c1[0] == out["count"] and np.array_equal(m1, out["mask"])
    if name in ("six_valid", "one_point_pair"):
        assert out["count"] == 0 and not out["F"].any() and not out["mask"].any() and not filled.any()


# ---------------------------------------------------------------------------------------------- h. score tile edges
@pytest.fixture(scope="module")
def tile_case():
    matches, cams, truth = R.synthetic(4097, seed=41)
    matches["invalid"][2::5] = 1
    F = R.F_of_pose(truth["Rp"], truth["C"], R.K_of(cams[0:1]), R.K_of(cams[1:2]))
    F = F / np.linalg.norm(F)
    rng = np.random.default_rng(42)
    eps = 10.0 ** rng.uniform(-9, -4, (3000, 1))  # from near-exact (every inlier) to far off (a few chance inliers)
    eps[0] = 1e-9
    Fs = (F.reshape(1, 9) + eps * rng.standard_normal((3000, 9))).astype(np.float32)
    Fs[5::97] = 0  # all-zero rows inside every candidate range of more than 5
    return matches, Fs


@pytest.mark.parametrize("n", [1, 7, 1023, 1024, 1025, 4097])
def test_score_tile_edges(capi, tile_case, n):
    """inlier + scoring kernel at the edges of its 1024-match block tile, its 256-candidate LDS chunk and its
    32-candidate range: counts within the 1e-3 band of float64, zero rows score 0, invalid matches are never inliers,
    and a candidate's count does not depend on how many others share the call."""
    matches, Fs = tile_case
    m = matches[:n]
    md = capi.to_dev(m)
    q, t, valid = R.split(m)
    full = capi.fmatrix_score(md, n, Fs, THR)[0]
    for k in (1, 31, 32, 255, 256, 257, 3000):
        counts = capi.fmatrix_score(md, n, Fs[:k], THR)[0]
        assert np.array_equal(counts, full[:k]), k
    assert not full[5::97].any()
    for i in range(len(Fs)):
        d2 = R.sampson_d2(Fs[i], q, t)
        ref = int(np.sum((d2 < THR * THR) & valid))
        band = int(np.sum(valid & (np.abs(d2 - THR * THR) <= 1e-3 * THR * THR)))
        assert abs(int(full[i]) - ref) <= band, (i, full[i], ref, band)
    c, mask = capi.fmatrix_score(md, n, Fs[0], THR, mask=True)
    assert not mask[~valid].any() and int(mask.sum()) == c[0]
    if n >= 1024:
        assert c[0] > 0.3 * valid.sum()  # the near-exact F passes the scene's inliers: the mask is not trivially empty


# ---------------------------------------------------------------------------------------------- the class API fallback
def test_pose_estimator_fallback_without_f(tmp_path):
    """PoseEstimator::estimatePoseRANSAC (tests/cpp/pose_ransac_test.cpp, fallback mode) with every match invalid: no F,
    so the pose is the cameras' relative pose (stage::relativePose) placed at baselineInQueryFrame() / 1000."""
    matches, cams, _ = R.synthetic(2000, seed=17)
    matches["invalid"] = 1
    cams["cam_rot"] = [(0.05, -0.02, 0.10), (0.12, 0.20, -0.30)]
    cams["cam_pos"] = [(10.0, 20.0, 30.0), (3610.0, 920.0, 1230.0)]
    path = str(tmp_path / "pair.bin")
    with open(path, "wb") as f:
        f.write(np.uint64(len(matches)).tobytes() + cams.tobytes() + matches.tobytes())
    exe = os.path.join(H.ROOT, "ssrlcv_amd", "host", "_build", "pose_ransac_test")
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "csrc"), "release"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "host"), "_build/pose_ransac_test"])
    out = subprocess.check_output([exe, path, "fallback"]).decode()
    assert out.splitlines()[-1] == "ok", out
    line = [x for x in out.splitlines() if x.startswith("ransac ")][0].split()
    inliers, pose = int(line[1]), np.array([float(x) for x in line[2:]])
    expect = H.relative_pose(cams).astype(np.float64)  # angles of Ra^T Rb, position Ra^T (b - a) / 1000
    assert inliers == 0
    assert np.abs(pose[:3] - expect[:3]).max() <= 1e-6, (pose, expect)
    assert np.abs(pose[3:] - expect[3:]).max() <= 1e-6 * np.linalg.norm(expect[3:]), (pose, expect)
