"""Pose LM terms, no GPU: the cases of tests/pose_cases.py test something.  Everything here is the CPU oracle
(oracle/oracle_pose.c) on the cases tests/test_gpu_pose_edges.py runs on the device: the per-match export is the body of
oracle_pose_lm_terms, the reference is finite and its bound holds for the oracle's own order and for the kernel's order
restated in numpy, and the ways the kernel could be wrong without the fixture test noticing (the other camera's
intrinsics, x for y, a Jacobian column 0.1 % off, a match, a wave or a stride pass lost) all land outside the bound."""
import numpy as np
import pytest

import helpers as H
import pose_cases as C


def _rebuild_one(lib, m, pose, cams):
    """(JTJ[6, 6], JTf[6], cost) of one match from oracle_pose_residual alone, in numpy float32: seven residuals, the
    central differences, and the sums in oracle_pose_lm_terms' order (rows 0..3; the 4th row and the position columns 0)"""
    def res(p):
        out = np.zeros(4, np.float32)
        q, t = np.ascontiguousarray(m["kp0_loc"], np.float32), np.ascontiguousarray(m["kp1_loc"], np.float32)
        lib.oracle_pose_residual(H.P(p), H.P(cams[0:1]), H.P(cams[1:2]), H.P(q), H.P(t), H.P(out))
        return out
    pose = np.asarray(pose, np.float32).copy()
    delta = np.float32(1e-5)
    f = res(pose)
    J = np.zeros((4, 6), np.float32)
    for c in range(3):
        p = pose.copy()
        p[c] = p[c] + delta
        right = res(p)
        p[c] = p[c] - np.float32(2) * delta
        left = res(p)
        J[:, c] = (right - left) / (np.float32(2) * delta)
    jtj, jtf = np.zeros((6, 6), np.float32), np.zeros(6, np.float32)
    for r in range(4):
        for i in range(6):
            for j in range(6):
                jtj[j, i] = jtj[j, i] + J[r, i] * J[r, j]
            jtf[i] = jtf[i] + J[r, i] * f[r]
    sq = f * f
    return jtj, jtf, np.float32(0) + (((sq[0] + sq[1]) + sq[2]) + sq[3]), f, J


def test_match_terms_is_the_body_of_lm_terms_on_the_fixture(oracle_lib):
    """300 fixture matches one at a time: the numpy rebuild from oracle_pose_residual, the export and
    oracle_pose_lm_terms(n = 1) agree bit for bit"""
    v = H.load_view("Pipeline2View")
    cams = v["cameras"]
    m = H.matches_from_matchset(v["kp0"])[:300]
    pose = H.relative_pose(cams)
    f, J = H.oracle_pose_match_terms(oracle_lib, m, pose, cams[0:1], cams[1:2])
    one = C.one_match_sums(C.products(f, J))
    for i in range(len(m)):
        jtj, jtf, cost = H.oracle_pose_terms(oracle_lib, m[i:i + 1], pose, cams[0:1], cams[1:2])
        rj, rf, rc, f1, J1 = _rebuild_one(oracle_lib, m[i], pose, cams)
        assert np.array_equal(H.bits(jtj), H.bits(rj)) and np.array_equal(H.bits(jtf), H.bits(rf)), i
        assert np.float32(cost).view(np.uint32) == rc.view(np.uint32), i
        assert np.array_equal(H.bits(f[i]), H.bits(f1[:3])) and np.array_equal(H.bits(J[i]), H.bits(J1[:3, :3])), i
        assert np.array_equal(H.bits(C.got10(jtj, jtf, cost)), H.bits(one[i])), i


def test_chain_depth_follows_the_launch_shape():
    assert [C.pose_blocks(n) for n in (1, 256, 257, 262144, 262145, C.STRIDE_N)] == [1, 1, 2, 1024, 1024, 1024]
    assert C.chain_depth(1, 3) == 3 + 6 + 4 and C.chain_depth(257, 1) == 1 + 6 + 8
    assert C.chain_depth(262144, 3) == 3 + 6 + 4096 and C.chain_depth(C.STRIDE_N, 3) == 6 + 6 + 4096
    assert abs(C.gamma(C.chain_depth(C.STRIDE_N, 3)) - 2.45e-4) < 1e-6
    assert C.STRIDE_N - 262144 == 256 * 256 + 63                               # 256 whole blocks and a partial wave


def _mutant_ratio(ref, mutant):
    """how far a wrong kernel's exact sums lie from the reference, in units of the reference's bound, per JTJ / JTf entry"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(mutant["S"] - ref["S"]) / ref["bound"])[:9]


@pytest.mark.parametrize("name", C.FINITE_CASES)
def test_finite_case_reference_and_mutants(oracle_lib, name):
    c = C.case(name)
    m, pose, cams = c["matches"], c["pose"], c["cams"]
    n = len(m)
    ref = C.reference(oracle_lib, name)
    f, J, prod = ref["f"], ref["J"], ref["prod"]
    # ---- the reference checks itself
    assert np.isfinite(f).all() and np.isfinite(J).all() and np.isfinite(prod).all()
    assert (ref["absum"][:9] > 0).all() and ref["absum"][9] > 0
    one = C.one_match_sums(prod)
    for i in sorted({0, n // 2, n - 1}):
        jtj, jtf, cost, _, _ = _rebuild_one(oracle_lib, m[i], pose, cams)
        oj, of, oc = H.oracle_pose_terms(oracle_lib, m[i:i + 1], pose, cams[0:1], cams[1:2])
        assert np.array_equal(H.bits(jtj), H.bits(oj)) and np.array_equal(H.bits(jtf), H.bits(of)), i
        assert np.array_equal(H.bits(C.got10(oj, of, oc)), H.bits(one[i])) and cost == np.float32(oc), i
    oj, of, oc = H.oracle_pose_terms(oracle_lib, m, pose, cams[0:1], cams[1:2])
    assert np.array_equal(oj, oj.T) and not oj[3:].any() and not of[3:].any()
    own = C.gamma(3 * n) * ref["absum"]                                         # the oracle adds match by match: 3 n additions
    miss = np.abs(C.got10(oj, of, oc).astype(np.float64) - ref["S"])
    assert (miss <= own).all(), (miss / own)
    assert abs(H.oracle_pose_cost(oracle_lib, m, pose, cams[0:1], cams[1:2]) - ref["S"][9]) <= own[9]
    sim = max(float(C.ratios(C.simulate(prod, seed), ref).max()) for seed in range(3))
    print("%s: n %d, bound / |exact| %.2g .. %.2g, the kernel's order in numpy is at %.3f of the bound"
          % (name, n, (ref["bound"] / np.abs(ref["S"])).min(), (ref["bound"] / np.abs(ref["S"])).max(), sim))
    assert sim <= 1
    if name == "big_angles":
        assert (ref["S"][:6] < 0).any() and (ref["absum"][:6] > 1.01 * np.abs(ref["S"][:6])).any()
    if name == "sym_true":
        assert (np.abs(ref["S"][6:9]) < 0.2 * ref["absum"][6:9]).all()           # JTf is small against its own terms
    if name == "outside":
        loc = np.concatenate([m["kp0_loc"], m["kp1_loc"]])
        assert (loc < 0).any() and (np.abs(loc) == 1e6).any() and (loc > 1280).any()

    # ---- mutants of the reference: each must fall outside the bound
    swapped, dpix, size = cams[::-1].copy(), cams.copy(), cams.copy()
    dpix["dpix"] = cams["dpix"][:, ::-1]
    size["size"] = cams["size"][:, ::-1]
    for what, mc in (("cameras swapped", swapped), ("dpix x/y swapped", dpix), ("size x/y swapped", size)):
        mut = C.reference(oracle_lib, name, cams=mc)
        if C.is_asymmetric(name):
            r = _mutant_ratio(ref, mut)
            print("  %s: at least %.3g bounds away" % (what, r.min()))
            assert (r > 1).all(), (what, r)
        else:
            # no-ops by construction: the reason the asymmetric cases exist
            assert np.array_equal(H.bits(mut["f"]), H.bits(f)) and np.array_equal(H.bits(mut["J"]), H.bits(J)), what
    Jp = J.copy()
    Jp[:, :, 1] = J[:, :, 1] * np.float32(1.001)
    r = _mutant_ratio(ref, C.reference_of(f, Jp))
    print("  pitch column x 1.001: at least %.3g bounds away" % r[list(C.PITCH_ENTRIES)].min())
    assert (r[list(C.PITCH_ENTRIES)] > 1).all(), r
    if n <= 2000:
        for what, keep in (("last match dropped", n - 1), ("last partial wave dropped", (n - 1) // 64 * 64)):
            r = _mutant_ratio(ref, C.reference_of(f[:keep], J[:keep]))
            print("  %s: at least %.3g bounds away" % (what, r.min()))
            assert (r > 1).all(), (what, r)
    if name == "stride":
        T = 256 * C.pose_blocks(n)
        assert T < n < 2 * T
        r = _mutant_ratio(ref, C.reference_of(f[:T], J[:T]))
        print("  second stride pass dropped: at least %.3g bounds away, %.3g of the sum lost"
              % (r.min(), 1 - T / n))
        assert (r > 1).all(), r


@pytest.mark.parametrize("name", C.NONFINITE_CASES)
def test_nonfinite_case_is_what_it_claims(oracle_lib, name):
    c = C.case(name)
    at = 0 if name.endswith("alone") else C.NONFINITE_AT
    assert len(c["matches"]) == (1 if name.endswith("alone") else C.NONFINITE_N)
    assert not c["pose"][:3].any()
    ref = C.reference(oracle_lib, name)
    # the parallel match: its residual is 0 / 0, and so is the yaw column (turning (0, 0, 1) about z leaves it parallel);
    # roll and pitch move the target ray off the query's, those columns are finite
    assert np.isnan(ref["f"][at]).all() and np.isnan(ref["J"][at][:, 2]).all()
    assert np.isfinite(ref["J"][at][:, :2]).all()
    rest = np.delete(np.arange(ref["n"]), at)
    assert np.isfinite(ref["f"][rest]).all() and np.isfinite(ref["J"][rest]).all()
    nan = np.isnan(ref["S"])
    assert list(nan) == [False, False, True, False, True, True, True, True, True, True], nan
    assert np.isfinite(ref["S"][~nan]).all()
    # the oracle itself: NaN where S is, and NaN * 0 = NaN in the position entries the yaw column and the residual reach
    # (upstream's arithmetic; the kernel never forms those products and returns +0 there)
    oj, of, oc = H.oracle_pose_terms(oracle_lib, c["matches"], c["pose"], c["cams"][0:1], c["cams"][1:2])
    got = C.got10(oj, of, oc)
    assert all(C.agrees(g, S, C.gamma(3 * ref["n"]) * a) for g, S, a in zip(got, ref["S"], ref["absum"]))
    assert np.isnan(oj[3:, 2]).all() and np.isnan(oj[2, 3:]).all() and np.isnan(of[3:]).all()
    assert np.isnan(H.oracle_pose_cost(oracle_lib, c["matches"], c["pose"], c["cams"][0:1], c["cams"][1:2]))


def test_single_includes_the_fixture_ends(oracle_lib):
    """the first and the last fixture match at the fixture pose are finite and have a reference"""
    v = H.load_view("Pipeline2View")
    m = H.matches_from_matchset(v["kp0"])
    f, J = H.oracle_pose_match_terms(oracle_lib, m[[0, -1]], H.relative_pose(v["cameras"]), v["cameras"][0:1],
                                     v["cameras"][1:2])
    assert np.isfinite(f).all() and np.isfinite(J).all() and J.any(axis=(1, 2)).all()
