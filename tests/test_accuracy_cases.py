"""The surface-accuracy cases test something: shown on the numpy reference alone (tests/accuracy_ref.py), without a GPU, so that
tests/test_gpu_accuracy.py's bit-for-bit comparisons are comparisons of results that matter."""
import math

import numpy as np
import pytest

import accuracy_cases as C
import accuracy_ref as A
import dsm_ref as D
import mesh_ref as M


def _finite(d):
    return np.isfinite(d)


@pytest.mark.parametrize("name", sorted(n for n in C.STATS if n != "big"))
def test_the_reference_s_quantiles_are_a_plain_sort_s_and_its_sums_agree_with_fsum(name):
    c, rec = C.STATS[name], C.stats_reference(name)
    y, valid, part = A.transformed(c.values, c.center, c.absolute)
    ys = np.sort(y[part])                                        # by value: -0 and +0 compare equal
    m = len(ys)
    assert (int(rec["n"]), int(rec["valid"]), int(rec["finite"])) == (len(c.values), int(valid.sum()), m)
    for k in range(8):
        if k < len(c.quantiles) and m:
            assert rec["quantile"][k] == ys[c.quantiles[k] * (m - 1) // 10000], (name, k)
            assert (D.bits(rec["quantile"][k]) == D.bits(y[part])).any()           # one of the inputs, bits and all
        else:
            assert D.bits(rec["quantile"][k]) == D.INVALID_BITS
    if m:
        assert rec["min"] == ys[0] and rec["max"] == ys[-1]
    else:
        assert D.bits(rec["min"]) == D.INVALID_BITS and D.bits(rec["max"]) == D.INVALID_BITS
    d = [float(v) for v in ys]
    bound = m * 2.0 ** -53 * math.fsum(abs(v) for v in d)        # recursive summation of m terms, any order
    assert abs(float(rec["sum"]) - math.fsum(d)) <= bound
    sq = [v * v for v in d]                                      # exact in float64: 24-bit significands
    assert abs(float(rec["sumSq"]) - math.fsum(sq)) <= m * 2.0 ** -53 * math.fsum(sq)


def test_the_statistics_cases_hold_what_they_claim():
    sizes = {len(C.STATS[n].values) for n in C.STATS}
    assert {0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1} <= sizes
    assert C.BIG_N == 4096 * 4096 + 5 and (C.BIG_N + 4095) // 4096 == 4097        # 4097 tile sums: two second-level tiles, then one
    rec = C.stats_reference("signed_zeros")
    assert D.bits(rec["quantile"][:4]).tolist() == [0x80000000, 0x80000000, 0, 0] and D.bits(rec["min"]) == 0x80000000 and D.bits(rec["max"]) == 0
    assert C.stats_reference("ties")["quantile"][:6].tolist() == [1.0, 2.0, 2.0, 3.0, 4.0, 2.0]   # ranks 99 | 100 and 399 | 400 | 401
    assert int(C.stats_reference("only_inf")["finite"]) == 0 and int(C.stats_reference("only_inf")["valid"]) == 600
    assert int(C.stats_reference("all_invalid")["valid"]) == 0
    over = C.stats_reference("center_overflows")
    assert int(over["valid"]) == 9 and int(over["finite"]) == 5                    # inf - finite and the overflow to inf leave the selection
    neg, pos = C.stats_reference("negative"), C.stats_reference("negative/absolute")
    assert neg["max"] < 0 and pos["min"] == -neg["max"] and pos["max"] == -neg["min"] and pos["sum"] == -neg["sum"]
    mm = C.stats_reference("min_max")
    assert mm["quantile"][0] == mm["min"] and mm["quantile"][1] == mm["max"]
    twice = C.stats_reference("same_quantile_twice")["quantile"]
    assert twice[0] == twice[2] and twice[1] == twice[3] and twice[0] != twice[1]
    bits = C.stats_reference("random_bits")
    assert 0 < int(bits["finite"]) < int(bits["valid"]) == 20000                   # NaN and inf patterns among them
    assert len(set(C.stats_reference("n4097/eight")["quantile"].tolist())) >= 6


@pytest.mark.parametrize("diagonal", sorted(C.PLANES))
def test_points_on_a_dyadic_plane_have_no_difference_under_either_diagonal(diagonal):
    height, fr, pts = C.plane(*C.PLANES[diagonal])
    cells = M.mesh(height, 1, np.inf)[1]
    assert (cells == (7 if diagonal == "b-c" else 3)).all()
    d = A.difference(pts, height, fr, cells)
    fin = _finite(d)
    assert fin.sum() > 300 and (d[fin] == 0).all()
    above = pts.copy()
    above[:, 2] += np.float32(0.5)
    assert (A.difference(above, height, fr, cells)[fin] == np.float32(0.5)).all()


@pytest.mark.parametrize("name", sorted(C.DIFFERENCE))
def test_every_mesh_mode_case_leaves_half_its_points_with_a_difference(name):
    c = C.DIFFERENCE[name]
    mesh, cell = C.difference_reference(name, True), C.difference_reference(name, False)
    assert len(mesh) == len(cell) == len(c.points)
    if c.exempt:
        assert len(c.points) == 0 or min(c.frame.w, c.frame.h) < 2
        assert not _finite(mesh).any()                                             # a grid with a side below 2 has no inside
    else:
        assert 2 * _finite(mesh).sum() >= len(mesh) > 0, (name, int(_finite(mesh).sum()), len(mesh))
    if len(c.points):
        assert _finite(cell).any()


def test_the_difference_cases_hold_what_they_claim():
    sizes = {(C.DIFFERENCE[n].frame.w, C.DIFFERENCE[n].frame.h) for n in C.DIFFERENCE}
    assert {(1, 1), (1, 5), (2, 2), (7, 5)} <= sizes
    assert {len(C.DIFFERENCE["n%d" % n].points) for n in (0, 1, 63, 64, 65, 1000)} == {0, 1, 63, 64, 65, 1000}
    c = C.DIFFERENCE["relief_7x5"]
    loc = D.locate(c.points, c.frame)
    uu, vv = loc["u"] - np.float32(0.5), loc["v"] - np.float32(0.5)
    with np.errstate(all="ignore"):
        s, t = uu - np.floor(uu), vv - np.floor(vv)
    mesh, cell = C.difference_reference("relief_7x5", True), C.difference_reference("relief_7x5", False)
    fin = _finite(mesh)
    for what, on in (("s == 0", s == 0), ("t == 0", t == 0), ("s == t", s == t), ("s + t == 1", s + t == 1)):
        assert (on & fin).sum() > 10, what                                         # exactly on the seams of the triangulation
    border = _finite(cell) & ((loc["u"] < 0.5) | (loc["v"] < 0.5) | (loc["u"] >= 6.5) | (loc["v"] >= 4.5))
    assert border.sum() > 50 and not fin[border].any()                             # inside in CELL mode, outside in MESH mode
    assert (loc["u"] == 7).any() and not _finite(cell)[loc["u"] == 7].any() and not _finite(cell)[loc["v"] == 5].any()
    cut, uncut = C.cells_of("relief_7x5"), C.cells_of("relief_7x5_uncut")
    assert {1, 2, 3, 5, 6, 7} <= set(cut.ravel().tolist())                         # both diagonals, cells with one triangle
    valid = D.bits(c.height) != D.INVALID_BITS
    three = (valid[:-1, :-1].astype(int) + valid[:-1, 1:] + valid[1:, :-1] + valid[1:, 1:]) == 3
    assert three.sum() == 4 and (np.isin(cut[three], (1, 2, 5, 6))).all()          # cells with three valid corners: one triangle
    assert ((cut & 3) != (uncut & 3)).sum() >= 2                                   # max_jump cuts triangles of the spike
    sp = C.DIFFERENCE["special_heights"]
    sloc = D.locate(sp.points, sp.frame)
    in_first = (sloc["u"] >= 0.5) & (sloc["u"] < 1.5) & (sloc["v"] >= 0.5) & (sloc["v"] < 1.5)    # the mesh cell whose corner a is +inf
    assert in_first.sum() > 10 and not _finite(C.difference_reference("special_heights", True))[in_first].all()
    assert not _finite(C.difference_reference("special_heights", False))[(np.floor(sloc["u"]) == 0) & (np.floor(sloc["v"]) == 0)].any()
    n_special = len(C.SPECIAL_POINTS)
    lat = len(C.lattice(7, 5, 0.5))
    got = mesh[lat:lat + n_special]
    assert (D.bits(got[:11]) == D.INVALID_BITS).all() and got[11] > 1e38           # NaN, inf, (0, 0, 0) and far points; a huge finite z has a difference
    zeros = C.difference_reference("signed_zeros", False)
    zb = set(D.bits(zeros[zeros == 0]).tolist())
    assert zb == {0, 0x80000000}                                                   # +0 and -0 among the differences
    skew = C.DIFFERENCE["skew_frame"].frame
    assert abs(float(np.dot(skew.ex, skew.ey))) > 0.1                              # not orthonormal


def test_the_scene_cases_reach_half_coverage_and_a_shift_moves_the_bias_alone():
    """the end-to-end cases on the reference alone: the ground-truth cloud of a view against the ground-truth height map, and the
    quantised scene raised by a power of two"""
    fr = C.DC.scene_frame()
    truth = C.truth_map()
    cells = M.mesh(truth, 1, np.inf)[1]
    rep = A.report(A.difference(C.truth_cloud(), truth, fr, cells))
    assert rep["coverage"] >= 0.5 and abs(rep["bias"]) < 0.05 and rep["nmad"] < 0.05 and rep["le95"] < 0.2   # km, on +-2 km of relief
    pts, height, qfr = C.quantised_scene()
    qcells = M.mesh(height, 1, np.inf)[1]
    base = A.report(A.difference(pts, height, qfr, qcells))
    assert base["coverage"] >= 0.5
    for delta in (0.5, 4.0):
        up = A.report(A.difference(C.quantised_scene(delta)[0], height, qfr, qcells))
        assert up["bias"] == base["bias"] + delta and up["nmad"] == base["nmad"] and up["coverage"] == base["coverage"]
        assert up["mean"] != base["mean"]
