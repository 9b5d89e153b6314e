"""tests/cloud_cases.py proved on the numpy reference alone (no GPU): the scale sweep does to the float32 key what the
contract says it does, the few-finite clouds have the stated tails, the all-far cell leaves no query on the grid, no filter
case has an m within reach of the last bit of its threshold, the constructed keep patterns are the reference's, and the
normals cases held to the angle bound have an eigengap.  tests/test_gpu_cloud_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import cloud_cases as C
import cloud_ref as R

KNN = C.knn_cases()
FILTER = C.filter_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def sweep():
    """e -> (nbr, d2) of the scale sweep by brute force"""
    return {e: R.knn_brute(KNN["scale_sweep_e%+d" % e].p, 16) for e in C.SCALE_EXPONENTS}


def test_scale_sweep_is_the_table_of_the_issue(sweep):
    n0, d0 = sweep[0]
    n = len(n0)
    lowest = np.array([[j for j in range(18) if j != i][:16] for i in range(n)], np.uint32)
    sub = lambda d: float(((d > 0) & (d < np.float32(2.0 ** -126))).mean())
    differ = {e: int((sweep[e][0] != n0).any(1).sum()) for e in C.SCALE_EXPONENTS}
    print("scale sweep: rows differing from e = 0: %s; subnormal share at -60 / -64 / -70: %.2f / %.2f / %.2f; zero share "
          "at -70: %.3f" % (differ, sub(sweep[-60][1]), sub(sweep[-64][1]), sub(sweep[-70][1]), (sweep[-70][1] == 0).mean()))
    for e in (-40, 40, 62):   # a power of two scales every step exactly while nothing leaves the normal range
        assert np.array_equal(sweep[e][0], n0)
        assert np.array_equal(_bits(sweep[e][1]), _bits(d0 * np.float32(4.0) ** np.float32(e)))
    assert np.array_equal(sweep[-60][0], n0) and sub(sweep[-60][1]) >= 0.5
    assert differ[-64] >= 1 and differ[-70] > n // 2
    assert (sweep[-80][1] == 0).all() and np.array_equal(sweep[-80][0], lowest)


def test_scale_overflow_keeps_valid_indices():
    case = KNN["scale_sweep_overflow"]
    nbr, d2 = R.knn_brute(case.p, case.k)
    inf = np.isinf(d2)
    assert inf.any() and (nbr[inf] != R.NONE).all() and (nbr < len(case.p)).all()
    assert (np.diff(nbr.astype(np.int64), axis=1)[inf[:, :-1] & inf[:, 1:]] > 0).all()   # ties at +inf: index order


def test_few_finite_tails():
    nbr, d2 = R.knn_brute(KNN["few_finite_13_others"].p, 16)
    fin = R.finite_mask(KNN["few_finite_13_others"].p)
    assert fin.sum() == 14
    assert ((nbr[fin] != R.NONE).sum(1) == 13).all() and (nbr[fin][:, 13:] == R.NONE).all() and np.isinf(d2[fin][:, 13:]).all()
    assert (nbr[~fin] == R.NONE).all() and np.isinf(d2[~fin]).all()
    nbr, d2 = R.knn_brute(KNN["few_finite_none"].p, 16)
    assert (nbr == R.NONE).all() and np.isinf(d2).all()
    assert R.finite_mask(KNN["few_finite_one"].p).sum() == 1
    nbr, d2 = R.knn_brute(KNN["few_finite_one"].p, 16)
    assert (nbr == R.NONE).all() and np.isinf(d2).all()


def test_small_cases_are_what_they_claim():
    for name, case in KNN.items():
        assert len(case.p) >= case.k + 1 and len(case.p) <= 3000, name
        if name.startswith("n_is_k_plus_1") or name == "n2_k1":
            assert len(case.p) == case.k + 1
    nbr, d2 = R.knn_brute(KNN["coincident"].p, 16)
    assert (d2 == 0).all() and np.array_equal(nbr[0], np.arange(1, 17)) and np.array_equal(nbr[299], np.arange(16))
    ext = lambda p: np.sort(p.max(0) - p.min(0))
    assert ext(KNN["plane"].p)[0] == 0 and ext(KNN["plane"].p)[1] > 0          # sheet branch
    assert ext(KNN["line"].p)[1] == 0 and ext(KNN["line"].p)[2] > 0            # line branch
    assert ext(KNN["coincident"].p)[2] == 0                                     # point branch
    assert KNN["outlier_range_raised"].cells[0] < ext(KNN["outlier_range_raised"].p)[2] / 2 ** 20
    e = KNN["ecef_quantised"].p
    assert len(np.unique(e, axis=0)) < len(e)                                   # float32 spacing made duplicates
    _, d2 = R.knn_brute(e, 16)
    assert (np.diff(d2, axis=1) == 0).mean() > 0.1                              # and ties


@pytest.mark.parametrize("name", [n for n, c in KNN.items() if c.all_far])
def test_all_far_cell_leaves_no_query_on_the_grid(name):
    """the grid search looks at most 3 rings out and stops only below (distance to the block's faces)^2 <= (4 h)^2: with
    every k-th d2 above that, and h not raised, every finite query goes to the far scan"""
    case = KNN[name]
    h = case.cells[0]
    assert len(case.cells) == 1 and h >= 1.0 / 2 ** 20
    _, d2 = R.knn_brute(case.p, case.k)
    assert (d2[:, case.k - 1] > (4 * h) ** 2).all()


def test_reference_tree_path_redoes_underflowing_rows():
    assert R.self_test()
    for e in (-70, -64, -60):
        p = KNN["scale_sweep_e%+d" % e].p
        a, b = R.knn(p, 16), R.knn_brute(p, 16)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])), e


# ---------------------------------------------------------------- filter
def _filter_margin(case):
    m = R.mean_distance(case.d2, case.k)
    mu, std, t = R.filter_stats(m, float(np.float32(case.sigma)))
    f = m[np.isfinite(m)].astype(np.float64)
    return m, mu, std, t, (np.abs(f - t).min() / abs(t) if len(f) and t != 0 else np.inf)


@pytest.mark.parametrize("name", list(FILTER) + ["big"])
def test_filter_case_margin_and_pattern(name):
    """no finite m within 1e-9 t of the reference's t, so the reference mask does not hang on the last bit of t (the GPU's
    statistics are held to 1e-12); the all-equal cases instead have std = 0 and m = t exactly"""
    case = C.filter_big() if name == "big" else FILTER[name]
    assert case.d2.shape[0] >= case.k + 1
    m, mu, std, t, margin = _filter_margin(case)
    keep = R.filter_mask(m, t)
    if case.exact:
        assert std == 0.0 and (m.astype(np.float64) == t).all() and keep.all()
    else:
        assert margin > 1e-9, (name, margin)
    if case.keep is not None:
        assert np.array_equal(keep, case.keep), name
    if name == "all_nonfinite":
        assert (mu, std, t) == (0.0, 0.0, 0.0) and not np.isfinite(m).any()
    if name.startswith("extremes"):
        assert (case.d2 == 0).any() and ((case.d2 > 0) & (case.d2 < np.float32(2.0 ** -126))).any() and (case.d2 > 2e38).any()
        assert np.isfinite(m).all()
    if name == "tile_rejected":
        assert keep[:2048].all() and not keep[2048:4096].any() and keep[4096:].all()
    if name == "big":
        assert len(m) == 2048 * 2048 + 2049 and 0.3 < keep.mean() < 0.7


def test_filter_margin_on_real_clouds():
    """cube and terrain at k = 2, 16, 32 (sigma = 2): the smallest |m - t| / t"""
    worst = np.inf
    for p in (C.cube(3000, 3), R.terrain_cloud(3000, seed=6)[0]):
        for k in (2, 16, 32):
            _, d2 = R.knn_brute(p, k)
            worst = min(worst, _filter_margin(C.FilterCase(d2, k, 2.0, None, False))[4])
    print("smallest |m - t| / t over cube and terrain at k = 2, 16, 32: %.2g" % worst)
    assert worst > 1e-9


# ---------------------------------------------------------------- normals
@pytest.fixture(scope="module")
def normal_cases():
    return C.normal_cases()


def test_normals_cases_have_an_eigengap(normal_cases):
    assert tuple(normal_cases) == C.NORMAL_NAMES
    held = total = 0
    smallest = np.inf
    for name, case in normal_cases.items():
        if not name.startswith(("cube", "terrain")) or case.k < 2:
            continue
        ref, gap = R.normals(case.p, case.nbr, case.k, case.vp)
        nz = np.abs(ref).sum(1) > 0
        held += int((gap[nz] > 1e-6).sum())
        total += int(nz.sum())
        smallest = min(smallest, gap[nz].min())
    print("rows with a relative eigengap above 1e-6: %d of %d (%.2f %%), smallest gap %.2g" % (held, total, 100.0 * held / total, smallest))
    assert held >= 0.99 * total


def test_normals_zero_rows_and_hand_tables(normal_cases):
    for name in ("coincident_table", "zero_rows"):
        case = normal_cases[name]
        ref, _ = R.normals(case.p, case.nbr, case.k, case.vp)
        assert np.array_equal(np.nonzero(np.abs(ref).sum(1) == 0)[0], case.zero_rows), name
    assert len(normal_cases["zero_rows"].zero_rows) == 6
    for name in ("collinear_table", "k1_table"):
        case = normal_cases[name]
        ref, gap = R.normals(case.p, case.nbr, case.k, case.vp)
        assert np.allclose(np.linalg.norm(ref, axis=1), 1.0, atol=1e-12) and np.abs(ref @ case.line).max() < 1e-12
    for name in ("plane_vp_above", "plane_vp_below"):
        case = normal_cases[name]
        ref, _ = R.normals(case.p, case.nbr, case.k, case.vp)
        assert np.array_equal(ref, np.tile([0.0, 0.0, 1.0 if "above" in name else -1.0], (len(ref), 1)))


def test_normals_reference_is_scale_invariant(normal_cases):
    """2^+-60 and the ECEF offset are exact images of the base cloud: the eigh reference agrees with itself to the
    solvers' share of the angle bound"""
    base = normal_cases["invariance_base"]
    ref, gap = R.normals(base.p, base.nbr, base.k, base.vp)
    good = gap > 1e-6
    assert good.mean() > 0.99
    for name in C.INVARIANT:
        case = normal_cases[name]
        got, g2 = R.normals(case.p, case.nbr, case.k, case.vp)
        ang = np.arctan2(np.linalg.norm(np.cross(got[good], ref[good]), axis=1), (got[good] * ref[good]).sum(1))
        assert (ang <= 2 * 64.0 * (case.k + 1) * 2.0 ** -53 / gap[good]).all(), (name, ang.max())
        assert np.allclose(g2[good], gap[good], rtol=1e-6)
