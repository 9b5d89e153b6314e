"""Point-cloud leg, no GPU: the cases of tests/pointcloud_cases.py test something.  Everything here is the CPU oracle
(oracle/oracle_pointcloud.c) on the cases tests/test_gpu_pointcloud_edges.py runs on the device: the synthetic cases are
finite, every degenerate row lands in the class its table claims, the numpy restatement of wave_sum and the bound on the
order of the atomics are what they say, and the parameter sets of every ba_sweep2 case can be told apart."""
import numpy as np
import pytest

import helpers as H
import pointcloud_cases as C


def test_rig_and_matchset_are_what_the_issue_asks():
    rng = np.random.default_rng(0)
    cams = C.rig(7, rng)
    assert (np.abs(cams["cam_pos"]) <= 50).all() and (np.abs(cams["cam_rot"]) <= np.pi).all()
    assert ((cams["fov"][:, 0] >= 0.05) & (cams["fov"][:, 0] <= 1.2)).all()
    assert ((cams["foc"] >= 0.01) & (cams["foc"] <= 0.5)).all()
    assert (cams["size"] >= 200).all() and (cams["size"] <= 5000).all() and (cams["size"][:, 0] != cams["size"][:, 1]).all()
    mm, kp = C.matchset(1000, 7, 2, 9, rng)
    assert set(np.unique(mm["numKeyPoints"])) == set(range(2, 10)) and set(np.unique(kp["parentId"])) == set(range(7))
    assert (np.diff(mm["index"]) < 0).any()                                    # not in bundle order
    # the runs tile the key-point array exactly
    covered = np.zeros(len(kp), int)
    for m in mm:
        covered[m["index"]: m["index"] + m["numKeyPoints"]] += 1
    assert (covered == 1).all()
    assert (kp["loc"] < 0).any() and (kp["loc"] > 5000).any() and kp["loc"].min() >= -100 and kp["loc"].max() <= 5100


def test_wave_partials_is_the_butterfly():
    for n in (1, 63, 64, 65, 300):
        for e in (-3, 0, 5):
            p = C.wave_partials(np.full(n, 2.0 ** e, np.float32))
            counts = np.minimum(64, n - 64 * np.arange((n + 63) // 64))
            assert p.dtype == np.float32 and np.array_equal(p, counts * np.float32(2.0 ** e)), (n, e)
    # the order matters and is the butterfly's: lane 0 adds (((((l0 + l32) + (l16 + l48)) + ...
    v = np.zeros(64, np.float32)
    v[0], v[32], v[16] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert C.wave_partials(v)[0] == np.float32(1.0)                            # 1 + 2^-24 rounds to 1 before l16 arrives
    v[:] = 0
    v[0], v[16], v[48] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert C.wave_partials(v)[0] == np.float32(1.0 + 2.0 ** -23)               # l16 + l48 = 2^-23 arrives whole
    assert C.wave_partials(np.zeros((3, 0), np.float32)).shape == (3, 0)
    assert C.sum_bound(np.ones(1, np.float32)) == 0.0 and C.sum_bound(np.ones(5, np.float32)) == 4 * 5 * 2.0 ** -24


def test_same_is_bits_or_both_nan():
    a = np.array([0.0, -0.0, np.inf, np.nan, 1.0, np.nan], np.float32)
    b = np.array([0.0, 0.0, np.inf, -np.nan, 1.0, 1.0], np.float32)
    assert list(C.same(a, b)) == [True, False, True, True, True, False]
    assert not C.same(np.float32(np.inf), np.float32(-np.inf))


@pytest.mark.parametrize("n", C.GEN_SIZES)
def test_generate_bundles_cases_are_finite(oracle_lib, n):
    cams, mm, kp = C.bundle_input(n)
    b, l, _ = H.oracle_bundles(oracle_lib, mm, kp, cams)
    assert np.isfinite(l["vec"]).all() and np.isfinite(l["pnt"]).all()
    assert np.abs(np.linalg.norm(l["vec"].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(b["index"], mm["index"]) and np.array_equal(b["numLines"], mm["numKeyPoints"])
    if n > 1:
        assert (np.diff(mm["index"]) < 0).any()
    # size.y matters (the principal point) and so does the camera a key point names
    sq = cams.copy()
    sq["size"][:, 1] = sq["size"][:, 0]
    assert not np.array_equal(H.oracle_bundles(oracle_lib, mm, kp, sq)[1]["vec"], l["vec"])


def _sum_figures(ref):
    """the oracle's own sequential float sum lies within sum_bound of the exact sum of the wave partials?"""
    p = C.wave_partials(ref["errors"])
    return abs(float(ref["sum"]) - float(C.sum_reference(p))), float(C.sum_bound(p)), p


@pytest.mark.parametrize("nview", [False, True])
@pytest.mark.parametrize("n", C.TRI_SIZES + (C.EMBED_N,))
def test_triangulation_cases_are_finite_and_their_sums_bounded(oracle_lib, n, nview):
    b, l = (C.n_view_input if nview else C.two_view_input)(oracle_lib, n)
    assert np.isfinite(l["vec"]).all() and np.isfinite(l["pnt"]).all()
    if nview:
        norms = np.linalg.norm(l["vec"].astype(np.float64), axis=1)
        assert norms.min() >= 0.499 and norms.max() <= 3.001 and (np.abs(norms - 1) > 0.01).mean() > 0.9
        if n >= 63:
            assert b["numLines"].min() == 2 and b["numLines"].max() == 9
    ref = C.triangulate_ref(oracle_lib, nview, b, l)
    assert np.isfinite(ref["points"]).all() and np.isfinite(ref["errors"]).all() and (ref["errors"] >= 0).all()
    assert (ref["points"].view(np.uint32) != C.SENTINEL).all()                 # no singular S among the random bundles
    miss, bound, p = _sum_figures(ref)
    # the float sum of the partials in the oracle's order (wave 0 first) is one of the orders the atomics can take: inside
    seq = np.float32(0)
    for w in p:
        seq = np.float32(seq + w)
    assert abs(float(seq) - float(C.sum_reference(p))) <= bound
    # The oracle's returned sum adds the n errors one by one, n - 1 roundings where the device's has W - 1 after six
    # butterfly levels, so sum_bound (W additions) is not a bound for it: at n = 65 it is 0.0078 away with a bound of 0.0071.
    # Its own bound is (n - 1) u sum e, and the partials carry at most 6 u sum e from the butterfly.
    own = (n - 1 + 6) * 2.0 ** -24 * float(ref["errors"].astype(np.float64).sum()) * (1 + 2.0 ** -20)
    print("n %d nview %d: oracle's sequential sum %r is %.3g from the partials' sum; bound of the device's sum %.3g, of the "
          "oracle's %.3g" % (n, nview, float(ref["sum"]), miss, bound, own))
    assert miss <= own
    if n == 1:
        assert ref["sum"] == p[0]
    # the cutoff: one bundle's own error; the strict compare keeps that bundle
    if n > 1:
        cut = C.pick_cutoff(ref["errors"])
        flagged = C.triangulate_ref(oracle_lib, nview, b, l, cutoff=cut)["invalid"]
        at = np.flatnonzero(ref["errors"] == np.float32(cut))
        assert len(at) >= 1 and (flagged[at] == 0).all() and 0 < flagged.sum() < n
        assert np.array_equal(flagged != 0, ref["errors"] > np.float32(cut))


def test_n_view_error_uses_the_raw_vec(oracle_lib):
    """scaling a line's vec changes the N-view error's rounding (lp2 = pnt + 1000 vec) but not S: the points stay, errors move"""
    b, l = C.n_view_input(oracle_lib, 257)
    unit = l.copy()
    n = np.linalg.norm(l["vec"].astype(np.float64), axis=1, keepdims=True)
    unit["vec"] = (l["vec"] / n).astype(np.float32)
    a, u = C.triangulate_ref(oracle_lib, True, b, l), C.triangulate_ref(oracle_lib, True, b, unit)
    assert (a["errors"] != u["errors"]).mean() > 0.5
    assert np.allclose(a["errors"], u["errors"], rtol=1e-2, atol=1e-6)


def test_two_view_degenerate_rows_land_in_their_classes(oracle_lib):
    b, l, classes = C.degenerate_two_view()
    assert classes == ["nan", "nan", "residue", "residue", "finite", "inf"]
    ref = C.triangulate_ref(oracle_lib, False, b, l, cutoff=1.0)
    for g, c in enumerate(classes):
        pt, e, inv = ref["points"][g], ref["errors"][g], ref["invalid"][g]
        L1, L2 = l[b["index"][g]], l[b["index"][g] + 1]
        cr = np.cross(L1["vec"].astype(np.float64), L2["vec"].astype(np.float64))
        if c == "nan":
            assert np.isnan(pt).all() and np.isnan(e) and inv == 0, (g, pt, e, inv)
        elif c == "residue":
            # parallel in exact arithmetic, and yet finite: the float cross product is a rounding residue, not zero
            assert np.abs(cr).max() < 1e-7 and np.isfinite(pt).all() and np.isfinite(e), (g, pt, e)
        elif c == "finite":
            assert np.array_equal(pt, np.array([3, 0, 0], np.float32)) and e == 0 and inv == 0
        else:
            assert np.isfinite(pt).all() and np.isposinf(e) and inv == 1, (g, pt, e, inv)
    assert np.array_equal(ref["points"][2], np.zeros(3, np.float32))           # the line through the origin, twice
    # NaN and inf together: the sum is NaN; the inf row alone: inf
    assert np.isnan(ref["sum"]) and np.isnan(C.sum_reference(C.wave_partials(ref["errors"])))
    assert np.isposinf(C.sum_reference(C.wave_partials(ref["errors"][2:])))
    ok, text = C.sum_agrees(ref["sum"], ref["errors"])
    assert ok, text


def test_n_view_degenerate_rows_land_in_their_classes(oracle_lib):
    b, l, classes = C.degenerate_n_view()
    assert classes == ["finite", "singular", "finite", "either", "finite", "nan"]
    assert (b["numLines"] >= 2).all()
    ref = C.triangulate_ref(oracle_lib, True, b, l, cutoff=0.25)
    unwritten = (ref["points"].view(np.uint32) == C.SENTINEL).all(1)
    for g, c in enumerate(classes):
        pt, e = ref["points"][g], ref["errors"][g]
        if c == "singular":
            assert unwritten[g] and e == np.float32(0.5) and ref["invalid"][g] == 1, (g, pt, e)
        elif c == "finite":
            assert not unwritten[g] and np.isfinite(pt).all() and np.isfinite(e), (g, pt, e)
        elif c == "nan":
            assert not unwritten[g] and np.isfinite(pt).all() and np.isnan(e) and ref["invalid"][g] == 0, (g, pt, e)
        print("n-view row %d (%s): point %s error %r unwritten %s" % (g, c, pt, float(e), bool(unwritten[g])))
    # the singular row's determinant is exactly zero, not small: S = sum(v v^T - I) = diag(-2, -2, 0)
    assert not unwritten[0] and not unwritten[2]


@pytest.mark.parametrize("nview", [False, True])
def test_embedded_cases_put_the_rows_where_they_claim(oracle_lib, nview):
    firsts = C.embedded_firsts(nview)
    assert firsts == (0, 3)
    seen = []
    for first in firsts:
        b, l, at = C.embedded(oracle_lib, nview, first)
        assert len(b) == C.EMBED_N and sorted(at) == [63, 64, 255]
        ref = C.triangulate_ref(oracle_lib, nview, b, l)
        rest = np.setdiff1d(np.arange(C.EMBED_N), list(at))
        assert np.isfinite(ref["errors"][rest]).all() and np.isfinite(ref["points"][rest]).all()
        for g, c in at.items():
            seen.append(c)
            if c == "nan":
                assert np.isnan(ref["errors"][g])
            if c == "inf":
                assert np.isposinf(ref["errors"][g])
            if c == "singular":
                assert (ref["points"][g].view(np.uint32) == C.SENTINEL).all()
        ok, text = C.sum_agrees(ref["sum"], ref["errors"]) if not np.isfinite(ref["sum"]) else (True, "")
        assert ok, text
    assert sorted(seen) == sorted((C.degenerate_n_view if nview else C.degenerate_two_view)()[2])


@pytest.mark.parametrize("n,K", C.SWEEP_CASES)
def test_sweep_parameter_sets_can_be_told_apart(oracle_lib, n, K):
    cams, mm, kp, params = C.sweep_input(n, K)
    assert len(cams) == C.SWEEP_NCAM and params.shape == (K, 30) and (mm["numKeyPoints"] == 2).all()
    pairs = kp["parentId"][mm["index"][:, None] + np.arange(2)]
    if n >= 63:
        assert (pairs[:, 0] < pairs[:, 1]).any() and (pairs[:, 0] > pairs[:, 1]).any()   # both orders
        assert set(np.unique(pairs)) == set(range(C.SWEEP_NCAM)) and (np.diff(mm["index"]) < 0).any()
    else:
        assert pairs[0, 0] > pairs[0, 1] and pairs[0, 0] >= 2                     # cameras past the first two, the higher first
    p = C.sweep_partials(oracle_lib, n, K)
    assert p.shape == (K, (n + 63) // 64) and np.isfinite(p).all()
    ref, bound = C.sum_reference(p), C.sum_bound(p)
    assert len(np.unique(ref.astype(np.float32))) == K                            # K distinct float32 values
    if K > 1:
        order = np.argsort(ref)
        gap = np.full(K, np.inf)
        d = np.diff(ref[order])
        gap[order[:-1]] = d
        gap[order[1:]] = np.minimum(gap[order[1:]], d)
        share = float((gap > 4 * bound).mean())
        print("ba_sweep2 n %d K %d: %.1f %% of the sets have no other set's reference within 4 x their bound" % (n, K, 100 * share))
        assert share >= 0.95
    # a kernel that read camera 0 / 1 for every key point, or set 0 for every set, computes something else
    folded = kp.copy()
    folded["parentId"] %= 2
    e = C.sweep_errors(oracle_lib, cams, mm, folded, params[:1])
    assert not np.array_equal(C.wave_partials(e)[0], p[0])


def test_fixture_sweep_reference(oracle_lib):
    """the reference of test_ba_sweep_matches_oracle: finite, and it is the oracle's own ba_eval up to the order of the sum"""
    import ctypes
    mm, kp, cams, params, p = C.fixture_sweep(oracle_lib)
    assert p.shape == (612, (len(mm) + 63) // 64) and np.isfinite(p).all()
    ref = C.sum_reference(p)
    for k in (0, 611):
        whole = oracle_lib.oracle_ba_eval(ctypes.c_uint32(len(mm)), H.P(mm), H.P(kp), H.P(cams), ctypes.c_uint32(2),
                                          H.P(np.ascontiguousarray(params[k])))
        assert abs(whole - ref[k]) <= 1e-4 * ref[k], (k, whole, ref[k])           # a sequential float sum of 13 308 terms
    bound = C.sum_bound(p)
    print("fixture sweep: bounds %.3g .. %.3g relative (was 2e-3 on five sets)" % ((bound / ref).min(), (bound / ref).max()))
    assert (bound / ref).max() < 2e-5
