"""GPU parity off the fixtures: csrc/pointcloud.hip (generate_bundles, triangulate2, triangulateN, ba_sweep2) against the
CPU oracle on the cases of tests/pointcloud_cases.py -- seven or five cameras anywhere with non-square images, key points
of any camera in any order, `index` against bundle order, 2 to 9 lines a bundle, sizes around the wave and the block,
every output combination with sentinel-filled buffers, and the degenerate tables.  Points, errors and flags are compared
bit for bit; an error sum is the butterfly's own value for one wave and within the derived bound on the order of one
atomic per wave otherwise (pointcloud_cases.sum_bound).  tests/test_pointcloud_cases.py proves the cases valid on the
oracle alone."""
import numpy as np
import pytest

import helpers as H
import pointcloud_cases as C

pytestmark = pytest.mark.gpu


def _filled(n):
    import torch
    return torch.full((n,), C.SENTINEL, dtype=torch.int32, device="cuda")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def run_tri(capi, nview, bundles, lines, points=True, errors=True, cutoff=None, esum=True, nev=False, invalid_before=0):
    """one triangulation through the C ABI with caller-owned buffers: sentinel-filled, one element longer than needed, the
    sum zeroed with a sentinel behind it -> dict of what came back (None for what was not asked for)"""
    import torch
    n = len(bundles)
    b = bundles.copy()
    b["invalid"] = invalid_before
    b_d, l_d = capi.to_dev(b), capi.to_dev(lines)
    pts_d = _filled(3 * n + 3) if points else None
    err_d = _filled(n + 1) if errors else None
    sum_d = _filled(2) if esum else None
    if esum:
        sum_d[0] = 0
    cut_d = None if cutoff is None else torch.tensor([cutoff], dtype=torch.float32, device="cuda")
    u32, ci = capi.c_u32, capi.c_int
    if nview:
        capi.check(capi.LIB.ssrlcv_hip_triangulateN(capi.ptr(l_d), capi.ptr(b_d), u32(n), capi.ptr(pts_d), capi.ptr(err_d),
                                                    capi.ptr(cut_d), capi.ptr(sum_d), ci(1 if nev else 0), capi.stream_ptr()))
    else:
        capi.check(capi.LIB.ssrlcv_hip_triangulate2(capi.ptr(l_d), capi.ptr(b_d), u32(n), capi.ptr(pts_d), capi.ptr(err_d),
                                                    capi.ptr(cut_d), capi.ptr(sum_d), capi.stream_ptr()))
    torch.cuda.synchronize()
    out = {"points": None, "errors": None, "sum": None}
    gb = capi.to_host(b_d, H.BUNDLE, n)
    assert np.array_equal(gb["index"], bundles["index"]) and np.array_equal(gb["numLines"], bundles["numLines"])
    out["invalid"] = gb["invalid"]
    assert np.array_equal(capi.to_host(l_d, H.LINE, len(lines)).view(np.uint8), lines.view(np.uint8))   # inputs stay
    if points:
        p = _host(pts_d)
        assert (p[3 * n:] == C.SENTINEL).all()
        out["points"] = p[:3 * n].reshape(n, 3).view(np.float32)
    if errors:
        e = _host(err_d)
        assert e[n] == C.SENTINEL
        out["errors"] = e[:n].view(np.float32)
    if esum:
        s = _host(sum_d)
        assert s[1] == C.SENTINEL
        out["sum"] = s[:1].view(np.float32)[0]
    return out


def _equal(got, want):
    return np.array_equal(H.bits(got), H.bits(want))


def check_against(out, ref, what=""):
    """whatever came back equals the oracle's: points and errors in bits (NaN for NaN), flags, and the sum by its structure"""
    if out["points"] is not None:
        bad = np.flatnonzero(~C.same(out["points"], ref["points"]).all(1))
        assert not len(bad), (what, "points", bad[:5], out["points"][bad[:5]], ref["points"][bad[:5]])
    if out["errors"] is not None:
        bad = np.flatnonzero(~C.same(out["errors"], ref["errors"]))
        assert not len(bad), (what, "errors", bad[:5], out["errors"][bad[:5]], ref["errors"][bad[:5]])
    assert np.array_equal(out["invalid"], ref["invalid"]), (what, "invalid", np.flatnonzero(out["invalid"] != ref["invalid"])[:5])
    if out["sum"] is not None:
        ok, text = C.sum_agrees(out["sum"], ref["errors"])
        print(what, "error sum:", text)
        assert ok, (what, text)


# ---- 1. generate_bundles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.GEN_SIZES)
def test_generate_bundles_off_the_fixtures(capi, oracle_lib, n):
    import torch
    cams, mm, kp = C.bundle_input(n)
    ob, ol, _ = H.oracle_bundles(oracle_lib, mm, kp, cams)
    nk = len(kp)
    b_d, l_d = _filled(3 * (n + 1)), _filled(6 * (nk + 1))
    mm_d, kp_d, cam_d = capi.to_dev(mm), capi.to_dev(kp), capi.to_dev(cams)    # named: a raw pointer keeps no tensor alive
    capi.check(capi.LIB.ssrlcv_hip_generate_bundles(capi.ptr(mm_d), capi.ptr(kp_d), capi.c_u32(n), capi.ptr(cam_d),
                                                    capi.c_u32(len(cams)), capi.ptr(b_d), capi.ptr(l_d), capi.stream_ptr()))
    torch.cuda.synchronize()
    lraw, braw = _host(l_d), _host(b_d)
    assert (lraw[6 * nk:] == C.SENTINEL).all() and (braw[3 * n:] == C.SENTINEL).all()      # the element past the end
    gl, gb = lraw[:6 * nk].view(H.LINE), braw[:3 * n].view(H.BUNDLE)
    assert _equal(gl["pnt"], ol["pnt"])
    bad = np.flatnonzero((H.bits(gl["vec"]) != H.bits(ol["vec"])).any(1))
    assert not len(bad), (bad[:5], gl["vec"][bad[:5]], ol["vec"][bad[:5]])
    assert np.array_equal(gb["numLines"], ob["numLines"]) and np.array_equal(gb["index"], ob["index"])
    assert np.array_equal(gb["invalid"], ob["invalid"]) and (gb["invalid"] == 0).all()


# ---- 2. triangulate2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.TRI_SIZES)
def test_triangulate2_every_output_combination(capi, oracle_lib, n):
    b, l = C.two_view_input(oracle_lib, n)
    free = C.triangulate_ref(oracle_lib, False, b, l)
    cut = C.pick_cutoff(free["errors"])
    flagged = C.triangulate_ref(oracle_lib, False, b, l, cutoff=cut)
    at = np.flatnonzero(free["errors"] == np.float32(cut))
    assert len(at) and (flagged["invalid"][at] == 0).all()                      # the bundle the cutoff was taken from stays
    if n > 1:
        assert 0 < flagged["invalid"].sum() < n
    # points only (the flags are reset: the two-view kernel writes 0 without a cutoff, like the oracle)
    check_against(run_tri(capi, False, b, l, errors=False, esum=False, invalid_before=1), free, "n %d points only" % n)
    # errors only
    check_against(run_tri(capi, False, b, l, points=False, invalid_before=1), free, "n %d errors only" % n)
    # void with cutoff: flags and the sum alone
    check_against(run_tri(capi, False, b, l, points=False, errors=False, cutoff=cut), flagged, "n %d void" % n)
    # everything
    check_against(run_tri(capi, False, b, l, cutoff=cut, invalid_before=1), flagged, "n %d everything" % n)


# ---- 3. triangulateN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.TRI_SIZES)
def test_triangulateN_every_output_combination(capi, oracle_lib, n):
    b, l = C.n_view_input(oracle_lib, n)
    free = C.triangulate_ref(oracle_lib, True, b, l, invalid_before=1)          # no cutoff: the flags are left alone
    cut = C.pick_cutoff(free["errors"])
    flagged = C.triangulate_ref(oracle_lib, True, b, l, cutoff=cut, invalid_before=1)
    at = np.flatnonzero(free["errors"] == np.float32(cut))
    assert len(at) and (flagged["invalid"][at] == 0).all()
    if n > 1:
        assert 0 < flagged["invalid"].sum() < n
    check_against(run_tri(capi, True, b, l, errors=False, esum=False, invalid_before=1), free, "n %d points only" % n)
    check_against(run_tri(capi, True, b, l, points=False, invalid_before=1), free, "n %d errors only" % n)
    check_against(run_tri(capi, True, b, l, points=False, errors=False, cutoff=cut, invalid_before=1), flagged, "n %d void" % n)
    check_against(run_tri(capi, True, b, l, cutoff=cut, invalid_before=1), flagged, "n %d everything" % n)
    # noErrorVariant: the points alone; errors, the sum and (no S is singular here) the flags stay as they were
    out = run_tri(capi, True, b, l, cutoff=cut, nev=True)
    assert _equal(out["points"], free["points"])
    assert (H.bits(out["errors"]) == C.SENTINEL).all() and H.bits(out["sum"]) == 0
    assert (out["invalid"] == 0).all()


# ---- 4. degenerate tables --------------------------------------------------------------------------------------------------
def _two_view_degenerate_cases(lib):
    b, l, classes = C.degenerate_two_view()
    yield "alone", b, l, dict(enumerate(classes))
    for first in C.embedded_firsts(False):
        yield ("embedded %d" % first,) + C.embedded(lib, False, first)


def test_triangulate2_degenerate_rows(capi, oracle_lib):
    for what, b, l, at in _two_view_degenerate_cases(oracle_lib):
        for cutoff in (None, 1.0):
            ref = C.triangulate_ref(oracle_lib, False, b, l, cutoff=cutoff)
            out = run_tri(capi, False, b, l, cutoff=cutoff, invalid_before=1)
            check_against(out, ref, "two-view %s cutoff %s" % (what, cutoff))
            for g, c in at.items():
                pt, e, inv = out["points"][g], out["errors"][g], out["invalid"][g]
                if c == "nan":
                    assert np.isnan(pt).all() and np.isnan(e) and inv == 0, (what, g, pt, e, inv)
                elif c == "inf":
                    assert np.isfinite(pt).all() and np.isposinf(e) and inv == (cutoff is not None), (what, g, pt, e, inv)
                else:
                    assert np.isfinite(pt).all() and np.isfinite(e), (what, g, pt, e)
            classes = set(at.values())
            want = np.nan if "nan" in classes else np.inf if "inf" in classes else None
            if want is not None:
                assert C.same(out["sum"], np.float32(want)), (what, out["sum"])
            else:
                assert np.isfinite(out["sum"])
            # the void form of the same: flags and sum alone
            void = run_tri(capi, False, b, l, points=False, errors=False, cutoff=cutoff, invalid_before=1)
            check_against(void, ref, "two-view %s void cutoff %s" % (what, cutoff))


def _n_view_degenerate_cases(lib):
    b, l, classes = C.degenerate_n_view()
    yield "alone", b, l, dict(enumerate(classes))
    for first in C.embedded_firsts(True):
        yield ("embedded %d" % first,) + C.embedded(lib, True, first)


def test_triangulateN_degenerate_rows(capi, oracle_lib):
    for what, b, l, at in _n_view_degenerate_cases(oracle_lib):
        singular = np.zeros(len(b), bool)
        singular[[g for g, c in at.items() if c == "singular"]] = True
        for cutoff in (None, 0.25):
            ref = C.triangulate_ref(oracle_lib, True, b, l, cutoff=cutoff)
            assert np.array_equal((H.bits(ref["points"]) == C.SENTINEL).all(1), singular)
            out = run_tri(capi, True, b, l, cutoff=cutoff)
            check_against(out, ref, "n-view %s cutoff %s" % (what, cutoff))
            # a singular S leaves the point unwritten and takes the error from (0, 0, 0)
            assert np.array_equal((H.bits(out["points"]) == C.SENTINEL).all(1), singular)
            for g in np.flatnonzero(singular):
                assert out["errors"][g] == np.float32(0.5) and out["invalid"][g] == (cutoff is not None)
            for g, c in at.items():
                if c == "nan":
                    assert np.isnan(out["errors"][g]) and out["invalid"][g] == 0 and np.isfinite(out["points"][g]).all()
            assert np.isnan(out["sum"]) == ("nan" in at.values())
        # noErrorVariant: the singular bundle alone is flagged, its neighbours are not; nothing else is written
        out = run_tri(capi, True, b, l, nev=True)
        assert np.array_equal(out["invalid"] != 0, singular) and singular.sum() <= 1
        assert C.same(out["points"], ref["points"]).all()
        assert (H.bits(out["errors"]) == C.SENTINEL).all() and H.bits(out["sum"]) == 0


# ---- 5. ba_sweep2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", C.SWEEP_CASES)
def test_ba_sweep2_every_set_against_its_own_reference(capi, oracle_lib, n, K):
    """Five cameras, pairs from any two of them in either order, K sets that each move every camera: all K sums, bit-equal
    to the butterfly's value where a set is one wave (n <= 64; at n = 1 that is the fused make_line -> two_view_point chain
    of one bundle) and within sum_bound of the exact sum of its wave partials otherwise."""
    cams, mm, kp, params = C.sweep_input(n, K)
    partials = C.sweep_partials(oracle_lib, n, K)
    sums = capi.ba_sweep2(capi.to_dev(mm), capi.to_dev(kp), n, capi.to_dev(cams), len(cams), capi.to_dev(params), K).cpu().numpy()
    miss = C.sums_within(sums, partials)
    ref, bound = C.sum_reference(partials), C.sum_bound(partials)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, np.abs(sums - ref) / bound, 0.0)))
    print("ba_sweep2 n %d K %d: %d sets miss; largest |sum - reference| / bound %.3f" % (n, K, len(miss), worst))
    assert not len(miss), (n, K, miss[:8], sums[miss[:8]], ref[miss[:8]], bound[miss[:8]])


def test_ba_sweep2_empty_inputs(capi):
    import torch
    cams, mm, kp, params = C.sweep_input(64, 7)
    mm_d, kp_d, cam_d, par_d = capi.to_dev(mm), capi.to_dev(kp), capi.to_dev(cams), capi.to_dev(params)

    def sweep(n, K, sums_d):
        capi.check(capi.LIB.ssrlcv_hip_ba_sweep2(capi.ptr(mm_d), capi.ptr(kp_d), capi.c_u32(n), capi.ptr(cam_d), capi.c_u32(len(cams)),
                                                 capi.ptr(par_d), capi.c_u32(K), capi.ptr(sums_d), capi.c_vp(0), capi.c_sz(0),
                                                 capi.stream_ptr()))
        torch.cuda.synchronize()
        return _host(sums_d)

    assert (sweep(64, 0, _filled(8)) == C.SENTINEL).all()                      # K = 0: OK, nothing touched
    got = sweep(0, 7, _filled(8))                                              # n = 0: the K sums come back zero
    assert (got[:7] == 0).all() and got[7] == C.SENTINEL
