"""The hole-filling cases test something (no GPU): every deliberate defect of tests/fill_ref.py changes the output of at least one
case of tests/fill_cases.py -- and of the cases named here, which were built to see it -- and the reference itself has the
properties include/ssrlcv_hip.h "hole filling" states."""
import numpy as np
import pytest

import fill_cases as C
import fill_ref as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differs(name, **defect):
    case = C.CASES[name]
    out, filled = R.fill(case.d, case.paths, case.max_gap, case.min_hits, case.rule, **defect)
    ref_out, ref_filled = C.reference(name)
    return not (np.array_equal(bits(out), bits(ref_out)) and np.array_equal(filled, ref_filled))


# defect -> the cases that must see it (small ones: the reference walks every ray)
SEEN_BY = {
    "reverse": (dict(reverse=True), ["dir_%d" % i for i in range(8)] + ["gap_exact_d%d" % i for i in range(8)]),
    "transpose": (dict(transpose=True), ["dir_5", "dir_6", "gap_exact_d5", "gap_exact_d6"]),
    "gap_plus": (dict(gap_off=1), ["star_gap7", "gap_1", "gap_0"] + ["gap_exact_d%d" % i for i in range(8)]),
    "gap_minus": (dict(gap_off=-1), ["star_gap7", "gap_1", "gap_7"] + ["gap_exact_d%d" % i for i in range(8)]),
    "upper": (dict(upper=True), ["checkerboard", "key_order_median", "paths_0f", "column_hole"]),
    "float_order": (dict(float_order=True), ["key_order_min", "key_order_median"]),
    "chained": (dict(chained=True), ["corner_pixel", "star_gap7", "frame", "gap_7", "serpentine", "half_hole", "centre_pixel", "strips_40x150"]),
    "ignore_min_hits": (dict(ignore_min_hits=True), ["paths_ff", "paths_0f", "checkerboard", "paths_03", "equal_hits"]),
}


@pytest.mark.parametrize("defect", sorted(SEEN_BY))
def test_each_defect_is_seen(defect):
    kwargs, names = SEEN_BY[defect]
    for name in names:
        assert differs(name, **kwargs), (defect, name)


def test_the_cases_cover_the_contracts_parameters():
    cases = C.CASES.values()
    assert {1 << i for i in range(8)} | {0x03, 0x0F, 0xF0, 0xFF} <= {c.paths for c in cases}
    assert {0, 1, 7, C.NO_LIMIT} <= {c.max_gap for c in cases}
    assert {C.MIN, C.MEDIAN} == {c.rule for c in cases}
    pop = lambda c: bin(c.paths).count("1")
    assert any(c.min_hits == 1 for c in cases) and any(c.min_hits == pop(c) > 1 for c in cases) and any(1 < c.min_hits < pop(c) for c in cases)
    shapes = {c.d.shape[::-1] for c in cases}
    assert {(1, 1), (1, 37), (41, 1), (63, 9), (64, 9), (65, 9), (129, 17), (257, 5), (97, 83), (83, 97)} <= shapes
    assert all(c.d.size <= 9600 and c.d.dtype == np.float32 for c in cases)
    for c in cases:
        assert 1 <= c.min_hits <= pop(c) and 1 <= c.paths <= 0xFF


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_references_own_properties(name):
    case = C.CASES[name]
    src = bits(case.d)
    out, filled = C.reference(name)
    out = bits(out)
    hole = src == R.INVALID
    assert np.array_equal(out[~hole], src[~hole])                        # measured pixels pass through bit for bit
    assert set(out[hole].tolist()) <= set(src[~hole].tolist()) | {R.INVALID}   # every output value is an input value
    assert np.array_equal(filled == 1, hole & (out != R.INVALID)) and set(filled.ravel().tolist()) <= {0, 1}
    if case.max_gap == 0 or hole.all() or not hole.any():
        assert np.array_equal(out, src) and not filled.any()


def test_max_gap_zero_is_the_identity_and_unlimited_is_the_image():
    case = C.CASES["gap_7"]
    out, filled = R.fill(case.d, case.paths, 0, 1, case.rule)
    assert np.array_equal(bits(out), bits(case.d)) and not filled.any()
    far = R.fill(case.d, case.paths, max(case.d.shape), 1, case.rule)
    unlimited = R.fill(case.d, case.paths, C.NO_LIMIT, 1, case.rule)
    assert np.array_equal(bits(far[0]), bits(unlimited[0])) and np.array_equal(far[1], unlimited[1])


def test_named_expectations():
    out, filled = C.reference("equal_hits")
    assert out[4, 4] == 5.0 and filled[4, 4] == 1
    out, filled = C.reference("star_gap7")
    assert filled.sum() == 8 * 7 and filled[20, 19 + 7] == 1 and filled[20, 19 + 8] == 0 and filled[20 - 7, 19 - 7] == 1
    out, filled = C.reference("corner_pixel")
    h, w = out.shape
    assert filled.sum() == (w - 1) + (h - 1) + (min(w, h) - 1)
    out, filled = C.reference("checkerboard")
    assert filled.sum() > 0 and not C.reference("all_holes")[1].any() and not C.reference("all_valid")[1].any()
    out, filled = C.reference("half_hole")
    assert filled[:, :70].any(axis=1).all()                               # the carry reaches column 0 of every row


def test_the_occlusion_band_takes_the_background():
    """The synthetic pair of tests/test_gpu_fill.py: a background shifted by d0 and a foreground square shifted by d1 > d0.
    The left-right check leaves a band of holes left of the square, the background the right view cannot see; with the
    horizontal directions and rule MIN the band must end on d0.  Printed, and held to the reference's own guarantee only: every
    filled band pixel whose two horizontal hits are d0 and d1 takes d0."""
    import fill_scene as S
    disp = S.reference_disparity()
    out, filled = R.fill(disp, 0x03, 32, 2, R.MIN)
    band = S.occlusion_band() & (bits(disp) == R.INVALID)
    on_d0 = int((out[band] == S.D0).sum())
    print("occlusion band: %d holes, %d filled, %d end on d0 = %d" % (band.sum(), filled[band].sum(), on_d0, S.D0))
    assert band.sum() > 0 and filled[band].sum() > 0
    assert not (out[band & (filled == 1)] == S.D1).any()
