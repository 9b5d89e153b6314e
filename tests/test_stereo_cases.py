"""Dense stereo, no GPU: the cases of tests/stereo_cases.py test something.  Everything here is the numpy reference
(tests/stereo_ref.py) on the deterministic scene: ties exist, the left-right check rejects some pixels and keeps most, the
sub-pixel step moves most pixels, offsets stay within half a pixel, and the recovered disparity is the scene's.  Shares are
of all w h pixels unless they say "of valid pixels"."""
import numpy as np
import pytest

import stereo_cases as C
import stereo_ref as R

SCENE = [n for n, c in C.CASES.items() if c.kind == "scene"]


def share(mask):
    return float(mask.mean()) if mask.size else 0.0


def test_the_case_set_covers_every_setting():
    cases = C.CASES.values()
    assert {c.lr for c in cases} >= {-1, 0, 1}
    assert {c.subpixel for c in cases} == {0, 1}
    assert any(c.max_cost == 0 and c.kind == "identical" and c.dmin == 0 for c in cases)
    assert any(c.w == 2 * c.r + 1 for c in cases)
    assert any(c.w < 2 * c.r + 1 for c in cases) and any(c.h < 2 * c.r + 1 for c in cases)
    assert any(c.D == 256 for c in cases) and any(c.w % 4 == 2 for c in cases) and any(c.w % 2 == 1 and c.r == 15 for c in cases)
    # every lane count per pixel of csrc/stereo.hip: numDisparities up to 8, 16, 32, 64, 128, 256
    assert {max(0, int(np.ceil(np.log2(max(c.D, 8) / 8.0)))) for c in cases} == {0, 1, 2, 3, 4, 5}
    for name in ("base_r1", "base_r4", "odd_pitch_r15", "wide_range"):
        c = C.CASES[name]
        assert (c.w, c.h, c.r, c.dmin, c.D) in {(96, 72, 1, -1, 12), (96, 72, 4, -1, 12), (131, 70, 15, 0, 10), (70, 37, 2, -3, 40)}


def test_the_scene_is_deterministic_and_has_its_parts():
    c = C.CASES["base_r1"]
    left, right = C.scene(c)
    again = C.scene(c)
    assert np.array_equal(left, again[0]) and np.array_equal(right, again[1])
    assert left.dtype == np.uint8 and left.shape == (c.h, c.w)
    assert (left == 255).sum() >= 12 and ((left == 255) & (right == 255)).sum() >= 12   # the saturated block, in both
    assert ((left == 97) & (right == 97)).sum() >= 4 * (c.w - 4)                        # the constant band, in both
    f = C.field(c)
    assert set(np.unique(f)) == {C.FAR, C.NEAR}                                         # two planes: an occlusion edge


def test_ties_exist():
    """a tied minimum on at least 5 % of the pixels of at least one case"""
    shares = {n: share(C.reference(n)["tied"]) for n in SCENE}
    assert max(shares.values()) >= 0.05, shares


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c.lr >= 0])
def test_left_right_check_rejects_some_and_keeps_most(name):
    ref = C.reference(name)
    rejected = share(ref["valid_before_lr"] & ~ref["valid"])
    assert rejected >= 0.01, rejected
    assert share(ref["valid"]) >= 0.30, share(ref["valid"])


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c.subpixel])
def test_subpixel_moves_most_valid_pixels(name):
    ref = C.reference(name)
    v = ref["valid"]
    assert v.any() and share(ref["off"][v] != 0) >= 0.50


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_offsets_stay_within_half_a_pixel(name):
    ref = C.reference(name)
    assert (np.abs(ref["off"]) <= 0.5).all()
    c = C.CASES[name]
    v = ref["valid"]
    d = ref["disparity"][v]
    assert np.isfinite(d).all() and (d >= c.dmin - 0.5).all() and (d <= c.dmin + c.D - 1 + 0.5).all()
    assert (ref["disparity"].view(np.uint32)[~v] == R.NAN_BITS).all() and (ref["cost"][~v] == R.NO_COST).all()
    assert (ref["cost"][v] <= 961 * 255).all()


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if min(c.w, c.h) >= 2 * c.r + 1])
def test_the_scene_field_is_recovered(name):
    ref = C.reference(name)
    v = ref["valid"]
    assert v.any()
    assert share(np.abs(ref["disparity"][v] - C.field(C.CASES[name])[v]) <= 0.5) >= 0.75


def edge_winners(ref, case, name):
    """the valid pixels of a reference whose disparity is not an integer and whose winner k sits at the end of a lane's eight
    disparities that the case is named for: the other lane of the pixel's group holds the sub-pixel neighbour's cost"""
    k = ref["k"]
    moved = ref["valid"] & (ref["disparity"] != np.floor(ref["disparity"]))
    at_edge = (k % 8 == 0) & (k >= 8) if name == "edge_below" else (k % 8 == 7) & (k + 1 < case.D)
    return int((moved & at_edge).sum())


@pytest.mark.parametrize("name", ["edge_below", "edge_above"])
def test_the_edge_cases_take_a_neighbour_from_the_adjacent_lane(name):
    n = edge_winners(C.reference(name), C.CASES[name], name)
    assert n >= 1000, n                                       # measured 1106 and 3932


def test_degenerate_cases():
    for name in ("narrower_than_window", "lower_than_window"):
        assert not C.reference(name)["has"].any()
    ref = C.reference("one_column")
    c = C.CASES["one_column"]
    assert ref["has"].sum() == c.h - 2 * c.r and (ref["k"][ref["has"]] == -c.dmin).all()      # x = r alone, d = 0 alone
    ref = C.reference("exact_only")
    assert ref["valid"].any() and (ref["cost"][ref["valid"]] == 0).all() and (ref["disparity"][ref["valid"]] == 0).all()
    # the same pair without the limit keeps more: the limit decided something
    c = C.CASES["limit"]
    left, right = C.scene(c)
    free = R.disparity_ref(left, right, c.r, c.dmin, c.D, C.NO_LIMIT, c.lr, c.subpixel)
    assert 0 < C.reference("limit")["valid"].sum() < free["valid"].sum()


def test_reference_against_a_direct_window_sum():
    """the integral-image volume against the definition written out, on a small pair"""
    c = C.CASES["wide_range"]
    left, right = C.scene(c)
    vol = R.cost_volume(left, right, c.r, c.dmin, c.D)
    rng = np.random.RandomState(0)
    L, Rr = left.astype(np.int64), right.astype(np.int64)
    for _ in range(300):
        k, y, x = rng.randint(c.D), rng.randint(c.h), rng.randint(c.w)
        d = c.dmin + k
        inside = c.r <= x <= c.w - 1 - c.r and c.r <= y <= c.h - 1 - c.r and c.r <= x - d <= c.w - 1 - c.r
        if not inside:
            assert vol[k, y, x] == R.BIG
            continue
        want = np.abs(L[y - c.r:y + c.r + 1, x - c.r:x + c.r + 1] - Rr[y - c.r:y + c.r + 1, x - d - c.r:x - d + c.r + 1]).sum()
        assert vol[k, y, x] == want
