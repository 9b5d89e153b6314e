"""CPU only, on the numpy reference alone (tests/census_ref.py): the cases of tests/census_cases.py test what their names
say, so a kernel that passes tests/test_gpu_census.py has been through every seam; and the property the census cost is built
for -- it does not move under a strictly increasing map of one image's grey levels -- holds where SAD falls apart."""
import numpy as np
import pytest

import census_cases as C
import census_ref as CR
import stereo_ref as R

BIG = CR.BIG


def test_the_code_is_the_contracts_bit_order():
    """a hand-made 3 x 3 and 5 x 5 window: bit b = row-major offset index, the centre skipped, strictly darker"""
    img = np.array([[9, 1, 9], [1, 5, 5], [9, 9, 0]], np.uint8)
    T = CR.census(img, 1)
    assert T[1, 1] == (1 << 1) | (1 << 3) | (1 << 7) and (T.ravel() != 0).sum() == 1      # (0,-1), (-1,0), (1,1); equal is not darker
    img = np.full((5, 5), 7, np.uint8)
    img[0, 0], img[2, 1], img[2, 3], img[4, 4] = 0, 0, 0, 0
    assert CR.census(img, 2)[2, 2] == (1 << 0) | (1 << 11) | (1 << 12) | (1 << 23)       # the centre is skipped between 11 and 12
    assert CR.census(np.zeros((6, 6), np.uint8), 3).shape == (6, 6) and not CR.census(np.zeros((6, 6), np.uint8), 3).any()
    assert CR.popcount(np.array([0, 1, 0xFFFFFFFFFFFF, 1 << 47, 0xF0F0], np.uint64)).tolist() == [0, 1, 48, 1, 8]


@pytest.mark.parametrize("name,c", [("c1_r0", 1), ("c2_r0", 2), ("c3_r0", 3)])
def test_the_bound_is_reached_without_aggregation(name, c):
    V = C.reference(name)["volume"]
    assert int(V[V < BIG].max()) == CR.bits(c) == {1: 8, 2: 24, 3: 48}[c]
    if c == 3:
        assert (V[V < BIG] > 32).mean() > 0.01      # the upper dword of the code counts


@pytest.mark.parametrize("name", C.ALL)
def test_costs_stay_inside_the_contracts_bound(name):
    c = C.CASES[name]
    V = C.reference(name)["volume"]
    if (V < BIG).any():
        assert 0 <= V.min() and int(V[V < BIG].max()) <= CR.bits(c.c) * (2 * c.r + 1) ** 2 <= 10800


@pytest.mark.parametrize("name", C.TIE_PRONE)
def test_tie_prone_cases_have_tied_winners(name):
    ref = C.reference(name)
    share = ref["tied"].sum() / ref["has"].sum()
    assert share > 0.10, share
    if name == "flat":
        # every pixel with more than one candidate ties (the leftmost interior column has d = 0 alone), and the smallest wins
        assert share > 0.95 and (ref["k"][ref["has"]] == 0).all() and not ref["volume"][ref["volume"] < BIG].any()


@pytest.mark.parametrize("name", sorted(C.EDGE))
def test_edge_cases_put_winners_on_the_lane_boundary(name):
    ref, k = C.reference(name), C.EDGE[name]
    on = (ref["k"] == k) & ref["both"] & ref["valid"]
    assert on.sum() > 500, int(on.sum())
    assert (ref["off"][on] != 0).sum() > 100          # and the parabola moves them


def test_the_limit_invalidates_a_share():
    ref = C.reference("limit_100")
    share = 1.0 - ref["valid"].sum() / ref["has"].sum()
    assert 0.01 < share < 0.5, share
    # maxCost 0: the comparison C* <= maxCost at its edge.  On the identical pair nothing is cut; on the scene only the exact
    # winners stay, which a call that lost its limit would not show
    assert C.CASES["exact_only"].max_cost == 0 and C.CASES["exact_on_scene"].max_cost == 0 and C.CASES["limit_100"].max_cost == 100
    exact = C.reference("exact_only")
    assert exact["valid"].sum() > 1000 and (exact["cost"][exact["valid"]] == 0).all()
    assert np.array_equal(exact["valid_before_lr"], exact["has"])
    cut = C.reference("exact_on_scene")
    best = cut["volume"].min(0)
    assert np.array_equal(cut["valid_before_lr"], cut["has"] & (best == 0))
    kept = cut["valid_before_lr"].sum() / cut["has"].sum()
    print("maxCost 0 on the scene keeps %.3f of the winners" % kept)
    assert 0 < cut["valid_before_lr"].sum() < cut["has"].sum() and cut["valid"].sum() > 0
    assert (cut["cost"][cut["valid"]] == 0).all() and (cut["cost"][~cut["valid"]] == 0xFFFFFFFF).all()


def test_the_degenerate_cases_are_what_they_say():
    one = C.reference("one_column")
    assert one["has"].sum() == 30 - 8 and (one["has"].nonzero()[1] == 4).all()
    row = C.reference("one_row")
    assert (row["has"].nonzero()[0] == 2).all() and row["has"].sum() == 40 - 4
    for name in ("narrower_than_footprint", "lower_than_footprint"):
        assert not C.reference(name)["has"].any()
        assert (C.reference(name)["disparity"].view(np.uint32) == CR.NAN_BITS).all()


def test_every_code_width_and_ring_is_met():
    cs = {(c.c, c.r) for c in C.CASES.values()}
    assert {(1, 0), (2, 0), (3, 0), (2, 2), (3, 1), (1, 7), (3, 7), (2, 1)} <= cs
    assert {c.c for c in C.SGM_CASES.values()} == {1, 2, 3}
    nD = lambda D: max(1, 1 << int(np.ceil(np.log2(max(D, 8) / 8))))
    assert {nD(c.D) for c in C.CASES.values() if (c.c, c.r) == (3, 7)} >= {1, 2, 4}    # the halved strip at 32, 64 and 128 threads
    assert {nD(c.D) for c in C.CASES.values()} == {1, 2, 4, 16, 32}


def test_sgm_cases_are_what_they_say():
    for name, c in C.SGM_CASES.items():
        assert bin(c.paths).count("1") * (c.clamp + c.P2) <= 65535, name
    b = C.SGM_CASES["bound_3paths"]
    assert bin(b.paths).count("1") * (b.clamp + b.P2) == 65535
    assert C.sgm_reference("clamp_bites")["clamped"] > 0.05
    assert C.sgm_reference("c2_r0_8paths")["clamped"] == 0.0
    p0 = C.SGM_CASES["p0_8paths"]
    assert p0.P1 == p0.P2 == 0 and p0.clamp >= CR.bits(p0.c) * (2 * p0.r + 1) ** 2 and C.sgm_reference("p0_8paths")["clamped"] == 0.0
    zero = C.sgm_reference("clamp0")
    assert zero["has"].sum() > 5000 and (zero["cost"][zero["valid"]] == 0).all()
    assert not C.sgm_reference("narrower_than_footprint")["has"].any()
    assert C.sgm_reference("one_column")["has"].sum() == 22 and C.sgm_reference("one_row")["has"].sum() == 36
    assert C.SGM_CASES["d1"].D == 1 and C.sgm_reference("d1")["valid"].sum() > 100
    # aggregation changes the winners: it is not the block-matching call in disguise
    wta = CR.census_disparity_ref(*C.scene(C.SGM_CASES["c2_r0_8paths"]), 2, 0, -1, 12, lr=1, subpixel=1)
    assert (wta["k"] != C.sgm_reference("c2_r0_8paths")["k"]).mean() > 0.05


def test_without_penalties_the_sum_is_the_block_matching_cost():
    for name in ("p0_4paths", "p0_8paths"):
        c = C.SGM_CASES[name]
        left, right = C.scene(c)
        bm = CR.census_disparity_ref(left, right, c.c, c.r, c.dmin, c.D, lr=c.lr, subpixel=c.subpixel)
        sg = C.sgm_reference(name)
        assert np.array_equal(bm["disparity"].view(np.uint32), sg["disparity"].view(np.uint32))
        want = np.where(bm["cost"] == 0xFFFFFFFF, bm["cost"].astype(np.int64), bm["cost"].astype(np.int64) * bin(c.paths).count("1"))
        assert np.array_equal(sg["cost"].astype(np.int64), want)


def test_radiometric_invariance():
    """both images halved, the right one through 2 v + 1 and through v + 100: the census costs do not move, the winners
    recover the scene; SAD at the same footprint is lost on the gained pair"""
    case, field, pairs = C.radiometric_pairs()
    vols = [CR.cost_volume(l, r, 2, 2, case.dmin, case.D) for l, r in pairs]
    assert np.array_equal(vols[0], vols[1]) and np.array_equal(vols[0], vols[2])
    win = CR.winners(vols[0], case.dmin)
    hit = ((case.dmin + win["k"]) == field) & win["has"]
    share = hit.sum() / win["has"].sum()
    print("census (2, 2) recovers %.3f of the field" % share)
    assert share >= 0.80
    sad = R.disparity_ref(pairs[1][0], pairs[1][1], 4, case.dmin, case.D)
    sad_share = (((case.dmin + sad["k"]) == field) & sad["has"]).sum() / sad["has"].sum()
    print("SAD radius 4 on the gained pair recovers %.3f" % sad_share)
    assert sad_share <= 0.20
