"""The semi-global-matching cases on the numpy reference alone (no GPU): they prove that tests/sgm_cases.py tests something --
that aggregation changes the winners, that the paths, penalties, clamp, left-right check and sub-pixel step all act -- and
hold tests/sgm_ref.py itself to a direct, loop-per-pixel evaluation of the contract.  The figures beside the assertions were
measured with the committed reference on base_r1 at costClamp 1000, P1 40, P2 400, 8 paths, lrTolerance 1."""
import numpy as np
import pytest

import sgm_cases as C
import sgm_ref as G
import stereo_cases as SC
import stereo_ref as R


def popcount(x):
    return bin(x).count("1")


def test_the_winners_differ_from_sads():
    g, s = C.reference("base_r1"), SC.reference("base_r1")
    has = g["has"]
    assert np.array_equal(has, s["has"])                      # the same pixels have candidates
    assert (g["k"] != s["k"])[has].mean() > 0.05              # measured 0.158


def test_four_and_eight_paths_differ():
    g8, g4 = C.reference("base_r1"), C.reference("base_r1_4paths")
    assert (g8["k"] != g4["k"])[g8["has"]].mean() > 0.01      # measured 0.051
    assert not np.array_equal(g8["cost"], g4["cost"])


def test_p1_equal_to_p2_changes_the_winners():
    g, e = C.reference("base_r1"), C.reference("p1_equals_p2")
    assert (g["k"] != e["k"])[g["has"]].mean() > 0.01         # measured 0.037


def test_the_eight_directions_give_pairwise_different_cost_maps():
    costs = [C.reference("dir%d" % i)["cost"] for i in range(8)]
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(costs[i], costs[j]), (i, j)


def test_the_clamp_engages_somewhere():
    assert 0.001 < C.reference("base_r1")["clamped"] < 0.5    # measured 0.0047 of the defined costs
    assert C.reference("clamp0")["clamped"] > 0.5             # costClamp 0 cuts every cost that is not 0 already


def test_the_lr_check_rejects_some_pixels_and_keeps_most():
    g = C.reference("base_r1")
    before, after = int(g["valid_before_lr"].sum()), int(g["valid"].sum())
    assert before > after > 0.9 * before                      # measured 6580 -> 6329


def test_the_subpixel_step_moves_most_valid_pixels():
    g = C.reference("base_r1")
    assert (g["off"][g["valid"]] != 0).mean() > 0.9           # measured 0.973
    assert (np.abs(g["off"]) <= 0.5).all()                    # S* is the minimum


@pytest.mark.parametrize("name", C.ALL)
def test_every_case_respects_the_bounds(name):
    c, g = C.CASES[name], C.reference(name)
    assert c.P1 <= c.P2 and popcount(c.paths) * (c.clamp + c.P2) <= 65535
    assert g["lmax"] <= c.clamp + c.P2                        # item 3
    valid = g["valid"]
    if valid.any():
        assert g["cost"][valid].max() <= popcount(c.paths) * (c.clamp + c.P2)   # item 4
    r = c.r
    border = np.ones((c.h, c.w), bool)
    border[r:c.h - r, r:c.w - r] = False
    assert not g["has"][border].any()


def test_two_cases_sit_on_the_bound_itself():
    for name in ("bound_3paths", "bound_1path"):
        c = C.CASES[name]
        assert popcount(c.paths) * (c.clamp + c.P2) == 65535
    assert C.reference("bound_1path")["lmax"] == 65535        # a 16-bit entry is filled to its last value
    c = C.CASES["bound_4paths"]
    assert 4 * (c.clamp + c.P2) == 65532                      # four paths: 16383 each is the most that fits


@pytest.mark.parametrize("name", ["edge_below", "edge_above"])
def test_the_edge_cases_take_a_neighbour_from_the_adjacent_lane(name):
    """as tests/test_stereo_cases.py counts it, on the winners of the summed costs"""
    from test_stereo_cases import edge_winners
    n = edge_winners(C.reference(name), C.CASES[name], name)
    assert n >= 1000, n                                       # measured 1102 and 4458


def test_the_constant_band_is_what_aggregation_repairs():
    c = C.CASES["base_r1"]
    g, s = C.reference("base_r1"), SC.reference("base_r1")
    truth = SC.field(SC.CASES["base_r1"]) - c.dmin
    band = np.zeros((c.h, c.w), bool)
    b0 = (3 * c.h) // 5
    band[b0:b0 + max(4, c.h // 6), 2:c.w - 2] = True          # stereo_cases.scene's band
    has = g["has"]
    sgm_band, sad_band = (g["k"] == truth)[band & has].mean(), (s["k"] == truth)[band & has].mean()
    sgm_rest, sad_rest = (g["k"] == truth)[~band & has].mean(), (s["k"] == truth)[~band & has].mean()
    assert sgm_band >= 2 * sad_band and sad_band > 0.05       # measured 0.611 against 0.162
    assert sgm_rest >= sad_rest - 0.01                        # measured 0.947 against 0.942


@pytest.mark.parametrize("name", ["p0_4paths", "p0_8paths"])
def test_without_penalties_it_is_sad(name):
    """P1 = P2 = 0 and a clamp no 3 x 3 cost reaches (9 x 255 = 2295): L_i = C, S = popcount(paths) C"""
    c = C.CASES[name]
    assert c.clamp == 9 * 255 and c.r == 1
    left, right = C.scene(c)
    s = R.disparity_ref(left, right, c.r, c.dmin, c.D, lr=c.lr, subpixel=c.subpixel)
    g = C.reference(name)
    assert np.array_equal(g["disparity"].view(np.uint32), s["disparity"].view(np.uint32))
    want = np.where(s["valid"], s["cost"].astype(np.int64) * popcount(c.paths), 0xFFFFFFFF)
    assert np.array_equal(g["cost"].astype(np.int64), want)


@pytest.mark.parametrize("name", ["flat", "clamp0"])
def test_ties_go_to_the_smallest_candidate(name):
    c, g = C.CASES[name], C.reference(name)
    left, right = C.scene(c)
    cand = R.cost_volume(left, right, c.r, c.dmin, c.D) < R.BIG
    has = cand.any(0)
    assert has.sum() > 500 and np.array_equal(has, g["has"])
    assert np.array_equal(g["k"][has], cand.argmax(0)[has])   # the first candidate
    assert (g["off"] == 0).all()                              # den = 0 everywhere
    assert (g["cost"][g["valid"]] == 0).all() if name == "clamp0" else True


@pytest.mark.parametrize("name", ["narrower_than_window", "lower_than_window"])
def test_an_image_below_one_window_is_all_invalid(name):
    g = C.reference(name)
    assert (g["disparity"].view(np.uint32) == G.NAN_BITS).all() and (g["cost"] == G.NO_COST).all()


def test_diagonals_of_one_pixel():
    """an interior one pixel wide or high: every diagonal path is a single pixel, so a diagonal's L is M itself"""
    for name in ("one_column", "one_row"):
        c = C.CASES[name]
        left, right = C.scene(c)
        M, _ = G.matching_cost(R.cost_volume(left, right, c.r, c.dmin, c.D), c.r, c.clamp)
        assert 1 in M.shape[:2]
        for i in range(4, 8):
            assert np.array_equal(G.path_cost(M, *G.DIRECTIONS[i], c.P1, c.P2), M)


def direct(left, right, r, dmin, D, clamp, P1, P2, paths):
    """items 1-5 pixel by pixel, path by path: -> (k winners with -1 for none, S* with -1 for none)"""
    h, w = left.shape
    L, Rr = left.astype(int), right.astype(int)
    inside = lambda x, y: r <= x <= w - 1 - r and r <= y <= h - 1 - r

    def M(x, y, k):
        d = dmin + k
        if not (r <= x - d <= w - 1 - r):
            return clamp, False
        cost = sum(abs(L[y + j, x + i] - Rr[y + j, x + i - d]) for j in range(-r, r + 1) for i in range(-r, r + 1))
        return min(cost, clamp), True

    S = {}
    for y in range(r, h - r):
        for x in range(r, w - r):
            S[x, y] = [0] * D
    for i, (dx, dy) in enumerate(G.DIRECTIONS):
        if not (paths >> i) & 1:
            continue
        done = {}

        def Lp(x, y):
            if (x, y) in done:
                return done[x, y]
            m_ = [M(x, y, k)[0] for k in range(D)]
            qx, qy = x - dx, y - dy
            if not inside(qx, qy):
                out = m_
            else:
                q = Lp(qx, qy)
                m = min(q)
                out = []
                for k in range(D):
                    terms = [q[k], m + P2]
                    if k >= 1:
                        terms.append(q[k - 1] + P1)
                    if k <= D - 2:
                        terms.append(q[k + 1] + P1)
                    out.append(m_[k] + min(terms) - m)
            done[x, y] = out
            return out

        for (x, y) in S:
            S[x, y] = [a + b for a, b in zip(S[x, y], Lp(x, y))]
    kw = -np.ones((h, w), int)
    sw = -np.ones((h, w), int)
    for (x, y), s in S.items():
        best = None
        for k in range(D):
            if M(x, y, k)[1] and (best is None or s[k] < s[best]):
                best = k
        if best is not None:
            kw[y, x], sw[y, x] = best, s[best]
    return kw, sw


@pytest.mark.parametrize("paths", [0xFF, 0x0F, 0x10, 0x20, 0x40, 0x80, 0x05])
def test_the_reference_equals_a_direct_evaluation(paths):
    c = C.Case(12, 9, 1, -2, 5, 600, 30, 250, paths, -1, 0, "scene", 31)
    left, right = C.scene(c)
    g = G.sgm_ref(left, right, c.r, c.dmin, c.D, c.clamp, c.P1, c.P2, paths)
    kw, sw = direct(left, right, c.r, c.dmin, c.D, c.clamp, c.P1, c.P2, paths)
    assert (kw >= 0).sum() > 50 and len(set(kw[kw >= 0].tolist())) > 2
    assert np.array_equal(g["k"], kw)
    assert np.array_equal(np.where(g["has"], g["cost"].astype(np.int64), -1), sw)
