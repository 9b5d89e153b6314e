"""The shift search without a GPU: the numpy restatement of include/ssrlcv_hip.h "shift search" (tests/shift_ref.py) against a
plain loop over cells, the properties the contract states (stride, centre), what the cases of tests/shift_cases.py claim to hold,
and the scene fixtures the section was proposed on."""
import numpy as np
import pytest

import shift_cases as C
import shift_ref as R

LOOP_BUDGET = 300000     # shifts x sampled cells a case may cost the plain loop


def same(a, b):
    return np.array_equal(R.table_bytes(*a), R.table_bytes(*b))


def loop_cost(w, h, p):
    g = p.get("stride", 1)
    return (2 * p["radius"] + 1) ** 2 * (-(-w // g)) * (-(-h // g))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_restatement_equals_the_plain_loop(size):
    w, h = size
    moving, reference = C.pair(w, h)
    ran = 0
    for p in C.PARAMS:
        if loop_cost(w, h, p) > LOOP_BUDGET:
            continue
        assert same(R.search(moving, reference, C.SCALE, **p), R.loop(moving, reference, C.SCALE, **p)), (size, p)
        ran += 1
    assert ran >= 6


def test_the_restatement_equals_the_plain_loop_on_the_special_contents():
    for name, (moving, reference, scale, params) in C.contents().items():
        h, w = moving.shape
        for p in params:
            if loop_cost(w, h, p) <= LOOP_BUDGET:
                assert same(R.search(moving, reference, scale, **p), R.loop(moving, reference, scale, **p)), (name, p)


def test_the_cases_hold_what_they_claim():
    moving, reference = C.pair(130, 35)
    assert 0.25 < np.isnan(moving).mean() < 0.35 and 0.05 < np.isnan(reference).mean() < 0.15
    head, entries = R.search(moving, reference, C.SCALE, radius=7)
    assert head["validMoving"] == np.isfinite(moving).sum() and head["clippedMoving"] == 0
    best = R.pick(entries, C.SCALE, min_overlap=1000)
    assert best["shift"] == (2, -1) and best["second"] > 20 * best["variance"] and abs(best["bias"] - 0.4) < 0.05   # what pair() built
    # the gates pass some differences and not all; a gate of 0 passes only d == centerQ
    free = entries["n"]
    for p in C.PARAMS:
        if p.get("gate_q") is None or p.get("center") is not None:
            continue
        gated = R.search(moving, reference, C.SCALE, **p)[1]
        whole = R.search(moving, reference, C.SCALE, **{k: v for k, v in p.items() if k not in ("gate_q", "center_q")})[1]
        assert 0 < gated["n"].sum() < whole["n"].sum(), p
    assert free.min() > 0
    # centres at the limits and far out: entries of zeros, the head still counts
    for center in ((C.LIMIT, -C.LIMIT), (-C.LIMIT, C.LIMIT), C.FAR):
        head, entries = R.search(moving, reference, C.SCALE, center=center, radius=7)
        assert not R.table_bytes(head, entries)[16:].any() and head["validMoving"] > 0
    # maps smaller than the radius: most entries are zeros
    _, small = R.search(*C.pair(37, 1), C.SCALE, radius=32)
    assert 0 < (small["n"] > 0).sum() <= 73 and small.size == 4225
    # clipping
    clip = C.clip_map()
    q, valid, clipped = R.quantise(clip, C.SCALE)
    assert clipped == C.CLIPPED_IN_CLIP_MAP and clip.size - valid == C.INVALID_IN_CLIP_MAP
    assert q.max() == 65536 and q[q != R.INVALID].min() == -65536                    # t = +-65536 exactly is valid
    assert R.quantise(np.float32([0.5, 1.5, 2.5, -0.5, -1.5]), 1.0)[0].tolist() == [0, 2, 2, 0, -2]   # ties to even
    # the 64-bit sums
    for name, sign in (("wide_plus", 1), ("wide_minus", -1)):
        moving, reference, scale, params = C.contents()[name]
        e = R.search(moving, reference, scale, **params[0])[1][1, 1]
        assert (int(e["n"]), int(e["sum"]), int(e["sumSq"])) == (1 << 18, sign * (1 << 35), 1 << 52)
    # beyond the caps of both launch grids
    moving, reference = C.beyond_caps()
    h, w = moving.shape
    assert (-(-w // C.TILE_W)) * (-(-h // C.TILE_H)) > C.SEARCH_CAP and w * h > C.QUANTISE_CAP * 256
    assert w % C.TILE_W and h % C.TILE_H and C.SEARCH_CAP >= 64 and C.QUANTISE_CAP >= 64
    best = R.pick(R.search(moving, reference, C.SCALE, radius=1)[1], C.SCALE)
    assert best["shift"] == (-1, 1) and best["variance"] == 0.0


@pytest.mark.parametrize("g", [2, 3, 5])
def test_the_table_at_a_stride_is_the_table_of_the_sampled_maps(g):
    for w, h in ((67, 17), (131, 37), (37, 1)):
        assert w % g and (h == 1 or h % g)
        moving, reference = C.pair(w, h)
        for p in (dict(radius=3), dict(radius=2, center=(1, -1), center_q=20, gate_q=100)):
            assert same(R.search(moving, reference, C.SCALE, stride=g, **p), R.search(moving[::g, ::g], reference[::g, ::g], C.SCALE, stride=1, **p))


def test_the_table_about_a_centre_is_a_block_of_the_table_about_zero():
    moving, reference = C.pair(65, 17)
    for center, S in (((5, -3), 4), ((-2, 6), 3), ((0, 1), 0)):
        wide = max(abs(center[0]), abs(center[1])) + S
        _, part = R.search(moving, reference, C.SCALE, center=center, radius=S, center_q=10, gate_q=400)
        _, whole = R.search(moving, reference, C.SCALE, radius=wide, center_q=10, gate_q=400)
        x0, y0 = wide + center[0] - S, wide + center[1] - S
        assert np.array_equal(part, whole[y0:y0 + 2 * S + 1, x0:x0 + 2 * S + 1])


@pytest.mark.parametrize("k", range(3))
def test_the_scene_fixtures(k):
    """accuracy_cases.truth_map() shifted by (7, -5), (-11, 9) and (12, 12) cells with a bias of 0.7 cell: radius 12, 64 quanta a
    cell, overlap 2304.  The measured second / variance is about 2 x 10^4; the bound is 100"""
    moving, reference, scale = C.shifted_truth(C.SCENE_SHIFTS[k])
    _, entries = R.search(moving, reference, scale, radius=C.SCENE_RADIUS)
    best = R.pick(entries, scale, min_overlap=C.SCENE_MIN_OVERLAP)
    print("shift %s: variance %.4f quanta^2, second %.1f, bias %.4f" % (best["shift"], best["variance"] * scale * scale, best["second"] * scale * scale,
                                                                        best["bias"]))
    assert best["shift"] == C.SCENE_SHIFTS[k]
    assert best["second"] >= 100 * best["variance"]
    import dsm_cases as DC
    assert abs(best["bias"] / float(DC.scene_frame().cell) - C.SCENE_BIAS_CELLS) < 0.01
    _, coarse = R.search(moving, reference, scale, stride=4, radius=4)
    assert R.pick(coarse, scale, stride=4, min_overlap=C.SCENE_MIN_OVERLAP // 16)["k"] == C.SCENE_COARSE[k]


def test_the_displaced_scene_through_the_levels():
    """the cloud of the truth map 7.3, -4.6, 0.5 cells and a small rotation off: the levels find (7, -5); with every tenth point
    raised 20 cells the gate keeps the bias where it was, and without it the bias is two cells off"""
    import accuracy_cases as AC
    import dsm_cases as DC
    cell, reference = float(DC.scene_frame().cell), AC.truth_map()
    clean = R.levels(C.displaced_map(False), reference, cell, gate=None)
    assert clean["levels"][-1]["result"]["shift"] == (7, -5) and abs(clean["bias"] / cell + C.MOTION_CELLS[2]) < 0.1
    gated = R.levels(C.displaced_map(True), reference, cell, gate=3.0)
    free = R.levels(C.displaced_map(True), reference, cell, gate=None)
    print("raised points: bias %.3f cells gated, %.3f without a gate; shifts %s and %s" % (gated["bias"] / cell, free["bias"] / cell,
                                                                                           gated["levels"][-1]["result"]["shift"], free["levels"][-1]["result"]["shift"]))
    assert gated["levels"][-1]["result"]["shift"] == (7, -5) and abs(gated["bias"] / cell + C.MOTION_CELLS[2]) < 0.1
    assert gated["levels"][-1]["result"]["n"] < free["levels"][-1]["result"]["n"]      # the gate left the raised cells out
    assert abs(free["bias"] / cell + C.MOTION_CELLS[2]) > 1.5                           # 20 cells x one tenth
    for lv in gated["levels"]:
        assert lv["params"]["gate_q"] != R.NO_GATE
