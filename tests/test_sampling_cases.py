"""The sampling cases, no GPU: tests/sampling_cases.py reaches what it claims.  Everything here is the CPU oracle: the feature
counts and window ranges of the plan-parameter cases (so that a case cannot silently degenerate), the per-key-point reference
chain against OracleSift.features, and for every hand-placed set the preconditions that keep the kernels inside memory and what
the placements reach (windows at coordinate -1 and W, key points without an orientation and with several, no empty descriptor).
Run with -s to see the figures."""
import numpy as np
import pytest

import helpers as H
import sampling_cases as C

f32 = np.float32


def test_the_case_tables_cover_what_they_are_there_for():
    cases = C.PLAN_CASES.values()
    assert len(C.PLAN_CASES) == 14
    assert {c.maxo for c in cases} == {1, 2, 3, 4}
    assert {0.1, 0.4, 1.5, 5.0} <= {c.ow for c in cases} and {0.2, 0.5, 1.0, 6.0, 12.0, 30.0} <= {c.dw for c in cases}
    assert any(c.ow == 5.0 and c.dw == 30.0 for c in cases) and any(c.ow == 0.1 and c.dw == 0.2 and c.maxo == 1 for c in cases)
    assert set(C.WIDE_IMAGE_CASES) == {"maxo3", "ow0.1", "ow5", "dw0.2", "dw30", "both_max", "both_min"}
    assert set(C.ENTRY_POINT_CASES + C.SCHEDULE_CASES) <= set(C.PLAN_CASES)
    assert sorted(C.EXPORT_CASES.values()) == [(4, 0.8, 0.4, 1.0), (4, 0.8, 5.0, 30.0)]
    assert set(C.PAIRS.values()) == {(1.5, 6.0), (0.4, 1.0), (5.0, 30.0), (0.1, 0.2)}
    assert set(C.SEGMENT_SIZES.values()) == {(1, 0, 1), (63, 64, 65), (15, 16, 17)}


@pytest.mark.parametrize("name", list(C.PLAN_CASES))
def test_plan_case_counts_and_window_ranges(name):
    """the oracle's feature count on the 256 x 192 image and the half-widths of the windows the case runs"""
    c = C.PLAN_CASES[name]
    n = len(C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw))
    ori, desc, kept = C.window_ranges("256x192", c.ow, c.dw)
    print("%s: %d features of %d key points, orientation half-width %d..%d, descriptor half-width %d..%d (%s)"
          % (name, n, kept, ori[0], ori[1], desc[0], desc[1], c.why))
    assert n == c.features
    assert desc == c.desc
    if c.ori is not None:
        assert ori == c.ori
    else:       # fewer key points pass checkKeyPoints at this dw: a sub-range of the row with the same ow
        full = (27, 72) if c.ow == 5.0 else (9, 22)
        assert full[0] <= ori[0] <= ori[1] <= full[1]
    if name == "thr1.0":
        assert n == kept == 838      # the stage-5 count the existing tests assert at the defaults
    if name in ("dw30", "both_max"):
        lists = C.checked_lists("256x192", c.dw)
        assert len(lists[0][0]) > 0 and len(lists[1][0]) > 0 and len(lists[2][0]) == 0 and len(lists[3][0]) == 0
    if name == "dw0.5":
        sizes = np.concatenate([C.desc_half(l["sigma"], c.dw, C.oracle_scale_space("256x192").octave_info(o)[2])
                                for o, (l, _) in enumerate(C.checked_lists("256x192", c.dw))])
        assert int((sizes == 1).sum()) == 172


@pytest.mark.parametrize("name", C.WIDE_IMAGE_CASES)
def test_plan_cases_on_the_wide_image_do_not_degenerate(name):
    c = C.PLAN_CASES[name]
    n = len(C.oracle_features("384x256", c.maxo, c.thr, c.ow, c.dw))
    ori, desc, kept = C.window_ranges("384x256", c.ow, c.dw)
    print("%s on 384 x 256: %d features of %d key points, orientation half-width %d..%d, descriptor half-width %d..%d"
          % (name, n, kept, ori[0], ori[1], desc[0], desc[1]))
    assert n > 200 and kept > 100
    if c.dw == 0.2:
        assert desc == (1, 1)
    if c.dw == 30.0:
        assert desc[1] >= 100
    if c.ow == 0.1:
        assert ori == (1, 2)
    if c.ow == 5.0:
        assert ori[1] >= 60


@pytest.mark.parametrize("name", ["ow0.4", "dw0.5", "dw30"])
def test_the_chain_reference_reproduces_the_oracle_features(name):
    """checkKeyPoints in numpy on the stage-4 list + the per-key-point oracle calls == OracleSift.features, byte for byte:
    the reference the hand-placed sets are held to is the oracle's own chain"""
    c = C.PLAN_CASES[name]
    s = C.oracle_scale_space("256x192")
    levels = {o: [s.level(2, o, b) for b in range(5)] for o in range(4)}
    geoms = [s.octave_info(o)[:3] for o in range(4)]
    ref = C.chain_reference(levels, geoms, [l for l, _ in C.checked_lists("256x192", c.dw)], c.maxo, c.thr, c.ow, c.dw)
    want = C.oracle_features("256x192", c.maxo, c.thr, c.ow, c.dw)
    assert len(want) == c.features
    H.assert_features_equal(ref["features"], want)


def test_placed_geometry_is_the_oracles():
    s = C.oracle_scale_space("placed")
    for o in range(4):
        g = C.geometry(o)
        w, h, pw, sig = s.octave_info(o)
        assert (g.w, g.h) == (w, h) == (512 >> o, 512 >> o) and g.pw == pw
        assert np.array_equal(H.bits(g.sigma), H.bits(sig))


@pytest.mark.parametrize("name", list(C.SETS))
def test_every_set_meets_the_preconditions(name):
    spec = C.SETS[name]
    dw = C.PAIRS[spec.pair][1]
    lists = C.build_set(name)
    assert len(lists) == 4 and len(lists[3][0]) == 0
    for o, (kps, idx) in enumerate(lists):
        C.check_preconditions(o, dw, kps, idx)
    if spec.kind == "segments":
        sizes = C.SEGMENT_SIZES[name.split("segments_")[1].replace("_min", "")]
        for kps, idx in lists[:3]:
            assert tuple(int((kps["blur"] == b).sum()) for b in (1, 2, 3)) == sizes      # nothing was dropped
            assert len(np.unique(kps["loc"], axis=0)) == max(sizes)                     # the windows differ inside a segment
    if spec.kind == "theta":
        assert len(C.forced_thetas()) == 25
        for kps, idx in lists[:3]:
            for b in (1, 2, 3):
                seg = kps[kps["blur"] == b]
                # the forced thetas on one key point first, the border-touching windows behind them
                assert len(seg) == 0 or np.array_equal(H.bits(seg["theta"][:25]), H.bits(np.array(C.forced_thetas(), f32)))
                assert len(seg) == 0 or len(np.unique(seg["loc"][:25], axis=0)) == 1
        assert sum(len(k) for k, _ in lists) >= 175


@pytest.mark.parametrize("name", list(C.SETS))
def test_what_every_set_reaches(name):
    spec = C.SETS[name]
    ow, dw = C.PAIRS[spec.pair]
    lists, ref = C.build_set(name), C.reference(name)
    feats = ref["features"]
    assert len(feats) == sum(len(e) for e in ref["expanded"]) > 0
    assert feats["values"].any(1).all(), "a reference descriptor without votes (0 / 0: undefined bytes)"
    norient = np.concatenate(ref["norient"])
    widest_o = max(int(C.ori_half(k["sigma"], ow, C.geometry(o).pw).max()) for o, (k, _) in enumerate(lists[:3]) if len(k))
    widest_d = max(int(C.desc_half(k["sigma"], dw, C.geometry(o).pw).max()) for o, (k, _) in enumerate(lists[:3]) if len(k))
    # the coordinates the descriptor windows reach (only key points close enough to a border can leave the level)
    low = high = 0
    for o, exp in enumerate(ref["expanded"]):
        g = C.geometry(o)
        for kp in exp:
            wc = C.desc_half(kp["sigma"], dw, g.pw)
            x, y = kp["loc"]
            if min(x, y) - wc > -0.5 and max(x, y) + wc < g.w - 0.5:
                continue
            x0, x1, y0, y1 = C.descriptor_window_reach(kp, dw, g.pw)
            assert -1 <= x0 and x1 <= g.w and -1 <= y0 and y1 <= g.h      # what the padded tables are sized for
            low += int(x0 == -1 or y0 == -1)
            high += int(x1 == g.w or y1 == g.h)
    print("%s: key points %s -> %d features; no orientation %d, two or more %d; widest orientation / descriptor half-width %d / %d; "
          "descriptor windows at -1: %d, at W or H: %d" % (name, [len(k) for k, _ in lists], len(feats), int((norient == 0).sum()),
                                                          int((norient >= 2).sum()), widest_o, widest_d, low, high))
    if spec.kind == "theta":       # an oriented list needs no orientation window: the table's padding at every parameter pair
        assert low >= 1 and high >= 1
    if spec.kind != "place":
        return
    for kps, _ in lists[:3]:
        assert len(kps) >= 20
    assert (norient >= 2).any()
    # checkKeyPoints keeps sigma dw / pixelWidth inside the level; the orientation half-width ceil(3 sigma ow / pixelWidth)
    # can only leave it where it is the larger of the two
    if 3.0 * ow <= dw:      # (otherwise a key point that close to the border has no orientation: the theta sets go there)
        assert low >= 1 and high >= 1
    else:
        assert (norient == 0).any()
        inside = np.concatenate([C.has_orientation_window(k["loc"][:, 0], k["loc"][:, 1], k["sigma"], ow, C.geometry(o).pw,
                                                          C.geometry(o).w, C.geometry(o).h) for o, (k, _) in enumerate(lists[:3])])
        assert (~inside).any() and (norient[~inside] == 0).all()
    if spec.pair == "max":
        assert widest_d == 240 and widest_o == 120      # sigma 3.99 in octave 0: 57 840 orbit indices, 241 columns
    # minx == 0.0 exactly somewhere, where the orientation half-width is the margin
    if 3.0 * ow > dw:
        k0 = lists[0][0]
        assert (k0["loc"][:, 0] - C.ori_half(k0["sigma"], ow, C.geometry(0).pw) == 0).any()
