"""The overflow cases, no GPU: tests/overflow_cases.py reaches what it claims.  Everything here is the CPU oracle: the per-octave
counts the capacities were chosen from (a drifting oracle fails here, loudly), where every named capacity falls in its list, that
no capacity is below the plan's floor, which octaves overflow, and the numpy restatement of truncation on small lists."""
import numpy as np
import pytest

import helpers as H
import overflow_cases as V
import sampling_cases as C

# octave 0: [idx0..idx4, n] after stages 0 and 1, n after stages 5 and 6 (maxOrientations 2, threshold 0.8)
MEASURED = {
    "noise256": ([0, 0, 141, 4134, 6471, 6471], [0, 0, 141, 4134, 6459, 6459], 4578, [0, 0, 176, 3348, 6379, 6379]),
    "syn512": ([0, 0, 2663, 7688, 9093, 9093], [0, 0, 234, 3439, 4756, 4756], 4028, [0, 0, 321, 3929, 5413, 5413]),
}
SMALL_OCTAVES_AT_MOST = {"noise256": 586, "syn512": 779}


@pytest.mark.parametrize("name", list(MEASURED))
def test_the_counts_the_capacities_were_chosen_from(name):
    raw, first, checked, expanded = MEASURED[name]
    assert V.counts(name, 0)[0] == raw
    assert V.counts(name, 1)[0] == first
    assert V.counts(name, 5)[0][5] == checked
    assert V.counts(name, 6)[0] == expanded
    small = max(c[5] for st in (0, 1, 5, 6) for c in V.counts(name, st)[1:])
    assert small == SMALL_OCTAVES_AT_MOST[name] < V.FLOOR


def test_syn512_features_per_octave():
    assert [len(f) for f in V.features_per_octave("syn512")] == [5413, 737, 133, 18] and len(V.features("syn512")) == 6301


def test_four_orientations_on_the_noise_image():
    """13598 features; octaves 1-3 give at most 4 x 450 of them, octave 0's expansion 12488: far past its 6459 extrema"""
    lists, feats = V.chain("noise256", V.MAXO4, V.THR4)
    assert [len(l) for l, _ in lists] == [12488, 1049, 59, 2]
    assert [int(v) for v in lists[0][1]] == [0, 0, 366, 6713, 12488]
    H.assert_features_equal(np.concatenate(feats), V.scale_space("noise256").features(V.MAXO4, V.THR4, 1.5, 6.0))
    assert sum(len(f) for f in feats) == 13598 and sum(len(f) for f in feats[1:]) <= 4 * 450
    c = V.EXPANSION_MAXO4
    assert V.counts("noise256", 1)[0][5] <= c.cap, "the extrema fit: the expansion is what overflows"
    assert c.claim <= V.where(lists[0][1], len(lists[0][0]), c.cap)
    for l, idx in lists[1:]:
        assert len(l) <= c.cap


def _octave0(name, stage):
    lst, idx = V.lists(name, stage)[0]
    return idx, len(lst)


@pytest.mark.parametrize("table, stage", [("STAGED_EXTREMA", 0), ("FUSED_EXTREMA", 1), ("EXPANSION", 6)])
def test_every_capacity_falls_where_it_is_claimed_to_fall(table, stage):
    cases = getattr(V, table)
    for c in cases:
        assert c.cap >= V.FLOOR, "the plan's floor would replace it"
        idx, n = _octave0(c.image, stage)
        got = V.where(idx, n, c.cap)
        print("%s %s cap %d: octave 0 has %d, idx %s -> %s" % (table, c.image, c.cap, n, [int(v) for v in idx], sorted(got)))
        assert c.claim <= got, (c, sorted(got))
        also = V.ALSO_OVERFLOWS.get((c.image, c.cap), {}) if table == "STAGED_EXTREMA" else {}
        for o in (1, 2, 3):
            for st in ((stage,) if stage < 6 else (1, 2, 3, 4, 5, 6)):
                lst, oidx = V.lists(c.image, st)[o]
                if o in also:
                    assert also[o] <= V.where(oidx, len(lst), c.cap)
                else:
                    assert len(lst) <= c.cap, (c, o, st)
        if stage == 6:      # the extrema (and every list between) fit: the expansion alone decides
            assert all(V.counts(c.image, st)[0][5] <= c.cap for st in (1, 2, 3, 4, 5))
    labels = set().union(*[c.claim for c in cases])
    if table == "STAGED_EXTREMA":
        assert labels == {"inside blur 1", "inside blur 2", "on the blur 2/3 boundary", "inside blur 3", "one too many", "exact fit"}
        idx, n = _octave0("noise256", 0)
        assert 4135 - int(idx[3]) == 1      # one blur-3 record survives
    else:
        assert {"exact fit", "one too many"} <= labels


def test_the_blur1_cut_candidate():
    """noise 768 x 768 is the first candidate with more than 4096 raw blur-1 extrema in octave 0; its octave 1 overflows too"""
    c = V.counts("noise768", 0)
    assert c[0] == [0, 0, 8567, 11039, 25973, 25973] and c[1] == [0, 0, 2730, 4505, 5184, 5184] and c[2][5] == 498 and c[3][5] == 61
    lst, idx = V.lists("noise768", 0)[0]
    _, st = V.truncate_extrema(lst, idx, 4096)
    assert st.tolist() == [0, 0, 4096, 4096, 4096, 4096, 1, 1]
    assert V.mask_of([V.truncate_extrema(l, i, 4096)[1] for l, i in V.lists("noise768", 0)]) == 0b0011


def test_the_image_that_fits():
    """under 4096 in every octave after every stage, raw list included, and not empty in any octave"""
    for st in range(7):
        c = V.counts(V.FITS, st)
        assert all(0 < o[5] < V.FLOOR for o in c), (st, c)
    assert V.counts(V.FITS, 0)[0][5] == 2716 and len(V.features(V.FITS)) == 568
    assert V.capacity_fits(V.FITS, 4096)


def test_the_re_run_loop_takes_the_steps_it_is_there_for():
    """syn512 from 4096: one re-run; the 512 x 512 noise image: two (13620 first-list records, 16211 after the expansion)"""
    assert V.counts("noise512", 1)[0] == [0, 0, 2332, 11719, 13620, 13620] and V.counts("noise512", 6)[0][5] == 16211
    for name, caps, nfeat in V.RERUNS:
        assert len(V.features(name)) == nfeat
        assert [V.capacity_fits(name, cap) for cap in caps] == [False] * (len(caps) - 1) + [True], name
        assert all(b == 2 * a for a, b in zip(caps, caps[1:])) and caps[0] == V.FLOOR


# ---- truncation restated, on lists small enough to read -----------------------------------------------------------------------------
def _list(blurs):
    kp = np.zeros(len(blurs), H.SSKEYPOINT)
    kp["blur"], kp["loc"][:, 0] = blurs, np.arange(len(blurs))
    return kp, C.partition_by_blur(kp)


def test_truncation_restated():
    lst, idx = _list([1, 1, 1, 2, 2, 3, 3, 3])
    assert idx.tolist() == [0, 0, 3, 5, 8]
    for cap, want in ((8, [0, 0, 3, 5, 8, 8, 1, 0]), (9, [0, 0, 3, 5, 8, 8, 1, 0]), (7, [0, 0, 3, 5, 7, 7, 1, 1]),
                      (5, [0, 0, 3, 5, 5, 5, 1, 1]), (4, [0, 0, 3, 4, 4, 4, 1, 1]), (2, [0, 0, 2, 2, 2, 2, 1, 1])):
        for fn in (V.truncate_extrema, V.truncate_expanded):
            got, st = fn(lst, idx, cap)
            assert st.tolist() == want, (fn.__name__, cap, st)
            assert np.array_equal(got["loc"][:, 0], np.arange(min(cap, 8)))
    empty, eidx = _list([])
    assert V.truncate_extrema(empty, eidx, 4)[1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    assert V.where(idx, 8, 8) == {"fits", "exact fit"} and V.where(idx, 8, 9) == {"fits"}
    assert V.where(idx, 8, 7) == {"inside blur 3", "one too many"} and V.where(idx, 8, 5) == {"on the blur 2/3 boundary"}
    assert V.where(idx, 8, 4) == {"inside blur 2"} and V.where(idx, 8, 3) == {"on the blur 1/2 boundary"} and V.where(idx, 8, 1) == {"inside blur 1"}
    f = [np.arange(5), np.arange(10, 13), np.arange(20, 20), np.arange(30, 32)]
    assert V.truncated_features(f, [2, 3, 0, 1]).tolist() == [0, 1, 10, 11, 12, 30]


# ---- the hand-placed lists whose expansion overflows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.PLACED_CUTS))
def test_hand_placed_expansion_overflow(name):
    """preconditions of every injected list; where 4096 falls in octave 0's expansion"""
    lists = V.placed_lists(name)
    _, dw = C.PAIRS[V.PLACED_PAIR]
    for o, (kps, idx) in enumerate(lists):
        C.check_preconditions(o, dw, kps, idx)
    (exp, feats, norient) = V.placed_reference(name)
    kps0, idx0 = lists[0]
    e0, eidx0 = exp[0]
    cap = C.CAPACITY
    assert len(kps0) <= cap < len(e0) and (norient >= 2).all() and norient.sum() == len(e0)
    assert 0 < len(lists[1][0]) and 0 < len(exp[1][0]) <= cap and len(lists[2][0]) == len(lists[3][0]) == 0
    assert np.array_equal(eidx0, [0, 0] + [int(norient[:idx0[b]].sum()) for b in (2, 3)] + [len(e0)])
    starts = np.concatenate([[0], np.cumsum(norient)])       # first expanded record of every key point (and the end)
    print(name, "octave 0:", len(kps0), "key points", idx0.tolist(), "->", len(e0), "records", eidx0.tolist())
    _, st = V.truncate_expanded(e0, eidx0, cap)
    if name == "mid_keypoint":
        k = int(np.searchsorted(starts, cap, side="right")) - 1      # the key point that holds record `cap`
        assert starts[k] == cap - 1 and norient[k] >= 2 and kps0["blur"][k] == 2, "cut behind its first orientation"
        assert st.tolist() == [0, 0, 1000, cap, cap, cap, 1, 1] and eidx0[3] > cap
    elif name == "segment_start":
        assert cap in starts and eidx0[3] == cap and eidx0[4] > cap, "blur 3 starts on the cut: no clamp needed, nothing of it kept"
        assert st.tolist() == [0, 0, 1000, cap, cap, cap, 1, 1]
    else:
        assert eidx0[2] > cap and eidx0[2] < eidx0[3] < eidx0[4]
        assert st.tolist() == [0, 0, cap, cap, cap, cap, 1, 1]
    assert len(feats[0]) == len(e0) and len(feats[1]) == len(exp[1][0])
