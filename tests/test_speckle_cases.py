"""The disparity post-filter cases bite: proven here on the numpy reference alone (tests/speckle_ref.py), without a GPU.  Each
named case of tests/speckle_cases.py has the components its construction says -- the sizes in closed form, never taken from
the reference --, the filter splits at exactly the stated size, the noisy real map has speckles to remove beside a surface that
stays, and the median cases hold every valid count.  tests/test_gpu_speckle.py then holds the kernels to this reference."""
import numpy as np
import pytest

import speckle_cases as S
import speckle_ref as R

CLOSED_FORM = [n for n in S.CASES if S.CASES[n].sizes is not None]


def component_sizes(labels, sizes):
    """one size per component, read at the pixel that carries its own raster index as label"""
    flat = labels.ravel()
    roots = np.flatnonzero(flat == np.arange(flat.size, dtype=np.uint32))
    return sorted(int(s) for s in sizes.ravel()[roots])


@pytest.mark.parametrize("name", CLOSED_FORM)
def test_components_are_what_the_construction_says(name):
    k = S.CASES[name]
    h, w = k.d.shape
    assert w <= 200 and h <= 200 and w * h <= 200 * 100
    ref = S.reference(name)
    labels, sizes = ref["labels"], ref["sizes"]
    assert component_sizes(labels, sizes) == k.sizes
    valid = R.valid_mask(k.d)
    assert int(valid.sum()) == sum(k.sizes)
    assert (labels[~valid] == R.NO_LABEL).all() and (sizes[~valid] == 0).all()
    # a label is the smallest raster index of its component, and a size the number of pixels that carry the label
    idx = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    assert (labels[valid] <= idx[valid]).all()
    for lab in np.unique(labels[valid])[:50]:
        members = labels == lab
        assert idx[members].min() == lab and (sizes[members] == members.sum()).all()


def test_the_cases_cross_the_seams_they_name():
    tw, th = S.TILE_W, S.TILE_H
    for name in ("constant", "checker_holes", "serpentine", "comb_bottom", "spirals", "blobs"):
        h, w = S.CASES[name].d.shape
        assert w > tw and h > th and (w % tw or h % th), name              # more than one tile each way, no multiple of it
    assert S.CASES["serpentine"].sizes == [34 * 200 + 33] and S.CASES["serpentine_t"].d.shape == (150, 67)
    assert S.CASES["column"].d.shape[1] == 1 and S.CASES["row"].d.shape[0] == 1 and S.CASES["one_pixel"].d.shape == (1, 1)
    # the comb's join is in the last row; its label, index 0, is the top of the first tooth
    comb = S.CASES["comb_bottom"].d
    assert not R.valid_mask(comb[:-1, 1::2]).any() and R.valid_mask(comb[-1]).all()
    assert (S.reference("comb_bottom")["labels"][R.valid_mask(comb)] == 0).all()
    top = S.CASES["comb_top"].d
    assert R.valid_mask(top[0]).all() and not R.valid_mask(top[1:, 1::2]).any()
    # the two blocks touch at the tile corner only
    d = S.CASES["corner_diagonal"].d
    v = R.valid_mask(d)
    assert v[th - 1, tw - 1] and v[th, tw] and not v[th - 1, tw] and not v[th, tw - 1]
    assert S.reference("corner_diagonal")["labels"][th, tw] == th * 100 + tw
    # the spirals are one pixel wide paths of one disparity: only geometry separates them
    sp = S.CASES["spirals"]
    assert len(np.unique(sp.d[R.valid_mask(sp.d)])) == 1 and len(sp.sizes) == 2 and min(sp.sizes) > 300


def test_the_ramps_split_at_one_ulp():
    ramp, seam, inside = (S.CASES[n] for n in ("ramp", "ramp_step_seam", "ramp_step_inside"))
    assert ramp.max_diff == seam.max_diff == inside.max_diff == 0.5
    steps = np.abs(np.diff(ramp.d[0]))
    assert (steps == np.float32(0.5)).all() and ramp.d[0].max() - ramp.d[0].min() > 40     # far apart, one component
    assert ramp.sizes == [450]
    for k, at in ((seam, 64), (inside, 75)):
        steps = np.abs(np.diff(k.d[0]))
        assert steps[at - 1] == np.nextafter(np.float32(0.5), np.float32(1)) and (np.delete(steps, at - 1) <= np.float32(0.5)).all()
        assert len(k.sizes) == 2
        labels = S.reference("ramp_step_seam" if at == 64 else "ramp_step_inside")["labels"]
        assert (labels[:, :at] == 0).all() and (labels[:, at:] == at).all()
    assert 64 % S.TILE_W == 0 and 75 % S.TILE_W != 0


def test_the_blobs_split_at_exactly_the_stated_size():
    k = S.CASES["blobs"]
    m = S.MAX_SPECKLE
    assert k.max_size == m and k.sizes == sorted(2 * [m - 1, m, m + 1])
    v = R.valid_mask(k.d)
    assert v[:, S.TILE_W - 1].sum() == 3 and v[:, S.TILE_W].sum() == 3 and v[S.TILE_H - 1].sum() == 3 and v[S.TILE_H].sum() == 3   # astride both seams
    out = S.reference("blobs")["speckles"]
    kept = R.valid_mask(out)
    assert int(kept.sum()) == 2 * (m + 1)                       # <=: the blobs of m - 1 and of m pixels go, those of m + 1 stay
    assert (S.reference("blobs")["sizes"][kept] == m + 1).all()
    assert R.bits(out)[kept].tolist() == R.bits(k.d)[kept].tolist()


def test_special_values_follow_item_1_as_written():
    z = S.CASES["max_diff_zero"]
    left = z.d[:, :33]
    assert (np.signbit(left).sum() > 100) and (left == 0).all() and z.max_diff == 0.0          # -0 and +0 mixed: one component
    assert z.sizes == [1, 33 * 18 - 1, 33 * 18]
    inf = S.CASES["infinite_diff"]
    assert np.isinf(inf.max_diff) and np.isinf(inf.d[5, 10]) and np.isinf(inf.d[5, 11])
    assert R.bits(inf.d)[7, 30] == 0x7FC00001 and R.valid_mask(inf.d)[7, 30] and not R.valid_mask(inf.d)[9, 40]
    ref = S.reference("infinite_diff")
    assert ref["sizes"][7, 30] == 1 and ref["labels"][7, 30] == 7 * 70 + 30                    # a NaN links to nothing
    assert ref["labels"][5, 10] == ref["labels"][5, 11] == 0                                    # joined through finite neighbours
    alone = S.reference("infinities_alone")
    assert alone["labels"][5, 63] != alone["labels"][5, 64]                                     # inf - inf is a NaN: no link
    assert S.CASES["infinite_values"].sizes == [1, 1, 1, 70 * 20 - 4]


def test_the_noisy_real_map_has_speckles_to_remove_and_a_surface_that_stays():
    k = S.case("noisy_real")
    ref = S.reference("noisy_real")
    sizes = component_sizes(ref["labels"], ref["sizes"])
    removed = [s for s in sizes if s <= k.max_size]
    assert len(removed) >= 3 and max(sizes) > 50 * k.max_size              # whole components go, the largest stays
    out = ref["speckles"]
    was, now = R.valid_mask(k.d), R.valid_mask(out)
    assert int(was.sum()) - int(now.sum()) == sum(removed) > 0
    assert (ref["sizes"][now] > k.max_size).all() and (ref["sizes"][was & ~now] <= k.max_size).all()
    assert int((ref["sizes"] == max(sizes)).sum()) == max(sizes) and now[ref["sizes"] == max(sizes)].all()
    assert (R.bits(out)[now] == R.bits(k.d)[now]).all()                     # nothing else is written
    # the salt matters: the clean pair's map, by the same call, is another one
    import stereo_cases as SC
    assert not np.array_equal(R.bits(SC.reference(S.REAL_BASE)["disparity"]), R.bits(S.noisy_real()[0]))


@pytest.mark.parametrize("name", ["blobs", "checker_holes", "infinite_values", "median_mix", "noisy_real"])
def test_the_speckle_reference_is_idempotent_and_only_removes(name):
    k = S.case(name)
    cost = np.arange(k.d.size, dtype=np.uint32).reshape(k.d.shape)
    once, cost1 = R.speckles_ref(k.d, cost, k.max_diff, k.max_size)
    twice, cost2 = R.speckles_ref(once, cost1, k.max_diff, k.max_size)
    assert np.array_equal(R.bits(once), R.bits(twice)) and np.array_equal(cost1, cost2)
    gone = R.valid_mask(k.d) & ~R.valid_mask(once)
    assert (cost1[gone] == 0xFFFFFFFF).all() and np.array_equal(cost1[~gone], cost[~gone])
    assert np.array_equal(R.bits(once)[~gone], R.bits(k.d)[~gone])
    assert np.array_equal(R.bits(once), R.bits(S.reference(name)["speckles"]))                  # with and without a cost map
    same, _ = R.speckles_ref(k.d, None, k.max_diff, 0)
    assert np.array_equal(R.bits(same), R.bits(k.d))                                            # maxSpeckleSize 0 removes nothing


def valid_counts(d, m):
    v = R.valid_mask(d)
    h, w = v.shape
    p = np.pad(v, m).astype(np.int64)
    return sum(p[j:j + h, i:i + w] for j in range(2 * m + 1) for i in range(2 * m + 1))


def test_the_median_cases_hold_every_valid_count_and_every_border():
    d = S.CASES["median_mix"].d
    v = R.valid_mask(d)
    for m in (1, 2):
        assert sorted(set(valid_counts(d, m)[v].tolist())) == list(range(1, (2 * m + 1) ** 2 + 1))   # both parities of the lower median
    assert v[0, 0] and v[0, -1] and v[-1, 0] and v[-1, -1] and v[0].sum() > 5 and v[-1].sum() > 5 and v[:, 0].sum() > 0 and v[:, -1].sum() > 5
    b = R.bits(d)
    assert (b == 0x80000000).any() and (b == 0).any() and np.isposinf(d).any() and np.isneginf(d).any() and (b == 0x7FC00001).any()
    assert d.shape[1] > S.TILE_W and d.shape[0] > S.TILE_H


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("name", ["median_mix", "noisy_real", "checker_holes", "infinite_diff", "max_diff_zero"])
def test_the_median_reference_returns_a_value_of_its_window(name, m):
    d = S.case(name).d
    out = S.reference(name)["median%d" % m]
    v = R.valid_mask(d)
    assert np.array_equal(R.valid_mask(out), v)                 # holes are never filled, valid pixels never lost
    h, w = d.shape
    b, ob = R.bits(d), R.bits(out)
    keys = R.order_key(d)
    for y, x in np.argwhere(v)[::7]:
        win = (slice(max(y - m, 0), min(y + m + 1, h)), slice(max(x - m, 0), min(x + m + 1, w)))
        inside = b[win][v[win]]
        assert ob[y, x] in inside
        ks = np.sort(keys[win][v[win]])
        assert R.order_key(out[y:y + 1, x:x + 1])[0, 0] == ks[(len(ks) - 1) // 2]      # the lower median, by a plain sort


def test_median_edge_cases():
    lonely, hole = S.CASES["lonely"].d, S.CASES["hole"].d
    for m in (1, 2):
        out = S.reference("lonely")["median%d" % m]
        assert np.array_equal(R.bits(out), R.bits(lonely))                         # it keeps its own value
        out = S.reference("hole")["median%d" % m]
        assert R.bits(out)[4, 4] == R.INVALID_BITS and R.valid_mask(out).sum() == 80   # it stays a hole
    # -0 sorts below +0: of {-0, +0} the lower median is -0; of {-0, +0, +0} it is +0
    d = np.full((1, 5), S.INVALID, np.float32)
    d[0, 0], d[0, 1] = 0.0, -0.0
    assert R.bits(R.median_ref(d, 1))[0, :2].tolist() == [0x80000000, 0x80000000]
    d[0, 2] = 0.0
    assert R.bits(R.median_ref(d, 1))[0, 1] == 0 and R.bits(R.median_ref(d, 2))[0, 0] == 0
    # equal values
    assert np.array_equal(R.median_ref(np.full((7, 9), 2.5, np.float32), 2), np.full((7, 9), 2.5, np.float32))
