"""The numpy restatement of the terrain filter (tests/terrain_ref.py) held to a plain double loop over the clipped 2-D window
that selects by key, to the properties include/ssrlcv_hip.h "terrain filter" states, and to what the contract implies on the
boxed scene map of tests/terrain_cases.py.  No GPU."""
import numpy as np
import pytest

import terrain_cases as C
import terrain_ref as R

SMALL_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 4), (13, 9), (24, 20))
SMALL_RADII = (1, 2, 3, 7, 30, C.UINT32_MAX)
SMALL_CONTENTS = ("hard", "holes5", "holes60", "noise", "single", "all_invalid", "constant")


def plain_key(b):
    b = int(b)
    b = b - (1 << 32) if b >= 1 << 31 else b
    return b if b >= 0 else b ^ 0x7FFFFFFF


def plain_select(bits, r, largest):
    """for every cell: the clipped window, its valid cells, the one with the smallest (largest) key"""
    h, w = bits.shape
    out = np.full((h, w), R.INVALID, np.uint32)
    for y in range(h):
        for x in range(w):
            window = bits[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].ravel()
            values = [int(b) for b in window if b != R.INVALID]
            if values:
                out[y, x] = max(values, key=plain_key) if largest else min(values, key=plain_key)
    return out


def plain_morphology(bits, radius, op):
    h, w = bits.shape
    r = min(radius, max(w, h) - 1)
    if op == R.ERODE:
        return plain_select(bits, r, False)
    if op == R.DILATE:
        return plain_select(bits, r, True)
    out = plain_select(plain_select(bits, r, op == R.CLOSE), r, op == R.OPEN)
    out[bits == R.INVALID] = R.INVALID
    return out


@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_restatement_equals_the_plain_loop(size):
    w, h = size
    for name in SMALL_CONTENTS:
        bits = R.bits_of(C.CONTENTS[name](w, h))
        for radius in SMALL_RADII:
            if min(radius, max(w, h) - 1) in {min(r, max(w, h) - 1) for r in SMALL_RADII if r < radius}:
                continue                                              # the same effective radius as a smaller one
            for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
                want, got = plain_morphology(bits, radius, op), R.morphology_bits(bits, radius, op)
                assert np.array_equal(got, want), (name, radius, op, np.argwhere(got != want)[:3])


def test_the_key_is_a_total_order_on_bit_patterns():
    bits = np.concatenate([C.HARD_BITS, np.array([1, 0x80000001, 0x7FC00001, 0x3F800000, 0xBF800000], np.uint32)])
    k = R.keys(bits)
    assert len(set(k.tolist())) == len(set(bits.tolist()))            # equal keys are equal bits
    assert np.array_equal(R.bits_from_keys(k), bits)
    as_key = {int(b): int(v) for b, v in zip(bits, k)}
    assert as_key[0x80000000] < as_key[0x00000000]                    # -0 < +0
    assert as_key[0xFFFFFFFF] < as_key[0xFF800000] < as_key[0xFF7FFFFF] < as_key[0x7F7FFFFF] < as_key[0x7F800000] < as_key[0x7FFFFFFF]
    assert as_key[0x7FBFFFFF] < as_key[R.INVALID] < as_key[0x7FC00001]   # the invalid pattern's key lies between two valid ones


def test_the_properties_the_header_states():
    for w, h in ((24, 20), (13, 9), (1, 7)):
        for name in ("hard", "holes5", "holes60", "noise"):
            bits = R.bits_of(C.CONTENTS[name](w, h))
            valid = bits != R.INVALID
            k = R.keys(bits)
            for radius in (1, 3, 30):
                opened, closed = R.morphology_bits(bits, radius, R.OPEN), R.morphology_bits(bits, radius, R.CLOSE)
                assert np.array_equal(opened != R.INVALID, valid) and np.array_equal(closed != R.INVALID, valid)
                assert (R.keys(opened)[valid] <= k[valid]).all() and (R.keys(closed)[valid] >= k[valid]).all()
                for out in (opened, closed, R.morphology_bits(bits, radius, R.ERODE), R.morphology_bits(bits, radius, R.DILATE)):
                    assert np.isin(out, np.append(bits.ravel(), np.uint32(R.INVALID))).all()     # input bits or the invalid pattern
            for radius in (max(w, h) - 1, max(w, h), C.UINT32_MAX):
                if radius < 1:
                    continue
                lowest = bits[valid][np.argmin(k[valid])]
                assert (R.morphology_bits(bits, radius, R.ERODE) == lowest).all()                # the global minimum everywhere
                assert (R.morphology_bits(bits, radius, R.DILATE) == bits[valid][np.argmax(k[valid])]).all()
    nothing = R.bits_of(C.all_invalid(5, 4))
    for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
        assert (R.morphology_bits(nothing, 2, op) == R.INVALID).all()


def test_a_plateau_that_holds_the_largest_window_is_ground():
    radii, thresholds = (1, 2, 4), (0.0, 0.0, 0.0)
    for side, flagged in ((2 * radii[-1] + 1, False), (2 * radii[-1], True)):
        height = np.zeros((30, 31), np.float32)
        height[8:8 + side, 9:9 + side] = 3.0
        level = R.terrain(height, radii, thresholds)["level"]
        assert ((level[8:8 + side, 9:9 + side] != 0).all() if flagged else (level == 0).all()), side
        assert (level[height == 0] == 0).all()


def test_the_interior_of_an_exact_plane_is_never_flagged_and_the_header_s_count():
    radii = (1, 2, 4, 8)
    jj, ii = np.mgrid[0:70, 0:80]
    plane = (0.3 * ii - 0.2 * jj + 1).astype(np.float32)
    level = R.terrain(plane, radii, (0.0,) * 4)["level"]
    border = np.minimum(np.minimum(ii, 79 - ii), np.minimum(jj, 69 - jj))           # cells between a cell and the nearest border
    assert (level[border >= 2 * sum(radii)] == 0).all()
    flagged = level != 0
    print("plane 80 x 70, radii 1 2 4 8, thresholds 0: %d cells flagged, the deepest %d cells from a border" % (int(flagged.sum()), int(border[flagged].max())))
    assert int(flagged.sum()) == 1136 and int(border[flagged].max()) <= 7           # the header's "border" paragraph


def test_terrain_outputs_agree_with_each_other():
    for name in ("hard", "holes60", "noise"):
        height = C.CONTENTS[name](24, 20)
        for radii, thresholds in C.TERRAIN_PARAMS:
            out = R.terrain(height, radii, thresholds)
            bits, level = R.bits_of(height), out["level"]
            assert np.array_equal(level == R.NO_CELL, bits == R.INVALID)
            assert np.array_equal(R.bits_of(out["terrain"]), np.where(level == 0, bits, np.uint32(R.INVALID)))
            assert level[level != R.NO_CELL].max(initial=0) <= len(radii)
            assert np.array_equal(R.bits_of(out["opened"]) != R.INVALID, bits != R.INVALID)


def test_subtract():
    a, b = C.subtract_pair(24, 20)
    out = R.bits_of(R.subtract(a, b))
    ua, ub = R.bits_of(a), R.bits_of(b)
    both = (ua != R.INVALID) & (ub != R.INVALID)
    assert (out[~both] == R.INVALID).all()
    inf_inf = both & (ua == 0x7F800000) & (ub == 0x7F800000)
    assert inf_inf.any() and (out[inf_inf] == R.INVALID).all()                      # inf - inf does not reach the map
    assert out[0, 2] == 0x7F800000 and out[0, 3] == R.INVALID                       # inf - -inf is inf; a NaN operand gives a NaN
    assert not np.isnan(out.view(np.float32)[out != R.INVALID]).any()
    x = np.array([[1.5, -2.0]], np.float32)
    assert np.array_equal(R.subtract(x, np.array([[0.25, 3.0]], np.float32)), np.array([[1.25, -5.0]], np.float32))


def scene_counts(height, s, radii, thresholds):
    level = R.terrain(height, radii, thresholds)["level"]
    valid = R.bits_of(height) != R.INVALID
    flagged = (level != 0) & valid
    return {"boxes": int((s["box"] & valid).sum()), "boxes_flagged": int((flagged & s["box"]).sum()), "ground_flagged": int((flagged & s["ground"]).sum()),
            "plateau_flagged": int((flagged & s["plateau"]).sum())}


def test_the_boxed_scene():
    """what follows from the contract: every box cell is flagged (a window wider than the box holds a ground cell, so the opening
    there is at most the relief, and 2 - 0.3 > 1.5); no ground cell is (an opening never goes below the global minimum, so
    d <= relief < 0.5); no plateau cell is"""
    s = C.scene()
    radii, thresholds = R.schedule(**C.SCHEDULE)
    assert tuple(radii) == C.SCENE_RADII and [float(t) for t in thresholds] == [float(np.float32(t)) for t in (0.5, 1.1, 1.5, 1.5)]
    got = scene_counts(s["height"], s, radii, thresholds)
    print("boxed scene %d x %d, relief %.3f: %d of %d box cells flagged, %d ground cells, %d plateau cells"
          % (s["height"].shape[1], s["height"].shape[0], float(s["height"][s["ground"]].max() - s["height"][s["ground"]].min()), got["boxes_flagged"],
             got["boxes"], got["ground_flagged"], got["plateau_flagged"]))
    assert got["boxes"] == sum(b[2] ** 2 for b in C.BOXES)
    assert got["boxes_flagged"] == got["boxes"] and got["ground_flagged"] == 0 and got["plateau_flagged"] == 0
    # with a tenth of the cells invalid a window may hold no valid ground: nothing is derivable, the reference's own result is kept
    holed = scene_counts(C.with_holes(s["height"]), s, radii, thresholds)
    print("with 10 %% of the cells invalid: %d of %d box cells flagged, %d ground cells, %d plateau cells"
          % (holed["boxes_flagged"], holed["boxes"], holed["ground_flagged"], holed["plateau_flagged"]))
    assert holed["boxes_flagged"] == holed["boxes"] and holed["ground_flagged"] == 0 and holed["plateau_flagged"] == 0
