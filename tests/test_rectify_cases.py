"""Without a GPU, on the numpy reference alone (tests/rectify_ref.py): the warp's invariants, that the cases of
tests/rectify_cases.py test something, and the whole chain on the scene pair -- rectify, SAD disparities, mask -- against the
scene's ground truth.  tests/test_gpu_rectify.py holds the kernels to this reference bit for bit, so the floors asserted here
carry over to the GPU with no tolerance of their own."""
import numpy as np

import helpers as H
import rectify_cases as C
import rectify_ref as R

f32 = np.float32


def image(w, h, seed=3):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)


def test_the_identity_warp_is_a_copy():
    src = image(67, 45)
    assert np.array_equal(R.warp_ref(src, C.IDENTITY, 67, 45), src)


def test_an_integer_translation_is_a_shifted_copy_with_replicated_border():
    src = image(67, 45)
    out = R.warp_ref(src, C.homography("shift_int", 67), 67, 45)   # sx = x + 3, sy = y - 2
    xs = np.clip(np.arange(67) + 3, 0, 66)
    ys = np.clip(np.arange(45) - 2, 0, 44)
    assert np.array_equal(out, src[ys[:, None], xs[None, :]])
    assert np.array_equal(out[:2], np.repeat(out[2:3], 2, 0)) and np.array_equal(out[:, 64:], np.repeat(out[:, 63:64], 3, 1))


def test_a_quarter_turn_is_rot90_exactly():
    src = image(67, 45)
    out = R.warp_ref(src, C.quarter_turn(45), 45, 67)   # sx = y, sy = 44 - x
    assert out.shape == (67, 45) and np.array_equal(out, np.rot90(src, -1))
    sq = image(31, 31, 4)
    assert np.array_equal(R.warp_ref(sq, C.quarter_turn(31), 31, 31), np.rot90(sq, -1))


def test_a_half_pixel_shift_of_a_two_valued_image_gives_the_rounded_means():
    src = np.where(np.random.RandomState(9).rand(20, 30) < 0.5, 10, 201).astype(np.uint8)
    out = R.warp_ref(src, [1, 0, 0.5, 0, 1, 0, 0, 0, 1], 30, 20)   # between columns x and x + 1
    a, b = src[:, :-1].astype(np.int64), src[:, 1:].astype(np.int64)
    assert np.array_equal(out[:, :-1], (a + b + 1) // 2)           # (10 + 201) / 2 = 105.5 rounds up to 106
    assert set(np.unique(out)) == {10, 106, 201}
    assert np.array_equal(out[:, -1], src[:, -1])                  # the last column replicates


def test_the_evaluation_is_float32_and_says_what_is_mapped():
    sx, sy, mapped = R.eval_h(C.homography("w_zero", 5), np.array([4, 0, 6], f32), np.array([0, 0, 1], f32))
    assert mapped.tolist() == [False, True, False] and sx.dtype == np.float32
    assert R.inside(C.IDENTITY, f32(66), f32(44), 67, 45) and not R.inside(C.IDENTITY, f32(66.00001), f32(44), 67, 45)
    assert not R.eval_h(C.homography("nan_w", 5), f32(1), f32(1))[2] and not R.eval_h(C.homography("all_behind", 5), f32(1), f32(1))[2]


def test_the_warp_cases_cover_what_the_kernel_can_get_wrong():
    names = set(C.WARP_CASES)
    widths = {c.dw for c in C.WARP_CASES.values()}
    assert set(C.WIDTHS) <= widths and {c.dh for c in C.WARP_CASES.values()} >= set(C.HEIGHTS)
    assert {c.source for c in C.WARP_CASES.values()} == set(C.SOURCES)
    assert {c.hom for c in C.WARP_CASES.values()} == set(C.HOMOGRAPHIES) | {"quarter_turn"}
    ref = {n: C.warp_reference(n) for n in names}
    # exactly on the last column: x = 64 reads column 66 itself, the pixels behind it replicate it
    src, _, out = ref["67x45/last_column/257x3"]
    assert np.array_equal(out[:, 64], src[:3, 66]) and (out[:, 65:] == src[:3, 66:67]).all() and np.array_equal(out[:, :64], src[:3, 2:66])
    # W changes sign inside the output: pixels on both sides, the far side zero
    src, Hm, out = ref["67x45/w_changes_sign/257x1"]
    _, _, mapped = R.eval_h(Hm, np.arange(257, dtype=f32), np.zeros(257, f32))
    assert mapped[:19].all() and not mapped[21:].any() and (out[0, 21:] == 0).all() and out[0, :19].any()
    src, Hm, out = ref["67x45/w_zero/65x3"]
    assert not R.eval_h(Hm, f32(4), f32(0))[2] and out[0, 4] == 0 and out[0, 3] != 0
    # everything outside: the clamped corner; everything behind: zero
    src, _, out = ref["67x45/all_outside/65x3"]
    assert (out == src[0, 66]).all()
    assert not ref["67x45/all_behind/65x3"][2].any() and not ref["67x45/nan_w/65x3"][2].any() and not ref["67x45/nan_entry/65x3"][2][:, 1:].all()
    # 1e30: finite while 1e30 x is, and overflowing behind that
    src, Hm, out = ref["67x45/1e30_entry/257x3"]
    assert (out[:, 1:] == src[:3, 66:67]).all()
    sx, _, mapped = R.eval_h(C.homography("1e30_squared", 5), np.arange(3, dtype=f32), np.zeros(3, f32))
    assert mapped.tolist() == [True, False, False] and np.isinf(sx[1])
    # the rig's homographies move every pixel by a fraction: no case of theirs is a copy
    src, _, out = ref["67x45/rig_Hl/65x3"]
    assert not np.array_equal(out, src[:3, :65])
    # the small sources interpolate along the one axis they have
    assert len(np.unique(ref["1x1/scale_4.1/5x3"][2])) == 1
    src, Hm, out = ref["67x45/zoom_out/2049x1025"]
    assert (2049 + 3) // 4 + 1 == 514 and 514 * 1025 > 2048 * 256 and len(np.unique(out[-4:])) > 50   # the last rows carry content
    assert len(np.unique(ref["7x1/scale_0.37/5x3"][2])) > 1 and len(np.unique(ref["1x7/scale_0.37/5x3"][2])) > 1


def test_the_mask_s_hand_made_map_has_every_kind_of_pixel():
    disp, cost = C.mask_map()
    out, out_cost = R.mask_ref(disp, cost, C.MASK_R, C.MASK_HL, C.MASK_HR, *C.MASK_SRC)
    before, after = H.bits(disp) != R.NAN_BITS, H.bits(out) != R.NAN_BITS
    assert (~before).sum() > 100 and after.sum() > 100 and (before & ~after).sum() > 100 and not (after & ~before).any()   # never rescues
    assert after[10, 4:36].all() and after[12, 4:36].all() and not after[11, 4:36].any()   # on the last column, inside it, past it
    assert np.array_equal(H.bits(out)[after], H.bits(disp)[after])
    assert (out_cost[~after] == R.NO_COST).all() and np.array_equal(out_cost[after], cost[after])
    assert R.mask_ref(disp, None, C.MASK_R, C.MASK_HL, C.MASK_HR, *C.MASK_SRC)[1] is None
    big, Hl, Hr, src = C.big_mask_map()
    kept = H.bits(R.mask_ref(big, None, 3, Hl, Hr, *src)[0]) != R.NAN_BITS
    assert big.size > 2048 * 256 and 100000 < kept.sum() < (H.bits(big) != R.NAN_BITS).sum() - 10000
    assert kept[-8:].any() and not kept[-8:].all()   # the rows a second turn of the loop handles hold both kinds
    assert not after[:, 37:].any() and not after[:2].any()   # the left window leaves its source there


def test_the_apply_records_have_every_kind():
    m = C.apply_records()
    out = R.apply_ref(m, C.APPLY_H0, C.APPLY_H1)
    was, now = m["invalid"] != 0, out["invalid"] != 0
    assert was.sum() > 20 and (now & ~was).sum() > 20 and (~now).sum() > 50 and now[5] and not was[5]
    raw_in, raw_out = m.view(np.uint8).reshape(-1, 40), out.view(np.uint8).reshape(-1, 40)
    assert np.array_equal(raw_in[was], raw_out[was])                        # an invalid record is not touched
    assert np.array_equal(raw_in[now & ~was][:, 1:], raw_out[now & ~was][:, 1:]) and (raw_out[now & ~was][:, 0] == 1).all()
    pad = [i for i in range(40) if i not in (0,) + tuple(range(8, 12)) + tuple(range(16, 28)) + tuple(range(32, 40))]
    assert (raw_out[:, pad] == 0xA5).all() and (out["kp0_parent"] == 4).all() and (out["kp1_parent"] == 9).all()
    moved = ~now
    assert not np.array_equal(out["kp0_loc"][moved], m["kp0_loc"][moved])
    one = R.apply_ref(m, None, C.APPLY_H1)                                   # a NULL side stays
    assert np.array_equal(one["kp0_loc"], m["kp0_loc"]) and not np.array_equal(one["kp1_loc"][moved], m["kp1_loc"][moved])


def test_the_chain_on_the_scene_pair_finds_the_ground_truth():
    c, t, ref = C.CHAIN, C.truth(), C.chain_reference()
    lo, hi = t["true_range"]
    print("true disparities %.2f ... %.2f, searched %d ... %d" % (lo, hi, t["dmin"], t["dmin"] + t["D"] - 1))
    assert t["dmin"] == int(np.floor(lo)) - 2 and t["dmin"] + t["D"] - 1 == int(np.ceil(hi)) + 2
    before = ref["stereo"]["valid"]
    valid = H.bits(ref["disparity"]) != R.NAN_BITS
    err = np.abs(ref["disparity"][valid].astype(np.float64) - t["disparity"][valid])
    within = float((err <= 0.5).mean())
    print("valid %d of %d, the mask removed %d, within 0.5 px %.2f %%, largest error %.3f px" % (
        valid.sum(), valid.size, before.sum() - valid.sum(), 100 * within, err.max()))
    assert valid.sum() >= c.min_valid
    assert within >= c.min_within_half
    assert err.max() <= c.max_error
    assert before.sum() > valid.sum() and not (valid & ~before).any()     # the mask removes something and rescues nothing
    assert (ref["cost"][~valid] == R.NO_COST).all()
    # what the mask removed had a window over replicated border: its source box is not inside
    removed = before & ~valid
    ys, xs = np.nonzero(removed)
    assert ((xs < 16) | (xs > c.size - 17) | (ys < 16) | (ys > c.size - 17)).all()
