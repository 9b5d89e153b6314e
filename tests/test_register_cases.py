"""The surface-registration cases test something: proved on the numpy restatement alone (tests/register_ref.py), without a GPU.
tests/test_gpu_register.py holds csrc/register.hip to the same reference on the same cases."""
import numpy as np

import accuracy_ref as A
import dsm_ref as D
import register_cases as C
import register_ref as R


def test_every_triangle_kind_occurs_and_the_gates_bite():
    seen = set()
    for name in sorted(C.TERMS):
        rows, rec = C.rows_reference(name), C.terms_reference(name)
        seen |= set(np.unique(rows["kind"][rows["inside"]]).tolist())
        assert int(rec["n"]) == len(C.TERMS[name].points) and int(rec["reserved"]) == 0
        assert int(rec["inside"]) == int(rows["inside"].sum()) and int(rec["used"]) == int(rows["used"].sum())
        if name.endswith("/gated") or name in ("relief_uncut", "n255", "n257", "n4095", "n4096", "n4097", "n8193"):
            assert 0 < int(rec["used"]) < int(rec["inside"]) < int(rec["n"]), name
    assert seen == {0, 1, 2, 3}
    for name in ("relief/rigid", "n8193", "skew_frame"):     # every kind inside one case, too
        rows = C.rows_reference(name)
        assert set(np.unique(rows["kind"][rows["inside"]]).tolist()) == {0, 1, 2, 3}, name
    assert set(np.unique(C.rows_reference("grid_2x2")["kind"]).tolist()) != set(np.unique(C.rows_reference("signed_zeros")["kind"]).tolist())


def test_the_edge_cases_are_what_they_claim():
    rec = C.terms_reference("grid_1x5")                      # a side below 2: nothing is inside, every sum is +0.0
    assert int(rec["n"]) > 0 and int(rec["inside"]) == 0 and int(rec["used"]) == 0
    assert rec.tobytes()[16:] == bytes(288)
    assert C.terms_reference("n0").tobytes() == bytes(304)
    rows = C.rows_reference("skew_frame")                    # an affine frame: the gradient has x and y parts
    G = rows["G"][rows["inside"]]
    assert (G[:, 0] != 0).all() and (G[:, 1] != 0).all()
    half = C.terms_reference("relief/half_off")              # the pose throws about half the cloud off the grid
    assert 0.3 < int(half["inside"]) / int(C.terms_reference("relief/identity")["inside"]) < 0.7
    assert int(C.terms_reference("special_heights")["inside"]) != int(C.terms_reference("relief/identity")["inside"])   # +inf and the NaN take cells away
    rows = C.rows_reference("overflowing_slopes")            # a difference exists, the slope over the cell overflows: not used
    assert rows["inside"].sum() > 100 and not rows["used"].any() and not np.isfinite(rows["J"][rows["inside"]]).all(1).any()
    assert C.terms_reference("overflowing_slopes").tobytes()[16:] == bytes(288)
    zeros = C.rows_reference("signed_zeros")
    assert (zeros["d"][zeros["inside"]] == 0).sum() > 20 and zeros["used"][zeros["inside"]].all()   # d = 0 is a difference like any other
    rigid = np.asarray(C.RIGID["m"], np.float64).reshape(3, 4)[:, :3]
    assert np.allclose(rigid @ rigid.T, np.eye(3), atol=1e-6) and not np.allclose(rigid, np.eye(3), atol=1e-3)
    sim = np.asarray(C.SIMILARITY["m"], np.float64).reshape(3, 4)[:, :3]
    assert np.allclose(sim @ sim.T, 1.03 ** 2 * np.eye(3), atol=1e-5)


def test_the_sums_are_the_shaped_sums_of_exact_products():
    name = "n8193"
    rows, rec = C.rows_reference(name), C.terms_reference(name)
    J, e = np.where(rows["used"][:, None], rows["J"], 0).astype(np.float64), np.where(rows["used"], rows["e"], 0).astype(np.float64)
    for k, (i, j) in enumerate(R.PAIRS):
        assert rec["jtj"][k] == A.shaped_sum(J[:, i] * J[:, j])
    assert rec["jte"][6] == A.shaped_sum(J[:, 6] * e) and rec["ee"] == A.shaped_sum(e * e)
    prod = J[:, 3] * J[:, 5]                                   # exact: a float32 product fits float64's 53 bits
    assert all(float(np.float32(a)) * float(np.float32(b)) == c for a, b, c in zip(rows["J"][:50, 3], rows["J"][:50, 5], prod[:50]) if c)


def test_the_big_case_has_three_live_tiles_and_needs_a_second_level():
    c = C.big_case()
    assert len(c.points) == 4096 * 4096 + 5 == C.BIG_N
    live = np.unique(np.nonzero(~R.skipped(c.points))[0] // 4096)
    assert live.tolist() == list(C.BIG_TILES) and (4096 * 4096 + 5 + 4095) // 4096 == 4097 > 4096
    rec = C.terms_reference("big")
    assert int(rec["n"]) == C.BIG_N and 0 < int(rec["used"]) < int(rec["inside"]) <= 2 * 4096 + 5 and rec["ee"] > 0


def test_the_transform_copies_what_the_skip_rule_skips():
    pts, g = C.TRANSFORM["specials"]
    out = R.transform(pts, g)
    skip = R.skipped(pts)
    assert skip.sum() >= 10 and (~skip).sum() >= 6
    assert np.array_equal(D.bits(out)[skip], D.bits(pts)[skip]) and (D.bits(out)[~skip] != D.bits(pts)[~skip]).any(1).all()
    assert np.array_equal(D.bits(R.transform(pts, C.IDENTITY))[~skip], D.bits(pts + np.float32(0))[~skip])


def test_the_reference_registers_the_displaced_scene():
    """the motion is 0.8, -0.6, 0.5 cells, 0.004, -0.003, 0.006 rad and for "similarity" a scale of 1.01: the cloud starts more
    than 1 cell RMS from its true points and lies within 0.1 cell of them after at most 6 iterations"""
    for dof in ("rigid", "similarity"):
        res, before, after = C.scene_reference(dof, None, False)
        print("%s: %.3f -> %.4f cells in %d iterations" % (dof, before, after, len(res["history"])))
        assert before > 1.0 and after < 0.1 and len(res["history"]) <= 6
        assert res["history"][-1]["rms"] < 0.3 * res["history"][0]["rms"]


def test_the_reference_needs_the_gate_against_outliers():
    """every tenth point raised 20 cells along ez: without a gate the loop ends more than a cell off, with gate 3 within 0.1"""
    free, _, off = C.scene_reference("rigid", None, True)
    gated, before, after = C.scene_reference("rigid", 3.0, True)
    print("outliers: without a gate %.3f cells, with %.4f" % (off, after))
    assert before > 1.0 and off > 1.0 and after < 0.1
    assert all(h["used"] < h["inside"] for h in gated["history"]) and all(h["used"] == h["inside"] for h in free["history"])
