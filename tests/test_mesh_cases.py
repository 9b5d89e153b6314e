"""The disparity-mesh reference (tests/mesh_ref.py) and cases (tests/mesh_cases.py) on the CPU: the properties that make the
restatement of include/ssrlcv_hip.h "disparity mesh" believable on its own, and the proof that the cases reach what the kernels
of csrc/mesh.hip can get wrong.  No GPU."""
import numpy as np
import pytest

import mesh_cases as C
import mesh_ref as R
import stereo_ref

NAMES = sorted(C.CASES)
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)


def test_the_cases_cover_the_shapes_the_steps_and_every_cell_byte():
    shapes = {(k.d.shape[1], k.d.shape[0]) for k in C.CASES.values()}
    assert {(1, 1), (1, 37), (41, 1), (2, 2), (3, 2), (67, 19), (97, 83), (131, 70)} <= shapes
    assert {k.step for k in C.CASES.values()} >= {1, 2, 3, 5, 7}
    assert {float(k.max_jump) for k in C.CASES.values()} >= {0.0, 1.0, float("inf")}
    k = C.CASES["step_past_w"]
    assert k.step > k.d.shape[1] and R.grid(k.d.shape[1], k.d.shape[0], k.step) == (1, 1)
    for name in ("rand_67x19", "rand_131x70_s2", "rand_97x83_s3", "rand_97x83"):
        cells = C.reference(name)["cells"]
        for b in C.BYTES:
            assert (cells == b).any(), (name, b)
        d = C.CASES[name].d
        bits = d.view(np.uint32)
        assert (bits == 0x7FC00001).any() and np.isposinf(d).any() and (bits == 0x80000000).any() and 0.2 < (bits == R.INVALID_BITS).mean() < 0.4
    for name in NAMES:
        assert set(np.unique(C.reference(name)["cells"])) <= {0, 1, 2, 3, 5, 6, 7}, name    # never 4: a byte without a triangle is 0
    # past a wave's run of 1024 nodes, and past a block of 4096 of either compaction
    assert C.CASES["rand_67x19"].d.size == 1273 and C.CASES["rand_97x83"].d.size == 8051 and 2 * C.reference("rand_97x83")["cells"].size == 2 * 7872
    assert C.reference("rand_97x83")["n"] > 4096 and C.reference("rand_67x19")["n"] < 1024 < 1273
    assert set(np.unique(C.reference("ramp")["cells"])) == {3, 7}                               # both diagonals, every triangle
    assert C.reference("all_invalid")["n"] == 0 and len(C.reference("all_invalid")["faces"]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_vertex_ranks_are_the_record_order_of_the_matches(name):
    k, ref = C.CASES[name], C.reference(name)
    rec = stereo_ref.matches_ref(k.d, k.step, 0, 1)
    assert len(rec) == ref["n"]
    vi = ref["vertex_index"]
    js, is_ = np.nonzero(vi != R.NONE)
    assert np.array_equal(vi[js, is_], np.arange(ref["n"]))                                    # raster order
    assert np.array_equal(rec["kp0_loc"][:, 0], (is_ * k.step).astype(np.float32)) and np.array_equal(rec["kp0_loc"][:, 1], (js * k.step).astype(np.float32))
    assert ((vi == R.NONE) == (R.nodes_of(k.d, k.step).view(np.uint32) == R.INVALID_BITS)).all()


def test_a_constant_map_gives_every_triangle_and_normals_straight_at_the_camera():
    k, ref = C.CASES["all_valid"], C.reference("all_valid")
    gh, gw = ref["vertex_index"].shape
    assert len(ref["faces"]) == 2 * (gw - 1) * (gh - 1) and (ref["cells"] == 3).all()
    pts = stereo_ref.points_ref(stereo_ref.matches_ref(k.d, k.step, 0, 1), **CAMERA)
    assert (pts[:, 2] > 0).all()
    nrm = R.normals(pts, ref["vertex_index"], ref["cells"])
    assert np.array_equal(nrm, np.tile(np.array([0, 0, -1], np.float32), (ref["n"], 1)))       # exactly (0, 0, -1), -1 bit for bit


@pytest.mark.parametrize("name", NAMES)
def test_every_face_joins_grid_neighbours_that_are_pairwise_joined_and_winds_one_way(name):
    k, ref = C.CASES[name], C.reference(name)
    nodes = R.nodes_of(k.d, k.step)
    gh, gw = nodes.shape
    where = np.zeros((ref["n"], 2), np.int64)
    js, is_ = np.nonzero(ref["vertex_index"] != R.NONE)
    where[ref["vertex_index"][js, is_]] = np.stack([is_, js], 1)
    for face in ref["faces"]:
        assert (face < ref["n"]).all() and len(set(face.tolist())) == 3
        xy = where[face.astype(np.int64)]
        assert np.ptp(xy[:, 0]) == 1 and np.ptp(xy[:, 1]) == 1                                  # three corners of one cell
        for a in range(3):
            (xa, ya), (xb, yb) = xy[a], xy[(a + 1) % 3]
            assert R.joined(nodes[ya, xa], nodes[yb, xb], k.max_jump)
        (px, py), (qx, qy), (rx, ry) = xy
        assert (qx - px) * (ry - py) - (qy - py) * (rx - px) == -1                              # x right, y down: z of the cross product below 0
    # and the other way round: a cell with four pairwise joined corners has both triangles
    full = 0
    for j in range(gh - 1):
        for i in range(gw - 1):
            c = [nodes[j, i], nodes[j, i + 1], nodes[j + 1, i], nodes[j + 1, i + 1]]
            if R.is_valid(c).all() and all(R.joined(p, q, k.max_jump) for p in c for q in c):
                assert ref["cells"][j, i] & 3 == 3
                full += 1
    if name in ("rand_97x83", "ramp", "all_valid"):
        assert full > 10


def test_the_diagonal_rule_in_the_small():
    inv, nan2, inf = R.INVALID, C.FOREIGN_NAN, np.float32(np.inf)
    byte = R.cell_byte
    assert byte(1, 1, 1, 1, 1.0) == 3                                   # a tie: a-d
    assert byte(1, 2, 2, 1.5, 1.0) == 7                                 # |b - c| = 0 < |a - d| = 0.5: b-c
    assert byte(1, 2, 1, 2, 1.0) == 3 and byte(1, 2, 1, 2, 0.5) == 0    # |b - c| = 1 = |a - d|; a diagonal that is not joined kills both
    assert byte(inv, 1, 1, 1, 1.0) == 6 and byte(1, 1, 1, inv, 1.0) == 5  # three corners: b-c, the triangle without the hole
    assert byte(1, inv, 1, 1, 1.0) == 1 and byte(1, 1, inv, 1, 1.0) == 2  # a-d
    assert byte(inv, inv, 1, 1, 1.0) == 0
    assert byte(1, 1, 1, 3, 1.0) == 5                                   # b-c is the smaller jump, d is cut off
    assert byte(3, 1, 1, 1, 1.0) == 6
    assert byte(1, 3, 1, 1, 1.0) == 1 and byte(1, 1, 3, 1, 1.0) == 2    # a-d; b / c cut off
    assert byte(1, nan2, 1, 1, 1.0) == 1 and byte(1, nan2, 1, 1, np.inf) == 1   # a NaN value is valid and joins nothing; NaN < x is false: a-d
    assert byte(nan2, 1, 1, nan2, np.inf) == 0                          # NaN comparison: a-d, which is not joined
    assert byte(inf, inf, inf, inf, np.inf) == 0                        # inf - inf is a NaN
    assert byte(inf, 1, 1, 1, np.inf) == 7 and byte(inf, 1, 1, 1, 1e30) == 6   # |1 - inf| = inf <= inf
    assert byte(-0.0, 0.0, 0.0, -0.0, 0.0) == 3
    assert byte(1, 5, 9, 30, np.inf) == 7 and byte(1, 5, 9, 30, 1.0) == 0


@pytest.mark.parametrize("name", ["rand_97x83_s3", "ramp", "shape_2x2", "rand_67x19"])
def test_select_with_the_identity_changes_nothing_and_select_commutes_with_the_face_list(name):
    ref = C.reference(name)
    n = ref["n"]
    vi, cells = R.select(ref["vertex_index"], ref["cells"], n, np.arange(n))
    assert np.array_equal(vi, ref["vertex_index"]) and np.array_equal(cells, ref["cells"])
    rng = np.random.default_rng(9)
    for kept in (np.nonzero(rng.random(n) < 0.6)[0], np.zeros(0, np.int64), np.concatenate([np.arange(0, n, 2), [n + 3]])):
        vi, cells = R.select(ref["vertex_index"], ref["cells"], n, kept)
        new_of = np.full(n, -1, np.int64)
        inside = kept < n
        new_of[kept[inside]] = np.nonzero(inside)[0]
        f = new_of[ref["faces"].astype(np.int64)]
        want = f[(f >= 0).all(1)].astype(np.uint32).reshape(-1, 3)
        assert np.array_equal(R.faces(vi, cells), want)
        assert set(np.unique(cells)) <= {0, 1, 2, 3, 5, 6, 7}
        assert ((vi != R.NONE).sum()) == int(inside.sum())


def test_normals_skip_what_lies_past_n_and_give_zero_without_a_triangle():
    ref = C.reference("rand_67x19")
    n = ref["n"]
    used = np.zeros(n, bool)
    used[ref["faces"].astype(np.int64).ravel()] = True
    assert used.any() and not used.all()
    assert not ref["normals"][~used].any()                                                     # no triangle: (0, 0, 0)
    half = R.normals(ref["points"][:n // 2], ref["vertex_index"], ref["cells"], out=np.full((n, 3), 7.5, np.float32))
    assert (half[n // 2:] == 7.5).all()
    length = np.linalg.norm(ref["normals"].astype(np.float64), axis=1)
    assert np.allclose(length[length > 0], 1.0, atol=1e-6)
