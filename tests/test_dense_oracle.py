"""The CPU oracle's dense SIFT (oracle_sift_dense, tests/dense_cases.py) checked on the CPU, before anything of it is compared
with a GPU: its grid is the library's and the contract's, truncation and the stride subset hold, it is the composition of the
two per-key-point oracle calls, its bytes do not depend on the thread count, and every case tests/test_gpu_dense.py runs is
a valid input (dense_cases: finite thetas, no descriptor without a vote, no vote bin at 2^31)."""
import ctypes

import numpy as np
import pytest

import dense_cases as C
import dense_ref as D
import helpers as H

u32 = ctypes.c_uint32

# (w, h, stride, sigma, ori_width, desc_width): the shapes of test_dense_host.test_grid_follows_the_formulas ...
HOST_SHAPES = [(64, 48, 1, 1.6), (160, 144, 1, 1.6), (97, 83, 3, 1.6), (97, 83, 7, 1.6), (128, 96, 1, 1.0), (128, 96, 1, 2.3),
               (128, 96, 4, 1.6), (21, 21, 1, 1.6), (22, 22, 1, 1.6), (22, 21, 1, 1.6)]
# ... and of every case, the degenerate grids and the long strides among them
SHAPES = sorted(set([s + (1.5, 6.0) for s in HOST_SHAPES] + [C.shape_of(name) for name in C.CASES]))


@pytest.fixture(scope="module")
def hip_lib():
    from ssrlcv_amd import _lib
    return _lib.load()


class Params(ctypes.Structure):
    _fields_ = [("stride", u32), ("sigma", ctypes.c_float), ("maxOrientations", u32), ("orientationThreshold", ctypes.c_float),
                ("orientationContribWidth", ctypes.c_float), ("descriptorContribWidth", ctypes.c_float)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-s%d-%g-%g-%g" % s)
def test_grid(oracle_lib, hip_lib, shape):
    w, h, stride, sigma, ow, dw = shape
    m, nx, ny, wo, wd = C.oracle_grid(oracle_lib, *shape)
    assert (m, nx, ny, wo, wd) == D.grid(*shape)
    p = Params(stride, sigma, 2, 0.8, ow, dw)
    gm, gnx, gny = u32(), u32(), u32()
    assert hip_lib.ssrlcv_sift_dense_grid(u32(w), u32(h), ctypes.byref(p), ctypes.byref(gm), ctypes.byref(gnx), ctypes.byref(gny)) == 0
    assert (gm.value, gnx.value, gny.value) == (m, nx, ny)
    assert m == max(wo, wd)


def test_grid_edges_are_what_the_case_table_says():
    assert C.grid_of("largest_wd") == (32, 35, 27, 24, 32)
    assert C.grid_of("both_halos_32") == (32, 35, 27, 32, 32)
    assert C.grid_of("wo_gt_wd") == (32, 35, 27, 32, 6)
    assert C.grid_of("small_wo_gt_wd") == (15, 66, 52, 15, 7)
    assert C.grid_of("stride_40")[:3] == (10, 3, 2)
    for name in ("stride_1000", "stride_0x11111112", "stride_0xFFFFFFFF", "one_point"):
        assert C.grid_of(name)[:3] == (10, 1, 1), name
    assert C.grid_of("one_column")[:3] == (10, 1, 19) and C.grid_of("one_row")[:3] == (10, 19, 1)
    assert C.grid_of("empty_grid")[:3] == (10, 0, 0)
    assert C.grid_of("saturated_wd_32") == (32, 25, 19, 24, 32)


def test_records_lie_on_the_grid_in_order(oracle_lib):
    """grid order, then slot order: the locations are those of dense_ref.keypoints, each repeated once per slot"""
    for name in ("base", "stride_7", "wo_gt_wd", "one_column", "stride_40"):
        feats, n, _, _ = C.oracle_case(oracle_lib, name)
        kp = D.keypoints(*C.shape_of(name))
        _, first, counts = np.unique(np.ascontiguousarray(feats["loc"]).view(np.uint64).reshape(-1), return_index=True, return_counts=True)
        order = np.argsort(first)
        maxo = C.CASES[name][1].get("max_orientations", 2)
        assert counts.max() <= maxo and counts.sum() == n
        assert np.array_equal(feats["loc"][first[order]], kp["loc"]), name  # every grid point of these images has a peak
        assert (feats["parent"] == -1).all() and (H.bits(feats["sigma"]) == H.bits(kp["sigma"][:1])).all()


def test_truncation(oracle_lib):
    spec, kw = C.CASES["base"]
    full, n, _, _ = C.oracle_case(oracle_lib, "base")
    twin = np.flatnonzero((full["loc"][1:] == full["loc"][:-1]).all(1))
    cap = int(twin[len(twin) // 2]) + 1  # between the two slots of one grid point
    got, count, _, _ = C.oracle_dense(oracle_lib, C.image(spec), capacity=cap, guard=16, **kw)
    assert count == n and len(got) == cap + 16
    assert got[:cap].tobytes() == full[:cap].tobytes()
    assert (got[cap:].view(np.uint8) == 0xA5).all()
    none, count, _, stats = C.oracle_dense(oracle_lib, C.image(spec), capacity=0, **kw)
    assert count == n and len(none) == 0 and stats == (0, 0)


def test_subset(oracle_lib):
    """the stride-4 result is the stride-1 result restricted to every fourth point, field by field"""
    img = C.image(C.S(128, 96, 11))
    m = D.grid(128, 96)[0]
    fine, n1, _, _ = C.oracle_dense(oracle_lib, img, stride=1)
    coarse, n4, _, _ = C.oracle_dense(oracle_lib, img, stride=4)
    x, y = fine["loc"][:, 0].astype(np.int64), fine["loc"][:, 1].astype(np.int64)
    keep = ((x - m) % 4 == 0) & ((y - m) % 4 == 0)
    assert n4 > 0 and keep.sum() == n4
    assert coarse.tobytes() == fine[keep].tobytes()


def test_composition(oracle_lib):
    """the dense records are what a loop over the two per-key-point oracle calls gives on the normalised level"""
    spec, kw = C.CASES["base"]
    feats, n, level, _ = C.oracle_case(oracle_lib, "base")
    img = C.image(spec).astype(np.float32)
    assert np.array_equal(H.bits(level), H.bits((img - img.min()) / (img.max() - img.min())))
    level = np.ascontiguousarray(level)
    want = []
    for kp in D.keypoints(*C.shape_of("base")):
        kp = np.array([kp])
        thetas, valid = C.oracle_thetas(oracle_lib, level, kp, 1.5, kw["max_orientations"], 0.8)
        for theta in thetas[valid != 0]:
            kp["theta"] = theta
            ft = np.zeros(1, H.FEATURE)
            oracle_lib.oracle_fill_descriptor(H.P(level), u32(64), u32(48), ctypes.c_float(1.0), ctypes.c_float(6.0), H.P(kp), H.P(ft))
            want.append(ft)
    want = np.concatenate(want)
    assert len(want) == n
    assert (want["parent"] == -1).all()
    H.assert_features_equal(feats, want)


def test_threads(oracle_lib):
    """one thread and sixteen give identical bytes, records and level"""
    omp = ctypes.CDLL("libgomp.so.1")
    omp.omp_get_max_threads.restype = ctypes.c_int
    before = omp.omp_get_max_threads()
    out = {}
    try:
        for threads in (1, 16):
            omp.omp_set_num_threads(threads)
            for name in ("base", "saturated", "one_column"):
                spec, kw = C.CASES[name]
                feats, n, level, stats = C.oracle_dense(oracle_lib, C.image(spec), **kw)
                out[threads, name] = (feats.tobytes(), n, level.tobytes(), stats)
    finally:
        omp.omp_set_num_threads(before)
    for name in ("base", "saturated", "one_column"):
        assert out[1, name] == out[16, name], name
        assert out[1, name][1] > 0


@pytest.mark.parametrize("name", list(C.CASES))
def test_input_conditions(oracle_lib, name):
    feats, n, level, stats = C.oracle_case(oracle_lib, name)
    C.assert_conditions(name, feats, n, stats)
    assert np.isfinite(level).all() and level.min() == 0.0 and level.max() == 1.0
    _, nx, ny, _, _ = C.grid_of(name)
    assert n <= nx * ny * C.CASES[name][1].get("max_orientations", 2)


def test_what_the_edge_images_reach(oracle_lib):
    """the properties the case table claims for its images, from the oracle's own output"""
    count = lambda name: C.oracle_case(oracle_lib, name)[1]
    points = lambda name: C.grid_of(name)[1] * C.grid_of(name)[2]
    # saturated: |dL/dx| = |dL/dy| = 1 at every pixel the windows sample (the image border's stencil is its inner neighbour's)
    L = C.oracle_case(oracle_lib, "saturated")[2]
    assert (np.abs(L[:, 2:] - L[:, :-2]) == 1.0).all() and (np.abs(L[2:, :] - L[:-2, :]) == 1.0).all()
    assert count("saturated") == 2 * points("saturated") == 3010  # more peaks than the two slots, at every point
    assert count("saturated_wd_32") == 2 * points("saturated_wd_32")
    assert C.oracle_case(oracle_lib, "saturated_wd_32")[3][0] > 2 ** 26  # the largest bins of all: within 2^5 of the limit
    # the four diagonal directions hold the whole histogram: with eight slots, four orientations per point
    img = C.image(C.CASES["saturated"][0])
    feats8, n8, _, _ = C.oracle_dense(oracle_lib, img, max_orientations=8)
    assert n8 == 4 * points("saturated")
    assert len(np.unique(H.bits(feats8["theta"]))) == 4  # no parabola offset: each peak's neighbours are both empty
    # step: one bin; the 18 columns whose orientation window (wo = 8) holds column 31 or 32
    assert count("step") == 18 * 35 == 630
    assert (H.bits(C.oracle_case(oracle_lib, "step")[0]["theta"]) == 0).all()  # hp = hn = 0: the peak sits at +0.0
    # ramp: the same single bin at every point, also with four slots
    assert count("ramp") == points("ramp") == 1505
    assert (H.bits(C.oracle_case(oracle_lib, "ramp")[0]["theta"]) == 0).all()
    assert 0 < count("one_pixel") < 2 * 19 * 19  # only windows that hold one of the four gradient pixels
    assert count("no_gradient") == 0 and points("no_gradient") == 43 * 27
    assert count("empty_grid") == 0 and points("empty_grid") == 0
    # slot logic: threshold 1.0 keeps the maximum alone, one slot keeps the strongest of many
    assert count("slots_8_thr_1") == points("slots_8_thr_1") == count("slots_1_low_thr")
    assert count("slots_8") > 3 * points("slots_8")
    per_point = np.unique(np.ascontiguousarray(C.oracle_case(oracle_lib, "slots_8")[0]["loc"]).view(np.uint64).reshape(-1), return_counts=True)[1]
    assert per_point.max() == 8  # at least one point fills every slot
    # holes: grid points deep in the flat part give nothing
    assert 0.3 * points("holes") < count("holes") < 0.9 * points("holes")
