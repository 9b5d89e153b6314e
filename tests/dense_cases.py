"""The dense-SIFT cases and their CPU oracle (oracle/oracle_sift.c: oracle_sift_dense, items 1-6 of the contract in
include/ssrlcv_hip.h restated in plain C from the oracle's own pieces, nothing of ssrlcv_amd/csrc).  tests/test_dense_oracle.py
proves on the CPU that every case is a valid input; tests/test_gpu_dense.py holds ssrlcv_hip_sift_dense_u8 and the export
chain (tests/dense_ref.py) to the oracle's records, bit for bit.

A case is (image, parameters).  The conditions every case must meet -- asserted, never worked round by skipping records:
no oracle theta is NaN or infinite (a 0 / 0 in the peak parabola has no defined bit pattern), no oracle descriptor is without
a vote (its bytes are (uint8_t)roundf(0 / 0)), no integer vote bin reaches 2^31."""
import ctypes

import numpy as np

import dense_ref as D
import helpers as H

u32, f32, i64 = ctypes.c_uint32, ctypes.c_float, ctypes.c_longlong

_IMAGES, _ORACLE = {}, {}


def saturated(w, h):
    """L(x, y) = ((x // 2) + (y // 2)) % 2: both central differences are +-1 at every pixel -- gradient magnitude sqrt(2),
    the bound the vote scale assumes -- and the four diagonal directions are equally frequent"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx // 2) + (yy // 2)) % 2) * 255).astype(np.uint8)


def step(w, h):
    """a vertical 0 / 255 step in the middle: the only gradient direction is +x, one histogram bin"""
    img = np.zeros((h, w), np.uint8)
    img[:, w // 2:] = 255
    return img


def ramp(w, h):
    """a horizontal ramp: the same gradient at every pixel"""
    return np.broadcast_to((np.arange(w) * (252 // (w - 1))).astype(np.uint8), (h, w)).copy()


def one_pixel(w, h):
    """one differing pixel on a constant field: four pixels carry a gradient"""
    img = np.full((h, w), 100, np.uint8)
    img[h // 2, w // 2] = 200
    return img


def checkerboard(w, h):
    """a 1-pixel checkerboard: L(x + 1) == L(x - 1) everywhere, every central difference is zero"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) % 2) * 255).astype(np.uint8)


def synthetic(w, h, seed, flat_share=0.0):
    img = H.synthetic_image(w, h, seed=seed)
    if flat_share:
        img = img.copy()
        img[:, : int(round(w * flat_share))] = 128
    return img


_BUILDERS = {"synthetic": synthetic, "saturated": saturated, "step": step, "ramp": ramp, "one_pixel": one_pixel,
             "checkerboard": checkerboard}


def image(spec):
    """spec = (builder name, w, h, ...) -> the u8 image, built once"""
    if spec not in _IMAGES:
        _IMAGES[spec] = np.ascontiguousarray(_BUILDERS[spec[0]](*spec[1:]))
    return _IMAGES[spec]


def S(w, h, seed, flat_share=0.0):
    return ("synthetic", w, h, seed, flat_share)


# name -> (image spec, parameters).  Unnamed parameters are the defaults: stride 1, sigma 1.6, max_orientations 2, thr 0.8,
# ori_width 1.5, desc_width 6.0 (wo = 8, wd = 10).
CASES = {
    # the cases tests/test_gpu_dense.py has always had
    "base": (S(64, 48, 3), dict(stride=1, sigma=1.6, max_orientations=2)),
    "many_tiles_1": (S(160, 144, 5), dict(stride=1, sigma=1.6, max_orientations=1)),
    "many_tiles_2": (S(160, 144, 5), dict(stride=1, sigma=1.6, max_orientations=2)),
    "many_tiles_4": (S(160, 144, 5), dict(stride=1, sigma=1.6, max_orientations=4)),
    "stride_3": (S(97, 83, 7), dict(stride=3, sigma=1.6, max_orientations=2)),
    "stride_7": (S(97, 83, 7), dict(stride=7, sigma=1.6, max_orientations=2)),
    "sigma_1.0": (S(128, 96, 11), dict(stride=1, sigma=1.0, max_orientations=2)),
    "sigma_2.3": (S(128, 96, 11), dict(stride=1, sigma=2.3, max_orientations=2)),
    "holes": (S(160, 96, 13, 0.4), dict(stride=1, sigma=1.6, max_orientations=1)),
    # halos up to the limit of 32, and the orientation window wider than the descriptor's
    "largest_wd": (S(100, 92, 17), dict(sigma=5.3)),                                     # wo 24, wd 32; 35 x 27 points
    "both_halos_32": (S(100, 92, 17), dict(sigma=5.3, ori_width=2.0)),                   # wo 32, wd 32
    "wo_gt_wd": (S(100, 92, 17), dict(sigma=2.0, ori_width=5.3, desc_width=3.0)),        # wo 32, wd 6: margin from wo
    "small_wo_gt_wd": (S(97, 83, 7), dict(sigma=1.6, ori_width=3.0, desc_width=4.0)),    # wo 15, wd 7; 66 x 52 points
    # slot logic
    "slots_8": (S(96, 80, 19), dict(max_orientations=8, thr=0.3)),
    "slots_8_thr_1": (S(96, 80, 19), dict(max_orientations=8, thr=1.0)),
    "slots_1_low_thr": (S(96, 80, 19), dict(max_orientations=1, thr=0.1)),
    # strides: the 2 x 2 tile; one point per tile; one point per grid, with and without the 32-bit wrap of 15 stride
    "stride_40": (S(128, 96, 11), dict(stride=40)),
    "stride_1000": (S(128, 96, 11), dict(stride=1000)),
    "stride_0x11111112": (S(128, 96, 11), dict(stride=0x11111112)),
    "stride_0xFFFFFFFF": (S(128, 96, 11), dict(stride=0xFFFFFFFF)),
    # every tile shape of csrc/dense.hip's pick_tile (k_dense_orient, k_dense_desc) that the strides above leave out, several
    # tiles of each with remainders: 16x8 16x8; 8x8 8x4; 8x4 8x4; 4x4 4x4; 4x4 4x2; 2x2 2x2; 2x1 2x1
    "tiles_stride_5": (S(256, 224, 23), dict(stride=5)),
    "tiles_stride_10": (S(256, 224, 23), dict(stride=10)),
    "tiles_stride_13": (S(256, 224, 23), dict(stride=13)),
    "tiles_stride_20": (S(256, 224, 23), dict(stride=20)),
    "tiles_stride_28": (S(256, 224, 23), dict(stride=28)),
    "tiles_stride_60": (S(256, 224, 23), dict(stride=60)),
    "tiles_stride_100": (S(256, 224, 23), dict(stride=100)),
    # degenerate grids (margin 10): one point, one column, one row
    "one_point": (S(22, 22, 1), dict()),
    "one_column": (S(22, 40, 1), dict()),
    "one_row": (S(40, 22, 1), dict()),
    # images at the edges of the arithmetic
    "saturated": (("saturated", 64, 56), dict()),
    "saturated_wd_32": (("saturated", 90, 84), dict(sigma=5.3)),
    "step": (("step", 64, 56), dict()),
    "ramp": (("ramp", 64, 56), dict(max_orientations=4)),
    "one_pixel": (("one_pixel", 64, 48), dict()),
    "no_gradient": (("checkerboard", 64, 48), dict()),
    "empty_grid": (S(21, 40, 1), dict()),                                                # one pixel short of a column
}


def shape_of(name):
    """(w, h, stride, sigma, ori_width, desc_width) of a case: the arguments of dense_ref.grid"""
    spec, kw = CASES[name]
    return (spec[1], spec[2], kw.get("stride", 1), kw.get("sigma", 1.6), kw.get("ori_width", 1.5), kw.get("desc_width", 6.0))


def oracle_grid(lib, w, h, stride=1, sigma=1.6, ori_width=1.5, desc_width=6.0):
    """-> (margin, nx, ny, wo, wd) as the oracle computes them"""
    out = [u32() for _ in range(5)]
    rc = lib.oracle_sift_dense_grid(u32(w), u32(h), u32(stride), f32(sigma), f32(ori_width), f32(desc_width),
                                    *[ctypes.byref(v) for v in out])
    assert rc == 0, rc
    return tuple(v.value for v in out)


def oracle_stats(lib):
    """-> (largest integer vote bin, descriptors without a vote) of the last oracle_dense call"""
    top, empty = u32(), u32()
    lib.oracle_sift_dense_stats(ctypes.byref(top), ctypes.byref(empty))
    return top.value, empty.value


def oracle_dense(lib, img, stride=1, sigma=1.6, max_orientations=2, thr=0.8, ori_width=1.5, desc_width=6.0, capacity=None,
                 guard=0):
    """-> (FEATURE records written, the full count, level L (h, w) float32, (largest vote bin, empty descriptors)).
    capacity None: the grid's maximum.  guard: records of 0xA5 bytes allocated behind capacity and returned with the rest."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    _, nx, ny, _, _ = oracle_grid(lib, w, h, stride, sigma, ori_width, desc_width)
    cap = nx * ny * max_orientations if capacity is None else capacity
    buf = np.full((cap + guard) * 152, 0xA5, np.uint8)
    level = np.zeros((h, w), np.float32)
    lib.oracle_sift_dense.restype = i64
    n = lib.oracle_sift_dense(H.P(img), u32(w), u32(h), u32(stride), f32(sigma), u32(max_orientations), f32(thr), f32(ori_width),
                              f32(desc_width), H.P(buf) if cap else None, u32(cap), H.P(level))
    assert n >= 0, n
    keep = (min(n, cap) + guard) if guard else min(n, cap)
    return buf[: keep * 152].view(H.FEATURE), int(n), level, oracle_stats(lib)


def oracle_case(lib, name):
    """the oracle's result of one case, computed once per process and shared; never modified"""
    if name not in _ORACLE:
        spec, kw = CASES[name]
        feats, n, level, stats = oracle_dense(lib, image(spec), **kw)
        feats.setflags(write=False)
        level.setflags(write=False)
        _ORACLE[name] = (feats, n, level, stats)
    return _ORACLE[name]


def assert_conditions(name, feats, n, stats):
    """the three conditions of the module docstring, on the oracle's output"""
    top, empty = stats
    assert len(feats) == n, (name, len(feats), n)
    assert np.isfinite(feats["theta"]).all(), (name, "non-finite theta", int((~np.isfinite(feats["theta"])).sum()))
    assert empty == 0, (name, "descriptors without a vote", empty)
    assert top < 2 ** 31, (name, "vote bin", top)
    if n:
        assert top > 0, name


def oracle_thetas(lib, level, kp, lam, maxo, thr):
    """oracle_compute_thetas of one SSKEYPOINT record on level (h, w) -> (thetas[maxo], valid[maxo])"""
    h, w = level.shape
    thetas, valid = np.zeros(8, np.float32), np.zeros(8, np.int32)
    lib.oracle_compute_thetas(H.P(level), u32(w), u32(h), f32(1.0), f32(lam), H.P(kp), u32(maxo), f32(thr), H.P(thetas), H.P(valid))
    return thetas[:maxo], valid[:maxo]


def grid_of(name):
    return D.grid(*shape_of(name))
