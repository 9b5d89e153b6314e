"""The dense-stereo cases and their deterministic scene.  Shared by tests/test_stereo_cases.py (which proves on the numpy
reference alone that the cases test something) and tests/test_gpu_stereo.py (which holds the kernels to that reference).

The scene: a seeded random texture, lightly smoothed; R is cut from it; L(x, y) = R(x - d(x, y), y) with a two-plane integer
disparity field (FAR behind, NEAR on a rectangle in front, so there is an occlusion edge); a constant band copied into both
images (windows inside it cost 0 at every disparity: ties); a saturated 255 block in both.  `identical` pairs are L = R (field 0).

The shapes are the smallest that cross every seam of csrc/stereo.hip: a lane owns 4 columns x 8 disparities, nD = 1, 2, 4, 8,
16 or 32 lanes share a pixel (numDisparities up to 8, 16, 32, 64, 128, 256), a block is 64 (nD = 1), 128 (nD = 2) or 256 threads
and 1024 / nD columns wide (at most 256), and marches down at least 8 r + 8 rows."""
from collections import namedtuple

import numpy as np

FAR, NEAR = 2, 6
NO_LIMIT = 0xFFFFFFFF

Case = namedtuple("Case", "w h r dmin D max_cost lr subpixel kind seed")


def _c(w, h, r, dmin, D, max_cost=NO_LIMIT, lr=-1, subpixel=0, kind="scene", seed=1):
    return Case(w, h, r, dmin, D, max_cost, lr, subpixel, kind, seed)


CASES = {
    # the four of the issue
    "base_r1": _c(96, 72, 1, -1, 12, lr=1, subpixel=1),
    "base_r4": _c(96, 72, 4, -1, 12, lr=0, subpixel=1, seed=2),
    "odd_pitch_r15": _c(131, 70, 15, 0, 10, lr=1, subpixel=1, seed=3),     # odd pitch, the largest window (8 dwords a row)
    "wide_range": _c(70, 37, 2, -3, 40, lr=0, subpixel=1, seed=4),         # w = 2 mod 4; D wider than many pixels' candidates
    # D = 256 (nD = 32: tiles of 32 columns): 297 interior columns = nine tiles and 9 columns, 41 interior rows = two marches
    # of 21 and 20 rows; disparities of both signs; every one of the 32 lanes of a pixel holds candidates somewhere
    "all_256": _c(301, 45, 2, -100, 256, lr=1, subpixel=1, seed=5),
    # the block shapes in between: nD = 1 (64 threads), 2 with two 256-column tiles, 4, 16
    "nd1": _c(61, 33, 3, 0, 8, lr=1, subpixel=0, seed=6),
    "two_wide_tiles": _c(290, 24, 1, 0, 12, lr=-1, subpixel=1, seed=7),
    "nd4_r7": _c(90, 50, 7, -2, 27, lr=0, subpixel=0, seed=8),
    "nd16_r12": _c(190, 60, 12, -40, 100, lr=-1, subpixel=1, seed=9),
    # a sub-pixel winner at either end of a lane's eight disparities, in a 4-lane group: with the planes at d = 2 and 6, dmin = -2
    # puts the near plane's winner on k = 8 (the cost of k - 1 comes from the lane below) and dmin = -5 the far plane's on k = 7
    # (the cost of k + 1 comes from the lane above)
    "edge_below": _c(96, 72, 2, -2, 20, lr=1, subpixel=1, seed=15),
    "edge_above": _c(96, 72, 2, -5, 20, lr=1, subpixel=1, seed=16),
    # no left-right check, no sub-pixel, a cost limit on the scene
    "limit": _c(96, 72, 4, -1, 12, max_cost=400, lr=-1, subpixel=0, seed=2),
    # degenerate
    "one_column": _c(9, 30, 4, -1, 3, kind="identical", seed=10),          # w = 2r + 1: x = r alone, d = 0 its one candidate
    "one_row": _c(40, 5, 2, 0, 6, kind="identical", seed=11),
    "narrower_than_window": _c(8, 30, 4, 0, 4, kind="identical", seed=12), # all invalid
    "lower_than_window": _c(30, 8, 4, 0, 4, kind="identical", seed=13),
    "exact_only": _c(64, 40, 2, 0, 6, max_cost=0, kind="identical", seed=14),  # maxCost 0: only exact matches survive
}


def texture(w, h, seed):
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 256, size=(h + 2, w + 2)).astype(np.int64)
    # lightly smoothed: centre weight 2 in a plus-shaped stencil
    s = (2 * t[1:-1, 1:-1] + t[:-2, 1:-1] + t[2:, 1:-1] + t[1:-1, :-2] + t[1:-1, 2:] + 3) // 6
    return s.astype(np.uint8)


def field(case):
    """the scene's integer disparity of every left pixel"""
    w, h = case.w, case.h
    f = np.full((h, w), 0 if case.kind == "identical" else FAR, np.int64)
    if case.kind == "scene":
        f[h // 5: h - h // 4, (2 * w) // 5: (4 * w) // 5] = NEAR
    return f


def scene(case):
    """-> (left, right) uint8 h x w"""
    w, h = case.w, case.h
    M = 8  # the texture is wider than the images, so that L samples texture everywhere
    t = texture(w + 2 * M, h, case.seed)
    right = t[:, M:M + w].copy()
    if case.kind == "identical":
        return right.copy(), right
    xs = np.arange(w)[None, :] + M - field(case)
    left = t[np.arange(h)[:, None], xs].copy()
    b0, b1 = (3 * h) // 5, (3 * h) // 5 + max(4, h // 6)   # the constant band
    left[b0:b1, 2:w - 2] = 97
    right[b0:b1, 2:w - 2] = 97
    s0, s1 = max(1, h // 12), max(1, h // 12) + max(3, h // 7)  # the saturated block
    left[s0:s1, w // 16: w // 16 + max(4, w // 8)] = 255
    right[s0:s1, w // 16: w // 16 + max(4, w // 8)] = 255
    return left, right


_REF = {}


def reference(name):
    """the numpy reference's result of one case, computed once and shared; never modified"""
    import stereo_ref as R
    if name not in _REF:
        c = CASES[name]
        left, right = scene(c)
        _REF[name] = R.disparity_ref(left, right, c.r, c.dmin, c.D, c.max_cost, c.lr, c.subpixel)
    return _REF[name]
