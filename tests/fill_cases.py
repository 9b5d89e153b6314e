"""The hole-filling cases.  Shared by tests/test_fill_cases.py (which proves on the numpy reference alone that the cases test
something) and tests/test_gpu_fill.py (which holds the kernels of csrc/disparity_filter.hip to that reference bit for bit).

The kernels carry (last measured value, steps since it) along every line of a direction: the horizontal directions a wave per
row in chunks of 64 pixels with a carry from chunk to chunk, the six others a lane per column or diagonal, 64 lines per wave,
16 rows in flight.  So the shapes straddle 64 and 128 in width, 16 in height, and come in both orientations; the holes
reach over chunk seams, to every border and into every corner.  Every map is a float32 array (H, W); INVALID marks a hole.

  shape_WxH         random clumps of holes in rich values on 1 x 1, 1 x 37, 41 x 1, 63 / 64 / 65 x 9, 129 x 17, 257 x 5 and
                    97 x 83 / 83 x 97 (one axis only can hit on the thin ones; a transposed diagonal shows on the last two)
  all_valid, all_holes   nothing to fill; nothing to fill with
  corner_pixel      one measured pixel at (0, 0), no gap limit: its row, its column and its diagonal fill, nothing else
  centre_pixel      one at the centre of 83 x 61: an eight-armed star to every border; the anti-diagonals end on different
                    borders than in the transposed image
  row_hole, column_hole   a hole that spans a whole row (through three chunks of a wave) / a whole column
  frame             measured pixels only in an inner rectangle: the hole reaches each border and each corner
  checkerboard      a one-pixel checkerboard of holes: every hole has 4 axis hits at distance 1 and no diagonal one
  serpentine        a one-pixel serpentine of measured pixels, three rows of holes between its rows, maxGap 1: the middle row stays
  star_gap7         one measured pixel in all-holes, maxGap 7: each arm ends at exactly 7 steps; the pixel at 8 stays a hole
  gap_exact_dI      direction I alone, maxGap 7, sources at exactly 7 and at 8 steps from holes (I = 0 .. 7)
  key_order_min / _median   hits drawn from -0, +0, the infinities, a foreign NaN, negative and equal values: the integer key,
                    not the float order, ranks them
  equal_hits        two equal hit values among three: the lower median is the doubled value
  dir_I             every single direction on one random map (I = 0 .. 7)
  paths_03 / _0f / _f0 / _ff   the usual masks, with minHits 1, popcount and one in between, both rules
  gap_0 / _1 / _7 / _unlimited   the same map under every maxGap of the contract
  half_hole         the left half one hole, no limit: the carry over 70 columns
  strips_WxH        taller than one strip of the march (128 rows): 40 x 150 is two strips, 33 x 290 three; 20 x 290 is two longer
                    ones, because the carries of three would not fit into the output map where they are kept.  Holes of whole
                    columns, a band of hole rows across a strip seam, and one more than a strip tall: the carry from strip to
                    strip, through a strip with no measured pixel on the line"""
from collections import namedtuple

import numpy as np

INVALID = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
FOREIGN_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
NO_LIMIT = 0xFFFFFFFF
MIN, MEDIAN = 0, 1

Case = namedtuple("Case", "d paths max_gap min_hits rule")

RICH = np.array([-0.0, 0.0, np.inf, -np.inf, -3.5, -1.0, 2.0, 2.0, 7.25, 1e-40, -1e-40, 31.0], np.float32)


def _holes(w, h):
    return np.full((h, w), INVALID, np.float32)


def _rich(rng, w, h):
    d = RICH[rng.integers(0, len(RICH), (h, w))].copy()
    d[rng.random((h, w)) < 0.05] = FOREIGN_NAN   # a valid value
    return d


def _clumps(w, h, seed, share=0.5):
    """rich values with rectangular clumps of holes and single-pixel holes, about `share` of the map"""
    rng = np.random.default_rng(seed)
    d = _rich(rng, w, h)
    hole = rng.random((h, w)) < share / 4
    for _ in range(max(1, w * h // 60)):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        hole[y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(1, 13))] = True
    d[hole] = INVALID
    return d


def _tall(w, h, seed):
    d = _clumps(w, h, seed, 0.4)
    d[:, 3] = INVALID                      # a whole column
    d[1:, w - 2] = INVALID                 # ... but for its first pixel: one value carried through every strip
    d[120:137, :] = INVALID                # a band of rows across the seam at 128
    d[120:137, 7] = 9.5
    if h > 280:
        d[100:270, 5:w - 5] = INVALID      # more than a strip tall: a strip with nothing measured on these lines
    return d


def _serpentine(w, h):
    d = _holes(w, h)
    d[0::4, :] = 3.0
    d[0::8, 1::3] = 4.0
    for y in range(0, h - 4, 4):
        d[y + 1:y + 4, w - 1 if y % 8 == 0 else 0] = 5.0
    return d


def _gap_exact(i):
    """direction i alone with maxGap 7: on every line of the direction, measured pixels 8 and 9 steps apart in turn: the holes
    between a pair 8 apart all fill (the last at exactly 7 steps), of those between a pair 9 apart the last one stays"""
    w, h = 71, 23
    d = _holes(w, h)
    rng = np.random.default_rng(100 + i)
    vals = rng.integers(1, 60, (h, w)).astype(np.float32)
    pos = np.cumsum(np.tile([8, 9], 8))
    if i < 2:
        cols = pos[pos < w]
        d[:, cols] = vals[:, cols]
    else:
        rows = pos[pos < h]
        d[rows, :] = vals[rows, :]
        d[0, ::2] = vals[0, ::2]
    return Case(d, 1 << i, 7, 1, MIN)


def build():
    c = {}
    for k, (w, h) in enumerate([(1, 1), (1, 37), (41, 1), (63, 9), (64, 9), (65, 9), (129, 17), (257, 5), (97, 83), (83, 97)]):
        big = w * h > 4000
        c["shape_%dx%d" % (w, h)] = Case(_clumps(w, h, 10 + k), 0xFF, NO_LIMIT if big else 7, 1 if w == 1 or h == 1 else 3, MEDIAN if k % 2 else MIN)
    c["shape_1x1"] = Case(_holes(1, 1), 0xFF, NO_LIMIT, 1, MIN)
    c["all_valid"] = Case(_rich(np.random.default_rng(1), 70, 20), 0xFF, NO_LIMIT, 1, MIN)
    c["all_holes"] = Case(_holes(70, 20), 0xFF, NO_LIMIT, 1, MEDIAN)
    d = _holes(67, 35)
    d[0, 0] = 4.0
    c["corner_pixel"] = Case(d, 0xFF, NO_LIMIT, 1, MIN)
    d = _holes(83, 61)
    d[30, 41] = -2.0
    c["centre_pixel"] = Case(d, 0xFF, NO_LIMIT, 1, MEDIAN)
    rng = np.random.default_rng(2)
    d = _rich(rng, 150, 9)
    d[4, :] = INVALID
    d[7, 1:] = INVALID
    d[2, :-1] = INVALID
    c["row_hole"] = Case(d, 0xFF, NO_LIMIT, 2, MIN)
    d = _rich(rng, 9, 70)
    d[:, 4] = INVALID
    d[1:, 7] = INVALID
    d[:-1, 2] = INVALID
    c["column_hole"] = Case(d, 0xFF, NO_LIMIT, 2, MEDIAN)
    d = _holes(90, 40)
    d[11:29, 13:77] = _rich(rng, 64, 18)
    c["frame"] = Case(d, 0xFF, NO_LIMIT, 1, MEDIAN)
    d = _rich(rng, 66, 19)
    yy, xx = np.mgrid[0:19, 0:66]
    d[(xx + yy) % 2 == 1] = INVALID
    c["checkerboard"] = Case(d, 0xFF, NO_LIMIT, 4, MEDIAN)
    c["serpentine"] = Case(_serpentine(70, 21), 0xFF, 1, 2, MIN)
    d = _holes(40, 40)
    d[20, 19] = 6.0
    c["star_gap7"] = Case(d, 0xFF, 7, 1, MIN)
    for i in range(8):
        c["gap_exact_d%d" % i] = _gap_exact(i)
    keys = _clumps(68, 18, 3, 0.6)
    c["key_order_min"] = Case(keys, 0xFF, 5, 2, MIN)
    c["key_order_median"] = Case(keys, 0xFF, 5, 2, MEDIAN)
    d = _holes(9, 9)
    d[4, 1], d[4, 7], d[0, 4] = 5.0, 5.0, 1.0    # the hole (4, 4): hits 5, 5, 1 -> the lower median is 5
    d[8, 4] = 9.0                                 # ... and 9 on the fourth ray: 1, 5, 5, 9 -> rank 1 is still 5
    c["equal_hits"] = Case(d, 0x0F, NO_LIMIT, 3, MEDIAN)
    one = _clumps(66, 19, 4)
    for i in range(8):
        c["dir_%d" % i] = Case(one, 1 << i, NO_LIMIT if i % 2 else 6, 1, MIN)
    many = _clumps(75, 21, 5, 0.7)
    c["paths_03"] = Case(many, 0x03, NO_LIMIT, 2, MIN)
    c["paths_0f"] = Case(many, 0x0F, 7, 3, MEDIAN)
    c["paths_f0"] = Case(many, 0xF0, 7, 1, MEDIAN)
    c["paths_ff"] = Case(many, 0xFF, 7, 8, MIN)
    c["paths_ff_5"] = Case(many, 0xFF, NO_LIMIT, 5, MEDIAN)
    for name, gap in (("gap_0", 0), ("gap_1", 1), ("gap_7", 7), ("gap_unlimited", NO_LIMIT)):
        c[name] = Case(many, 0xFF, gap, 2, MEDIAN)
    d = _rich(rng, 140, 11)
    d[:, :70] = INVALID
    c["half_hole"] = Case(d, 0xFF, NO_LIMIT, 1, MIN)
    c["strips_40x150"] = Case(_tall(40, 150, 6), 0xFF, NO_LIMIT, 2, MEDIAN)
    c["strips_33x290"] = Case(_tall(33, 290, 7), 0xFF, NO_LIMIT, 1, MIN)
    c["strips_20x290"] = Case(_tall(20, 290, 8), 0xFC, 140, 1, MEDIAN)
    return c


CASES = build()
_reference = {}


def reference(name):
    """fill_ref.fill of the case, computed once and shared: (out, filled), read-only"""
    if name not in _reference:
        import fill_ref
        case = CASES[name]
        out, filled = fill_ref.fill(case.d, case.paths, case.max_gap, case.min_hits, case.rule)
        out.setflags(write=False)
        filled.setflags(write=False)
        _reference[name] = (out, filled)
    return _reference[name]
