"""The semi-global-matching cases.  Shared by tests/test_sgm_cases.py (which proves on the numpy reference alone that the
cases test something) and tests/test_gpu_sgm.py (which holds the kernels to that reference).  The scenes are those of
tests/stereo_cases.py (scene / field, by import) plus `flat`: both images constant, so every cost of every pixel ties.

The seams of the kernels as built (csrc/stereo.hip):
  cost pass     k_stereo_sad's march with the volume store: its seams are those of stereo_cases.py (nD = 1 .. 32 lanes a pixel,
                4 columns a lane, tiles of 1024 / nD columns, marches of at least 8 r + 8 rows); a pixel's entry is 8 nD uint16,
                so D = 100 leaves 28 padded entries and D = 1, 2 leave 7 and 6 in the one lane.
  path pass     nD lanes own one path, 64 / nD paths a wave, one wave a block: D <= 8 packs 64 paths into a block and D = 256
                two, so every shape here has a last, partly filled block.  The loads of 8 steps are in flight ahead of the
                chain: paths of every length from 1 up occur (the interiors 1 wide or high, 3 x 3, 35 x 7 and 7 x 35, whose
                diagonals run from length 1 to 7, and base_r1's 94 x 70, whose diagonals run from 1 to 70: below, at and past
                one and several rings).  The group minimum and the neighbours' edge entries move by DPP inside a row of 16
                lanes for nD <= 16 and by shuffles for nD = 32 (all_256).  Diagonals start on the first row (wi of them) and on the
                first column below it (hi - 1): w > h and h > w both occur, and interiors 1 wide or 1 high make every diagonal
                one pixel long.  The first selected direction stores S, the others add: every direction is first in its
                single-direction case, and in 0xFF directions 1 .. 7 add.
  winners       a block owns one interior row and a strip of T = 16384 / (8 nD) pixels of it (1024 at most): 64 pixels at D = 256,
                128 at D = 100, 256 at D = 40, 512 at D = 20, 1024 below; it walks 256 / nD left pixels at a time from
                min(dmin, 0) before the strip to dmin + D - 1 behind it, and the right winners come from an LDS tile [T][8 nD].
                all_256 (five strips, disparities of both signs), nd16_r12 (two) and the four strips_* cases (two strips at
                every other tile shape, negative and positive dmin) cross the strip ends.
Every case keeps popcount(paths) (costClamp + P2) <= 65535, two of them with equality."""
from collections import namedtuple

import numpy as np

import stereo_cases as SC

Case = namedtuple("Case", "w h r dmin D clamp P1 P2 paths lr subpixel kind seed")


def _from(name, clamp, P1, P2, paths=0xFF, **over):
    c = SC.CASES[name]
    d = dict(w=c.w, h=c.h, r=c.r, dmin=c.dmin, D=c.D, clamp=clamp, P1=P1, P2=P2, paths=paths, lr=c.lr, subpixel=c.subpixel, kind=c.kind,
             seed=c.seed)
    d.update(over)
    return Case(**d)


def _c(w, h, r, dmin, D, clamp, P1, P2, paths=0xFF, lr=1, subpixel=1, kind="scene", seed=21):
    return Case(w, h, r, dmin, D, clamp, P1, P2, paths, lr, subpixel, kind, seed)


CASES = {
    # the stereo_cases shapes that cross the lane grouping
    "base_r1": _from("base_r1", 1000, 40, 400),
    "base_r1_4paths": _from("base_r1", 1000, 40, 400, 0x0F),
    "base_r4": _from("base_r4", 3000, 100, 1200),
    "wide_range": _from("wide_range", 1500, 60, 500),
    "nd1": _from("nd1", 2000, 80, 700),
    "nd4_r7": _from("nd4_r7", 6000, 300, 2000),
    "nd16_r12": _from("nd16_r12", 14000, 500, 2000, 0x0F, lr=1),   # 25 x 25 windows: four paths leave room for a clamp of 14000
    "all_256": _from("all_256", 1500, 50, 450),
    "two_wide_tiles": _from("two_wide_tiles", 1000, 40, 400, lr=0),
    "edge_below": _from("edge_below", 1500, 60, 500),              # the winner pass's sub-pixel neighbour from the adjacent lane
    "edge_above": _from("edge_above", 1500, 60, 500),
    # degenerate shapes
    "one_column": _from("one_column", 1000, 40, 400, lr=1, subpixel=1),
    "one_row": _from("one_row", 1000, 40, 400, lr=1, subpixel=1),
    "narrower_than_window": _from("narrower_than_window", 1000, 40, 400),
    "lower_than_window": _from("lower_than_window", 1000, 40, 400),
    "five_by_five": _c(5, 5, 1, -1, 3, 1000, 40, 400),
    "wide_37x9": _c(37, 9, 1, -1, 6, 1000, 40, 400, seed=22),
    "tall_9x37": _c(9, 37, 1, -1, 6, 1000, 40, 400, seed=23),
    "d1": _c(40, 21, 2, 2, 1, 1500, 60, 500, seed=24),
    "d2": _c(40, 21, 2, 2, 2, 1500, 60, 500, seed=25),
    # two strips of the winner pass at the tile shapes the cases above leave at one strip: T = 1024 (nD = 1, 2), 512, 256
    "strips_nd1": _c(1100, 7, 1, -2, 6, 1000, 40, 400, seed=26),
    "strips_nd2": _c(1100, 6, 1, 3, 12, 1000, 40, 400, 0x0F, seed=27),
    "strips_nd4": _c(600, 7, 1, -9, 20, 1000, 40, 400, 0xF0, lr=0, seed=28),
    "strips_nd8": _c(300, 7, 1, -5, 40, 1000, 40, 400, seed=29),
    # P1 = P2 = 0 with a clamp no 3 x 3 cost reaches: SAD's own winners, popcount(paths) times its costs
    "p0_4paths": _from("base_r1", 2295, 0, 0, 0x0F),
    "p0_8paths": _from("base_r1", 2295, 0, 0, 0xFF),
    # ties.  On the flat pair d = 0 is a candidate of every interior pixel and costs 0 along every path, so S(d = 0) = 0 and the
    # smallest candidate wins everywhere, although the non-candidates (costClamp) make the other S differ from pixel to pixel
    "flat": _c(50, 30, 2, 0, 10, 1000, 40, 400, kind="flat"),
    "clamp0": _from("base_r1", 0, 40, 400),
    # the edges of the bound: 3 x 21845 = 65535 and, with one direction, 65535 itself; the 4-path form's largest, 4 x 16383;
    # and P1 = P2
    "bound_3paths": _from("nd4_r7", 21445, 150, 400, 0x07, lr=1, subpixel=1),
    "bound_1path": _from("nd4_r7", 45535, 1000, 20000, 0x10, lr=1, subpixel=1),
    "bound_4paths": _from("base_r4", 15983, 100, 400, 0x0F),
    "p1_equals_p2": _from("base_r1", 1000, 400, 400),
}
for _i in range(8):  # each direction alone
    CASES["dir%d" % _i] = _from("base_r1", 1000, 40, 400, 1 << _i)

# the shapes whose reference the GPU file compares every pixel against
ALL = sorted(CASES)


def scene(case):
    """-> (left, right) uint8 h x w"""
    if case.kind == "flat":
        img = np.full((case.h, case.w), 97, np.uint8)
        return img, img.copy()
    return SC.scene(case)


_REF = {}


def reference(name):
    """the numpy reference's result of one case, computed once and shared; never modified"""
    import sgm_ref as G
    if name not in _REF:
        c = CASES[name]
        left, right = scene(c)
        _REF[name] = G.sgm_ref(left, right, c.r, c.dmin, c.D, c.clamp, c.P1, c.P2, c.paths, c.lr, c.subpixel)
    return _REF[name]
