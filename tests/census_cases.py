"""The census-cost cases.  Shared by tests/test_census_cases.py (which proves on the numpy reference alone that the cases test
something) and tests/test_gpu_census.py (which holds the kernels to that reference).  The scenes are those of
tests/stereo_cases.py (scene / field, by import) plus `flat`: both images constant, so every code is 0 and every cost ties.

c is the census radius, r the aggregation radius, rho = c + r the footprint.  The seams of the kernels as built
(csrc/stereo.hip):
  k_census         one thread a pixel; the code is 0 on the border of width c.
  k_stereo_census  k_stereo_sad's ownership (4 columns x 8 disparities a lane, nD = 1 .. 32 lanes a pixel, strips of 1024 / nD
                   columns, 256 at most, marches of at least 8 rho + 8 rows), so the block shapes are those of stereo_cases.py.
                   The codes are staged as uint8 (c = 1), uint32 (c = 2) or uint64 (c = 3): every c runs another instantiation,
                   and c = 3 alone has Hamming distances above 32, where the upper dword counts.  r = 0 takes the path without a
                   ring and without a leaving row; r = 7 has the longest ring (17 rows).  At c = 3, r = 7 and nD <= 4 the strip
                   is halved to 128 columns to keep the ring inside 64 KB: 64 threads a block at nD = 2 (c3_r7), 32 at nD = 1
                   (nd1_c3_r7), 128 at nD = 4 (nd4_c3_r7), and halved_strip_tiles has three such strips side by side.
                   nd1_c3_r6 is the largest ring that is not halved: 65280 bytes of LDS.
  the three forms  winners (left), k alone (right: every case with lr >= 0), the clamped volume (every SGM case); the winner
                   step, the left-right check, the path and winner passes are those of the SAD calls, with rho for r.
Every SGM case keeps popcount(paths) (costClamp + P2) <= 65535, bound_3paths with equality."""
from collections import namedtuple

import numpy as np

import stereo_cases as SC

NO_LIMIT = SC.NO_LIMIT

Case = namedtuple("Case", "w h c r dmin D max_cost lr subpixel kind seed")
SgmCase = namedtuple("SgmCase", "w h c r dmin D clamp P1 P2 paths lr subpixel kind seed")


def _bm(name, c, r, **over):
    s = SC.CASES[name]
    d = dict(w=s.w, h=s.h, c=c, r=r, dmin=s.dmin, D=s.D, max_cost=NO_LIMIT, lr=s.lr, subpixel=s.subpixel, kind=s.kind, seed=s.seed)
    d.update(over)
    return Case(**d)


def _sgm(name, c, r, clamp, P1, P2, paths=0xFF, **over):
    s = SC.CASES[name]
    d = dict(w=s.w, h=s.h, c=c, r=r, dmin=s.dmin, D=s.D, clamp=clamp, P1=P1, P2=P2, paths=paths, lr=s.lr, subpixel=s.subpixel, kind=s.kind,
             seed=s.seed)
    d.update(over)
    return SgmCase(**d)


CASES = {
    # per-pixel Hamming distance at every code width; c = 3 reaches distances above 32
    "c1_r0": _bm("base_r1", 1, 0),
    "c2_r0": _bm("base_r1", 2, 0),
    "c3_r0": _bm("base_r1", 3, 0),
    "c2_r2": _bm("base_r1", 2, 2),
    "c3_r1": _bm("base_r1", 3, 1),
    # the widest aggregation and the widest footprint (rho = 10) on the odd pitch 131 x 70
    "c1_r7": _bm("odd_pitch_r15", 1, 7),
    "c3_r7": _bm("odd_pitch_r15", 3, 7),
    # the block shapes of stereo_cases
    "nd1": _bm("nd1", 2, 1),
    "two_wide_tiles": _bm("two_wide_tiles", 2, 1),
    "nd4_r7": _bm("nd4_r7", 2, 1),
    "nd16_r12": _bm("nd16_r12", 2, 1),
    "all_256": _bm("all_256", 2, 1),
    # the halved strip of c = 3, r = 7 at the other lane groupings, and three of them side by side
    "nd1_c3_r7": _bm("nd1", 3, 7),
    "nd4_c3_r7": _bm("nd4_r7", 3, 7),
    "nd1_c3_r6": _bm("nd1", 3, 6),
    "halved_strip_tiles": _bm("two_wide_tiles", 3, 7),
    # a sub-pixel winner at either end of a lane's eight disparities: the neighbour's cost comes from the adjacent lane
    "edge_below_r2": _bm("edge_below", 2, 2),
    "edge_above_r2": _bm("edge_above", 2, 2),
    "edge_below_r0": _bm("edge_below", 2, 0),
    "edge_above_r0": _bm("edge_above", 2, 0),
    # the cost limit
    "limit_100": _bm("limit", 2, 2, max_cost=100),
    "exact_only": _bm("exact_only", 1, 1, max_cost=0),              # maxCost 0 on an identical pair: every winner costs 0 and stays
    "exact_on_scene": _bm("base_r1", 2, 1, max_cost=0),             # maxCost 0 on the scene: only the exact winners stay
    # degenerate: w = 2 rho + 1, h = 2 rho + 1, one short of each, and the flat pair
    "one_column": _bm("one_column", 2, 2),                          # 9 x 30, rho = 4
    "one_row": _bm("one_row", 2, 0),                                # 40 x 5, rho = 2
    "narrower_than_footprint": _bm("narrower_than_window", 2, 2),   # 8 x 30
    "lower_than_footprint": _bm("lower_than_window", 2, 2),         # 30 x 8
    "flat": Case(50, 30, 2, 1, 0, 10, NO_LIMIT, 1, 1, "flat", 0),
}

TIE_PRONE = ["c1_r0", "c2_r0", "c3_r0", "flat"]
EDGE = {"edge_below_r2": 8, "edge_above_r2": 7, "edge_below_r0": 8, "edge_above_r0": 7}   # the k the winners crowd on

SGM_CASES = {
    "c2_r0_8paths": _sgm("base_r1", 2, 0, 24, 3, 20),
    "c3_r1_4paths": _sgm("base_r1", 3, 1, 432, 20, 150, 0x0F),
    "d1": SgmCase(40, 21, 2, 0, 2, 1, 24, 3, 20, 0xFF, 1, 1, "scene", 24),
    "all_256": _sgm("all_256", 1, 0, 8, 1, 6),
    "one_column": _sgm("one_column", 2, 2, 600, 20, 150, lr=1, subpixel=1),
    "one_row": _sgm("one_row", 2, 0, 24, 3, 20, lr=1, subpixel=1),
    "narrower_than_footprint": _sgm("narrower_than_window", 2, 2, 600, 20, 150),
    "clamp_bites": _sgm("base_r1", 2, 0, 10, 3, 20),
    "clamp0": _sgm("base_r1", 2, 0, 0, 3, 20),
    # P1 = P2 = 0 and a clamp at the bound n (2r + 1)^2 = 216, which cuts nothing: the block-matching winners, popcount(paths)
    # times their costs
    "p0_4paths": _sgm("base_r1", 2, 1, 216, 0, 0, 0x0F),
    "p0_8paths": _sgm("base_r1", 2, 1, 216, 0, 0, 0xFF),
    "bound_3paths": _sgm("nd4_r7", 2, 1, 21445, 150, 400, 0x07, lr=1, subpixel=1),   # 3 x 21845 = 65535
}

ALL = sorted(CASES)
SGM_ALL = sorted(SGM_CASES)


def scene(case):
    """-> (left, right) uint8 h x w"""
    if case.kind == "flat":
        img = np.full((case.h, case.w), 97, np.uint8)
        return img, img.copy()
    return SC.scene(case)


def radiometric_pairs():
    """base_r1 with both images halved to 0 .. 127, and the right image through v -> 2 v + 1 and v -> v + 100: three pairs whose
    census costs are equal entry for entry.  -> (case, field, [(left, right) x 3])"""
    case = SC.CASES["base_r1"]
    left, right = SC.scene(case)
    l2, r2 = left >> 1, right >> 1
    gained = (r2.astype(np.int64) * 2 + 1).astype(np.uint8)
    lifted = (r2.astype(np.int64) + 100).astype(np.uint8)
    return case, SC.field(case), [(l2, r2), (l2, gained), (l2, lifted)]


_REF = {}


def reference(name):
    """the numpy reference's result of one block-matching case, computed once and shared; never modified"""
    import census_ref as CR
    if ("bm", name) not in _REF:
        c = CASES[name]
        left, right = scene(c)
        _REF["bm", name] = CR.census_disparity_ref(left, right, c.c, c.r, c.dmin, c.D, c.max_cost, c.lr, c.subpixel)
    return _REF["bm", name]


def sgm_reference(name):
    """the numpy reference's result of one semi-global case, computed once and shared; never modified"""
    import census_ref as CR
    if ("sgm", name) not in _REF:
        c = SGM_CASES[name]
        left, right = scene(c)
        _REF["sgm", name] = CR.census_sgm_ref(left, right, c.c, c.r, c.dmin, c.D, c.clamp, c.P1, c.P2, c.paths, c.lr, c.subpixel)
    return _REF["sgm", name]
