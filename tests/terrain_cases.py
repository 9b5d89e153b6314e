"""The cases of the terrain filter (include/ssrlcv_hip.h "terrain filter"): the sizes, radii and contents that
tests/test_gpu_terrain.py runs against tests/terrain_ref.py, and the boxed scene map both it and tests/test_terrain_cases.py
use.  Sizes are (w, h)."""
import zlib

import numpy as np

import terrain_ref as R

UINT32_MAX = 0xFFFFFFFF
# one-cell lines, the edges of a wave's 64 cells and of a block's 4 rows (rows) and 256 columns (columns), heights and widths
# that no 2r + 1 divides
SIZES = ((1, 1), (1, 37), (37, 1), (2, 2), (63, 5), (64, 64), (65, 33), (129, 70), (200, 131), (257, 96), (300, 260))
LARGEST = SIZES[-1]
FORM_RADII = (8, 9)   # the library takes the direct form up to radius 8 and the running minima above
RADII = (1, 2, 3) + FORM_RADII + (33, UINT32_MAX)
LARGEST_RADII = (7, 31, 32, 64, 100, LARGEST[0] - 1, LARGEST[0], 1 << 31)
# the kernels' own boundaries: a column block is 256 lanes wide -- 255, 256 and 257 columns --, and a column of more than 65535
# segments has its segments walked by a grid of 65535 in strides -- 65535 and 65536 segments of 3 rows, and 200 000 rows
BOUNDARY_SIZES = ((255, 6), (256, 6), (1, 3 * 65535), (2, 3 * 65536), (1, 200000))
BOUNDARY_RADII = (1, 33)

HARD_BITS = np.array([0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00001, 0x7FBFFFFF, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                      0x7F7FFFFF, 0xFF7FFFFF, R.INVALID], np.uint32)   # NaNs beside the invalid pattern, +-inf, +-0, +-FLT_MAX, itself


def _rng(name, w, h):
    return np.random.RandomState(zlib.crc32(("%s-%dx%d" % (name, w, h)).encode()) & 0x7FFFFFFF)


def _with_holes(a, share, rng):
    b = R.bits_of(a).copy()
    b[rng.rand(*b.shape) < share] = R.INVALID
    return b.view(np.float32)


def noise(w, h):
    return (_rng("noise", w, h).randn(h, w) * 3).astype(np.float32)


def holes5(w, h):
    rng = _rng("holes5", w, h)
    return _with_holes((rng.randn(h, w) * 3).astype(np.float32), 0.05, rng)


def holes60(w, h):
    rng = _rng("holes60", w, h)
    return _with_holes((rng.randn(h, w) * 3).astype(np.float32), 0.60, rng)


def all_invalid(w, h):
    return np.full((h, w), R.INVALID, np.uint32).view(np.float32)


def single(w, h):
    rng = _rng("single", w, h)
    b = np.full((h, w), R.INVALID, np.uint32)
    b[rng.randint(h), rng.randint(w)] = np.float32(-2.5).view(np.uint32)
    return b.view(np.float32)


def constant(w, h):
    return np.full((h, w), 1.25, np.float32)


def hard(w, h):
    """drawn from the bit patterns a sentinel could collide with"""
    rng = _rng("hard", w, h)
    return HARD_BITS[rng.randint(len(HARD_BITS), size=(h, w))].view(np.float32)


def plane(w, h):
    """dsm_cases.tilted_plane: 0.3 i - 0.2 j + 1 with two holes, on the sizes that hold them"""
    import dsm_cases as DC
    return DC.tilted_plane(w, h)[0]


def plane_fits(w, h):
    return w > 11 and h > 5


def subtract_pair(w, h):
    """two hard maps; where the map has the cells, the first four of row 0 hold inf - inf, -inf - -inf, inf - -inf and a NaN - 1"""
    rng = _rng("subtract", w, h)
    a, b = hard(w, h).view(np.uint32).copy(), HARD_BITS[rng.randint(len(HARD_BITS), size=(h, w))].copy()
    forced = ((0x7F800000, 0x7F800000), (0xFF800000, 0xFF800000), (0x7F800000, 0xFF800000), (0x7FC00001, 0x3F800000))
    for i, (x, y) in enumerate(forced[:w]):
        a[0, i], b[0, i] = x, y
    return a.view(np.float32), b.view(np.float32)


CONTENTS = {"noise": noise, "holes5": holes5, "holes60": holes60, "all_invalid": all_invalid, "single": single, "constant": constant,
            "hard": hard, "plane": plane}


def maps(w, h):
    """(name, map) of every content on a size"""
    for name, make in CONTENTS.items():
        if name != "plane" or plane_fits(w, h):
            yield name, make(w, h)


def radii_of(size):
    return RADII + (LARGEST_RADII if size == LARGEST else ())


# the terrain call: 1, 4 and 8 levels, thresholds that include 0
TERRAIN_PARAMS = (((3,), (0.5,)),
                  ((1, 2, 4, 8), (0.0, 0.25, 1.0, 0.0)),
                  ((1, 2, 3, 5, 8, 13, 40, UINT32_MAX), (0.5, 0.0, 1.5, 0.75, 0.0, 2.0, 3.0, 1.0)))


# ---- the boxed scene: the rendered scene's true heights, flattened to a relief below 0.3, with boxes and one plateau on them
RELIEF = 0.29
SCENE_RADII = (1, 2, 4, 8)
SCHEDULE = dict(cell=1, max_radius=8, slope=0.3, initial=0.5, maximum=1.5)
# (x0, y0, side, height): sides 1, 3, 5, 8 and 16, heights 2 to 6; the 5 touches the top border, the 8 the left one; the 1 and
# the 3 stand one ground cell apart.  A box in a corner of side above r_max + 1 would hold a whole clipped window and be ground
BOXES = ((10, 10, 1, 2.0), (12, 9, 3, 3.0), (40, 0, 5, 4.0), (0, 40, 8, 5.0), (60, 60, 16, 6.0))
PLATEAU = (30, 30, 17, 3.0)   # side 2 r_max + 1: never flagged
_SCENE = {}


def boxed(base):
    """boxes and plateau on a relief -> dict(height, box: bool map, plateau: bool map, ground: bool map, top: the boxes' heights)"""
    base = np.asarray(base, np.float64)
    spread = base.max() - base.min()
    ground = ((base - base.mean()) * (RELIEF / spread if spread > 0 else 0.0)).astype(np.float32)
    assert float(ground.max()) - float(ground.min()) < 0.3
    h, w = ground.shape
    height, box, plateau, top = ground.copy(), np.zeros((h, w), bool), np.zeros((h, w), bool), np.zeros((h, w), np.float32)
    taken = np.zeros((h, w), bool)
    for x0, y0, side, up in BOXES + (PLATEAU,):
        assert x0 + side <= w and y0 + side <= h
        assert not taken[max(y0 - 1, 0):y0 + side + 1, max(x0 - 1, 0):x0 + side + 1].any()   # a ground cell between any two, 8-neighbours counted
        taken[y0:y0 + side, x0:x0 + side] = True
        height[y0:y0 + side, x0:x0 + side] += np.float32(up)
        top[y0:y0 + side, x0:x0 + side] = up
        (plateau if (x0, y0, side, up) == PLATEAU else box)[y0:y0 + side, x0:x0 + side] = True
    return {"height": height, "box": box, "plateau": plateau, "ground": ~taken, "top": top}


def scene():
    """the boxed scene map of the rendered scene (render_cases.scene_model, 96 x 96), computed once; never modified"""
    if not _SCENE:
        import render_cases as RC
        _SCENE.update(boxed(RC.scene_model()["height"]))
    return _SCENE


def with_holes(height, share=0.10, seed=7):
    return _with_holes(height, share, np.random.RandomState(seed))
