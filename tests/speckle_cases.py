"""The disparity post-filter cases.  Shared by tests/test_speckle_cases.py (which proves on the numpy reference alone that the
cases test something) and tests/test_gpu_speckle.py (which holds the kernels of csrc/disparity_filter.hip to that reference).

The labelling kernels work on tiles of TILE_W x TILE_H = 64 x 16 pixels: a block unites one tile in LDS (a wave per row: row
runs by ballot, then the rows through atomicMin), a second pass unites across the tile seams (the columns x = 64 k and the
rows y = 16 k), a third takes every pixel to its root.  Every map is a float32 array; INVALID marks a hole.  Each case names
the seam it crosses:

  constant          150 x 40, no multiple of the tile: ONE component over 3 x 3 tiles -- every seam pixel unites, every tile
                    adds its count to one counter (the count-contention path)
  checker_holes     valid / invalid checkerboard: no link at all, ceil(w h / 2) components of one pixel, runs of length 1
  checker_values    two disparities further apart than maxDiff: w h components, every pixel valid
  serpentine        a one-pixel path: the full even rows joined alternately at the right and the left end.  It crosses every
                    vertical seam in every even row and a horizontal seam at an image edge every 16 rows: the union-find depth
  serpentine_t      its transpose: full even columns, crossing every horizontal seam in every even column
  comb_bottom       teeth (the even columns) that join only in the LAST row: the smallest index, the top of the first tooth, is
                    not where the join happens, so the roots of all teeth change at the very end
  comb_top          teeth that join in the first row
  spirals           two interleaved one-pixel spirals of the SAME disparity, one pixel apart everywhere: two components
  ramp              rises by exactly maxDiff per pixel away from column 63: one component (the transitive closure)
  ramp_step_seam    the same with one step of nextafter(maxDiff) between columns 63 and 64, on a tile seam: two components
  ramp_step_inside  that step between columns 74 and 75, inside a tile (a row run ends there)
  corner_diagonal   two blocks that meet only diagonally at the tile corner (64, 16): not linked
  blobs             bars of maxSpeckleSize - 1, maxSpeckleSize and maxSpeckleSize + 1 pixels astride the seam x = 64, and three
                    more astride y = 16: the <= of the filter, with the count of a component summed over two tiles
  column, row, one_pixel   w = 1 (a wave with one lane in the image), h = 1, 1 x 1
  all_invalid       nothing to label
  max_diff_zero     maxDiff = 0: equal values only; -0 and +0 are equal; one pixel a single ulp off is alone
  infinite_diff     maxDiff = +inf over random values: everything links, except that inf - inf is a NaN (two adjacent +inf pixels
                    are joined through their other neighbours only) and a foreign NaN pixel, valid, links to nothing
  infinities_alone  maxDiff = +inf, two adjacent +inf pixels in a hole: two components
  infinite_values   a finite maxDiff: the +inf pixels and the foreign NaN are components of one pixel
  median_mix        (median) values from a small set with equal values, -0 and +0, the infinities and a foreign NaN, the share
                    of holes falling from left to right so that every valid count 1 .. 9 and 1 .. 25 occurs; valid corners
  lonely, hole      (median) a valid pixel among holes keeps its value; a hole among valid pixels stays a hole
  noisy_real        the disparity of the stereo_cases scene "base_r4" matched without the left-right check against a right image
                    with deterministic salt noise: real speckles beside one large surface"""
from collections import namedtuple

import numpy as np

TILE_W, TILE_H = 64, 16
INVALID = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
FOREIGN_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
MAX_SPECKLE = 12

# d: the map; max_diff, max_size: the filter's parameters; sizes: the sorted component sizes its construction gives (None: no
# closed form, the real map)
Case = namedtuple("Case", "d max_diff max_size sizes")


def _holes(w, h):
    return np.full((h, w), INVALID, np.float32)


def _serpentine(w, h):
    d = _holes(w, h)
    d[0::2, :] = 3.0
    for y in range(1, h - 1, 2):
        d[y, w - 1 if y % 4 == 1 else 0] = 3.0
    rows, joins = (h + 1) // 2, len(range(1, h - 1, 2))
    return d, rows * w + joins


def _spirals(w, h):
    """two walkers, clockwise from opposite corners, a step each in turn; a cell is taken only if none of its 4-neighbours is
    marked but the one the walker stands on -> (map, length of the first, length of the second)"""
    mark = np.zeros((h, w), np.int32)
    walkers = [dict(x=0, y=0, dx=1, dy=0, n=1, alive=True), dict(x=w - 1, y=h - 1, dx=-1, dy=0, n=1, alive=True)]
    mark[0, 0], mark[h - 1, w - 1] = 1, 2

    def free(k, x, y):
        if not (0 <= x < w and 0 <= y < h) or mark[y, x]:
            return False
        for ax, ay in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
            if 0 <= ax < w and 0 <= ay < h and mark[ay, ax] and (ax, ay) != (k["x"], k["y"]):
                return False
        return True

    while any(k["alive"] for k in walkers):
        for i, k in enumerate(walkers):
            if not k["alive"]:
                continue
            if not free(k, k["x"] + k["dx"], k["y"] + k["dy"]):
                k["dx"], k["dy"] = -k["dy"], k["dx"]           # turn right (y grows downwards)
                if not free(k, k["x"] + k["dx"], k["y"] + k["dy"]):
                    k["alive"] = False
                    continue
            k["x"] += k["dx"]
            k["y"] += k["dy"]
            mark[k["y"], k["x"]] = i + 1
            k["n"] += 1
    d = _holes(w, h)
    d[mark > 0] = 7.0
    return d, walkers[0]["n"], walkers[1]["n"]


def _ramp(w, h, at, step):
    """0.5 per pixel down to 0 at column at - 1, then `step`, then 1.0 and 0.5 per pixel up: every difference but the one
    between columns at - 1 and at is exactly 0.5 or, behind `step`, a little less"""
    row = np.zeros(w, np.float32)
    for x in range(at):
        row[x] = 0.5 * (at - 1 - x)
    row[at] = step
    for x in range(at + 1, w):
        row[x] = 1.0 + 0.5 * (x - at - 1)
    return np.tile(row, (h, 1))


def _blobs():
    d = _holes(100, 40)
    for k, n in enumerate((MAX_SPECKLE - 1, MAX_SPECKLE, MAX_SPECKLE + 1)):
        d[3 + 3 * k, 58:58 + n] = 4.0 + k          # astride x = 64
        d[10:10 + n, 10 + 3 * k] = 9.0             # astride y = 16
    return d


def _median_mix(w, h, seed):
    rng = np.random.RandomState(seed)
    values = np.array([0.0, -0.0, 1.0, 1.0, 1.5, -2.25, 3.0, 3.0, 17.5, np.inf, -np.inf, 1e-40, -1e-40], np.float32)
    d = values[rng.randint(0, len(values), size=(h, w))]
    d[rng.rand(h, w) < 0.004] = FOREIGN_NAN
    share = np.linspace(0.97, 0.0, w)[None, :]      # of holes
    d[rng.rand(h, w) < share] = INVALID
    d[0, 0] = d[0, w - 1] = d[h - 1, 0] = d[h - 1, w - 1] = 1.0
    return d


def _build():
    c = {}
    c["constant"] = Case(np.full((40, 150), 5.0, np.float32), 1.0, MAX_SPECKLE, [150 * 40])
    d = _holes(131, 35)
    yy, xx = np.mgrid[0:35, 0:131]
    d[(xx + yy) % 2 == 0] = 2.0
    c["checker_holes"] = Case(d, 1.0, MAX_SPECKLE, [1] * ((131 * 35 + 1) // 2))
    d = np.where((xx + yy) % 2 == 0, np.float32(1.0), np.float32(10.0)).astype(np.float32)
    c["checker_values"] = Case(d, 1.0, 0, [1] * (131 * 35))
    d, n = _serpentine(200, 67)
    c["serpentine"] = Case(d, 0.25, MAX_SPECKLE, [n])
    d, n = _serpentine(150, 67)
    c["serpentine_t"] = Case(np.ascontiguousarray(d.T), 0.25, MAX_SPECKLE, [n])
    d = _holes(140, 37)
    d[:, 0::2] = 6.0
    d[36, :] = 6.0
    c["comb_bottom"] = Case(d, 1.0, MAX_SPECKLE, [70 * 36 + 140])
    c["comb_top"] = Case(np.ascontiguousarray(d[::-1]), 1.0, MAX_SPECKLE, [70 * 36 + 140])
    d, na, nb = _spirals(70, 40)
    c["spirals"] = Case(d, 1.0, MAX_SPECKLE, sorted([na, nb]))
    above = np.nextafter(np.float32(0.5), np.float32(1.0))
    c["ramp"] = Case(_ramp(150, 3, 64, np.float32(0.5)), 0.5, MAX_SPECKLE, [450])
    c["ramp_step_seam"] = Case(_ramp(150, 3, 64, above), 0.5, MAX_SPECKLE, sorted([64 * 3, 86 * 3]))
    c["ramp_step_inside"] = Case(_ramp(150, 3, 75, above), 0.5, MAX_SPECKLE, sorted([75 * 3, 75 * 3]))
    d = _holes(100, 30)
    d[8:16, 48:64] = 1.0
    d[16:24, 64:80] = 1.0
    c["corner_diagonal"] = Case(d, 1.0, MAX_SPECKLE, [128, 128])
    c["blobs"] = Case(_blobs(), 0.5, MAX_SPECKLE, sorted(2 * [MAX_SPECKLE - 1, MAX_SPECKLE, MAX_SPECKLE + 1]))
    c["column"] = Case(np.full((37, 1), 2.0, np.float32), 1.0, MAX_SPECKLE, [37])
    c["row"] = Case(np.full((1, 131), 2.0, np.float32), 1.0, MAX_SPECKLE, [131])
    c["one_pixel"] = Case(np.full((1, 1), 2.0, np.float32), 1.0, 1, [1])
    c["all_invalid"] = Case(_holes(70, 20), 1.0, MAX_SPECKLE, [])
    d = np.zeros((18, 66), np.float32)
    d[(np.mgrid[0:18, 0:66][0] + np.mgrid[0:18, 0:66][1]) % 2 == 1] = -0.0
    d[:, 33:] = 1.0
    d[9, 50] = np.nextafter(np.float32(1.0), np.float32(2.0))
    c["max_diff_zero"] = Case(d, 0.0, MAX_SPECKLE, sorted([33 * 18, 33 * 18 - 1, 1]))
    rng = np.random.RandomState(7)
    d = (rng.rand(20, 70) * 200.0 - 100.0).astype(np.float32)
    d[5, 10] = d[5, 11] = np.inf
    d[7, 30] = FOREIGN_NAN
    d[9, 40] = INVALID
    c["infinite_diff"] = Case(d, np.inf, MAX_SPECKLE, sorted([70 * 20 - 2, 1]))
    d = _holes(70, 20)
    d[5, 63] = d[5, 64] = np.inf
    c["infinities_alone"] = Case(d, np.inf, 1, [1, 1])
    d = np.full((20, 70), 2.0, np.float32)
    d[5, 10] = d[5, 11] = np.inf
    d[7, 30] = FOREIGN_NAN
    d[9, 40] = INVALID
    c["infinite_values"] = Case(d, 1.0, MAX_SPECKLE, sorted([70 * 20 - 4, 1, 1, 1]))
    c["median_mix"] = Case(_median_mix(150, 40, 3), 0.0, 3, None)
    d = _holes(9, 9)
    d[4, 4] = -3.5
    c["lonely"] = Case(d, 1.0, 0, [1])
    d = np.arange(81, dtype=np.float32).reshape(9, 9)
    d[4, 4] = INVALID
    c["hole"] = Case(d, 100.0, MAX_SPECKLE, [80])
    return c


CASES = _build()

# the real map: block matching of the stereo_cases scene without the left-right check, salt on the right image
REAL_BASE, REAL_SALT_SHARE, REAL_SEED = "base_r4", 0.04, 21
REAL_MAX_DIFF, REAL_MAX_SIZE = 1.0, 30

_REAL = {}


def noisy_pair():
    import stereo_cases as SC
    case = SC.CASES[REAL_BASE]
    left, right = SC.scene(case)
    right = right.copy()
    rng = np.random.RandomState(REAL_SEED)
    right[rng.rand(*right.shape) < REAL_SALT_SHARE] = 255
    return case, left, right


def noisy_real():
    """-> (disparity float32 (h, w), cost uint32 (h, w)) of the noisy pair by the numpy reference of dense stereo; computed once"""
    if "maps" not in _REAL:
        import stereo_ref as R
        case, left, right = noisy_pair()
        ref = R.disparity_ref(left, right, case.r, case.dmin, case.D, case.max_cost, -1, case.subpixel)
        _REAL["maps"] = (np.ascontiguousarray(ref["disparity"], np.float32), np.ascontiguousarray(ref["cost"]).astype(np.uint32))
    return _REAL["maps"]


def case(name):
    if name == "noisy_real":
        return Case(np.ascontiguousarray(noisy_real()[0], np.float32), REAL_MAX_DIFF, REAL_MAX_SIZE, None)
    return CASES[name]


NAMES = list(CASES) + ["noisy_real"]

_REF = {}


def reference(name):
    """-> dict(labels, sizes, speckles, median1, median2) of one case by tests/speckle_ref.py; computed once, never modified"""
    import speckle_ref as R
    if name not in _REF:
        k = case(name)
        labels, sizes = R.components_ref(k.d, k.max_diff)
        _REF[name] = dict(labels=labels, sizes=sizes, speckles=R.speckles_ref(k.d, None, k.max_diff, k.max_size)[0],
                          median1=R.median_ref(k.d, 1), median2=R.median_ref(k.d, 2))
    return _REF[name]
