"""Cases of the shift search (include/ssrlcv_hip.h "shift search"), shared by tests/test_shift_cases.py (the restatement against a
plain loop and its properties, no GPU), tests/test_shift_host.py (the host pick and the refusals) and tests/test_gpu_shift.py (the
kernels against the restatement).

  sizes      1 x 1, 1 x 37, 37 x 1: one cell, one row, one column; 63 x 15, 64 x 16, 65 x 17: one cell less than the search
             kernel's tile of 64 x 16, the tile, one more; 130 x 35: three tiles by three
  radii      0 (one shift), 1, 7 (225 shifts: one slot a thread), 32 (4225: seventeen slots, the last one mostly empty); most
             maps are smaller than 2 x 32 + 1, so most entries of the radius-32 tables are zeros
  strides    1, 2, 3, 5: no size is a multiple of all of them
  centres    (0, 0); (5, -3); (1000, 0): nothing overlaps; (2^24, -2^24) and (-2^24, 2^24): the limits
  gate       0 and 1 about a centre inside the differences; 2^18 + 600 about centres of +-2^18, the limits, which passes the
             differences of one sign; NO_GATE
  contents   RELIEF (30 % holes in the moving map, 10 % in the reference), all-invalid maps, CLIP (t = +-65536 exactly, the next
             float outside, 1e30, +-inf, three NaN patterns), WIDE (+-65536 against -+65536: every d = +-131072)
  grid cap   BEYOND_CAPS: more tiles than the search kernel's grid and more cells than one trip of the quantise kernel's,
             both read from csrc/shift.hip
  scene      the rendered scene's truth map shifted by whole cells with a height bias; and its truth cloud displaced by 7.3,
             -4.6, 0.5 cells and register_cases.MOTION_ROTATION about its centroid, with every tenth point raised 20 cells"""
import os
import re

import numpy as np

import shift_ref as R

NAN = np.float32(np.nan)
NO_GATE = R.NO_GATE
SIZES = ((1, 1), (1, 37), (37, 1), (63, 15), (64, 16), (65, 17), (130, 35))
SCALE = 64.0
FAR = (1000, 0)
LIMIT = 1 << 24
LIMIT_Q = 1 << 18

# every size runs all of these; between them the radii 0, 1, 7, 32, the strides 1, 2, 3, 5, the centres and the gates
PARAMS = (
    dict(radius=0),
    dict(radius=1, stride=2),
    dict(radius=7, center=(5, -3)),
    dict(radius=32),
    dict(radius=7, stride=3, center_q=-40, gate_q=0),
    dict(radius=1, stride=5, center_q=25, gate_q=1),
    dict(radius=7, center=(LIMIT, -LIMIT)),
    dict(radius=32, center=(-LIMIT, LIMIT), stride=2),
    dict(radius=32, center=FAR),
    dict(radius=7, center_q=LIMIT_Q, gate_q=LIMIT_Q + 600),
    dict(radius=1, center=(-1, 2), center_q=-LIMIT_Q, gate_q=LIMIT_Q + 600),
    dict(radius=8, center=(-2, 1), gate_q=300),           # 289 shifts: the second slot of one wave only
    dict(radius=5, stride=2, center_q=10, gate_q=150),    # 121 shifts: two groups of threads share the rows of a tile
    dict(radius=3),                                       # 49 shifts: four groups
)


def relief(w, h, seed, holes=0.0):
    """heights of about +-12 (keys of +-800 at SCALE) with a slope, and a share of invalid cells"""
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:h, 0:w]
    a = (3.0 * np.sin(ii * 0.37 + seed) + 2.0 * np.cos(jj * 0.23) + 0.11 * ii - 0.07 * jj + rng.normal(0, 2.5, (h, w))).astype(np.float32)
    a[rng.random((h, w)) < holes] = NAN
    return a


def pair(w, h):
    """-> (moving, reference): the same relief, moving(x, y) showing reference(x + 2, y - 1), raised by 0.4 and noisy"""
    big = relief(w + 8, h + 8, 7 * w + h)
    rng = np.random.default_rng(w * 1000 + h)
    moving = (big[3:3 + h, 6:6 + w] + np.float32(0.4) + rng.normal(0, 0.05, (h, w)).astype(np.float32)).astype(np.float32)
    reference = big[4:4 + h, 4:4 + w].copy()
    moving[rng.random((h, w)) < 0.3] = NAN
    reference[rng.random((h, w)) < 0.1] = NAN
    return moving, reference


def clip_map(w=65, h=17):
    """SCALE = 64: 1024 gives t = 65536 exactly"""
    a = relief(w, h, 3)
    edge = np.float32(1024.0)
    specials = [edge, -edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(-edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(0)),
                np.float32(1e30), np.float32(-1e30), np.float32(np.inf), np.float32(-np.inf), np.float32(3.4e38),
                np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)]
    flat = np.concatenate([np.atleast_1d(s) for s in specials]).astype(np.float32)
    a.reshape(-1)[5:5 + 3 * len(flat):3] = flat
    return a


CLIPPED_IN_CLIP_MAP = 5       # the two next floats outside, +-1e30 and 3.4e38; the infinities and the NaNs are invalid, not clipped
INVALID_IN_CLIP_MAP = 11      # those five, the two infinities and the four NaNs


def wide_pair(n=512):
    """scale 1: every cell of the moving map is +65536 and every cell of the reference -65536, so every d is +131072: at shift 0,
    n = 2^18, sum = 2^35 and sumSq = 2^52.  Swapped, every d is -131072.  A 32-bit sum that is not flushed in time fails both"""
    moving = np.full((n, n), 65536.0, np.float32)
    reference = np.full((n, n), -65536.0, np.float32)
    return moving, reference


def contents():
    """name -> (moving, reference, scale, the PARAMS-like dictionaries to run)"""
    out = {}
    m, r = pair(65, 17)
    out["no_moving"] = (np.full_like(m, NAN), r, SCALE, (dict(radius=7), dict(radius=1, stride=2)))
    out["no_reference"] = (m, np.full_like(r, NAN), SCALE, (dict(radius=7), dict(radius=1, stride=2)))
    c = clip_map()
    out["clip_moving"] = (c, relief(65, 17, 4), SCALE, (dict(radius=7), dict(radius=2, center=(1, 1))))
    out["clip_reference"] = (relief(65, 17, 4), c, SCALE, (dict(radius=7),))
    out["clip_both"] = (c, c[::-1].copy(), SCALE, (dict(radius=1),))
    wm, wr = wide_pair()
    out["wide_plus"] = (wm, wr, 1.0, (dict(radius=1),))                     # d = +131072: sum = +2^35 and sumSq = 2^52 at shift 0
    out["wide_minus"] = (wr, wm, 1.0, (dict(radius=1, center_q=-(1 << 17), gate_q=0),))   # d = -131072, gated exactly
    return out


def read_constant(name):
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ssrlcv_amd", "csrc", "shift.hip")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


SEARCH_CAP = read_constant("kSearchGridCap")
QUANTISE_CAP = read_constant("kQuantiseGridCap")
TILE_W, TILE_H = 64, 16


def beyond_caps():
    """-> (moving, reference): 33 tiles wide, and so high that the tiles outnumber the search grid and the cells one trip of the
    quantise grid; neither side a multiple of the tile"""
    w = 33 * TILE_W - 5
    h = max((SEARCH_CAP // 33 + 1) * TILE_H - 3, QUANTISE_CAP * 256 // w + 2)
    rng = np.random.default_rng(11)
    base = rng.integers(-2000, 2000, (h + 2, w + 2)).astype(np.float32) / np.float32(SCALE)
    moving, reference = base[1:1 + h, 0:w].copy(), base[0:h, 1:1 + w].copy()      # the moving map shows the reference at (-1, +1)
    moving[rng.random((h, w)) < 0.3] = NAN
    return moving, reference


# ---- the rendered scene
SCENE_SHIFTS = ((7, -5), (-11, 9), (12, 12))
SCENE_BIAS_CELLS = 0.7
SCENE_RADIUS, SCENE_MIN_OVERLAP = 12, 2304
SCENE_COARSE = ((2, -1), (-3, 2), (3, 3))     # at stride 4, radius 4, overlap 2304 / 16
MOTION_CELLS = (7.3, -4.6, 0.5)               # along ex, ey, ez; the rotation is register_cases.MOTION_ROTATION
# Every tenth point is raised 20 cells, as in register_cases.  With restatement and level loop on the CPU the un-gated search
# (gate=None) still picks (7, -5) at this share and at every larger one tried -- every 7th, 5th, 4th, 3rd and 2nd point --: points
# raised at regular places add the same to the variance of every shift.  What the raised points break without the gate is the
# bias, 1.44 cells high at a tenth, and the registration that starts from it; the share therefore stays at a tenth.
OUTLIER_EVERY, OUTLIER_CELLS = 10, 20.0
_SCENE = {}


def shifted_truth(shift):
    """-> (moving, reference, scale): moving(x, y) = truth(x + sx, y + sy) + 0.7 cell where that cell exists"""
    import accuracy_cases as AC
    import dsm_cases as DC
    truth, cell = AC.truth_map(), float(DC.scene_frame().cell)
    h, w = truth.shape
    sx, sy = shift
    (x0, x1), (y0, y1) = R.window(w, sx), R.window(h, sy)
    moving = np.full_like(truth, NAN)
    moving[y0:y1, x0:x1] = truth[y0 + sy:y1 + sy, x0 + sx:x1 + sx] + np.float32(SCENE_BIAS_CELLS * cell)
    return moving, truth, 64.0 / cell


def truth_points():
    """the cloud of the truth map: its cells as points at their centres (the restatement of ssrlcv_hip_dsm_points)"""
    if "points" not in _SCENE:
        import accuracy_cases as AC
        import dsm_cases as DC
        import dsm_ref as D
        _SCENE["points"] = D.points(AC.truth_map(), DC.scene_frame())
    return _SCENE["points"]


def motion():
    """-> (A, b): the true motion x -> A x + b that takes the displaced cloud back (register_cases.motion with MOTION_CELLS)"""
    import accuracy_cases as AC
    import dsm_cases as DC
    import register_cases as RC
    import register_ref as RR
    fr = DC.scene_frame()
    c = truth_points().astype(np.float64).mean(0)
    A = RR.rotation(RC.MOTION_ROTATION)
    t = float(fr.cell) * (MOTION_CELLS[0] * fr.ex.astype(np.float64) + MOTION_CELLS[1] * fr.ey.astype(np.float64) + MOTION_CELLS[2] * fr.ez.astype(np.float64))
    return A, c - A @ c + t


def displaced(outliers=False):
    """-> (cloud float32 (n, 3), truth float32 (n, 3), keep bool (n,)): truth_points() under the inverse of motion(), every tenth
    point raised 20 cells along ez with `outliers`; keep: the points that are no outliers"""
    if outliers not in _SCENE:
        import accuracy_cases as AC
        import dsm_cases as DC
        fr = DC.scene_frame()
        truth = truth_points()
        A, b = motion()
        cloud = np.linalg.solve(A, (truth.astype(np.float64) - b).T).T
        keep = np.ones(len(truth), bool)
        if outliers:
            keep[::OUTLIER_EVERY] = False
            cloud[~keep] += OUTLIER_CELLS * float(fr.cell) * fr.ez.astype(np.float64)
        _SCENE[outliers] = (cloud.astype(np.float32), truth, keep)
    return _SCENE[outliers]


def displaced_map(outliers=False):
    """the height map of the displaced cloud in the scene's frame (the restatement of the rasterisation, rule max)"""
    key = ("map", outliers)
    if key not in _SCENE:
        import dsm_cases as DC
        import dsm_ref as D
        _SCENE[key] = D.rasterize(displaced(outliers)[0], DC.scene_frame(), D.MAX)[0]
    return _SCENE[key]
