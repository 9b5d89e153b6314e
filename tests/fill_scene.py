"""The synthetic rectified pair of the hole-filling tests: a textured background at disparity D0 and a textured foreground square
at D1 > D0, integer shifts, 96 x 72.  A left pixel (x, y) of disparity d is seen at (x - d, y) in the right view.  Left of the
square lies the band of background the right view cannot see -- the square hides it there -- which the left-right check
(tolerance 0) turns into holes.  Shared by tests/test_fill_cases.py (reference only) and tests/test_gpu_fill.py."""
import numpy as np

W, H = 96, 72
D0, D1 = 4, 11
RADIUS, DMIN, NUM = 2, 0, 16
SQUARE = (40, 24, 28, 26)      # x, y, w, h in the left view
ARGS = dict(radius=RADIUS, min_disparity=DMIN, num_disparities=NUM, lr_tolerance=0, subpixel=False)
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)
_cache = {}


def pair():
    """-> (left, right) uint8 (H, W)"""
    if "pair" not in _cache:
        rng = np.random.default_rng(77)
        back = rng.integers(0, 256, (H, W + D1 + D0), dtype=np.uint8)     # the background in right-view coordinates, wide enough
        front = rng.integers(0, 256, (SQUARE[3], SQUARE[2]), dtype=np.uint8)
        sx, sy, sw, sh = SQUARE
        left = back[:, D0:D0 + W].copy()
        right = back[:, 2 * D0:2 * D0 + W].copy()                         # left(x) = back(x + D0) = right(x - D0)
        left[sy:sy + sh, sx:sx + sw] = front
        right[sy:sy + sh, sx - D1:sx - D1 + sw] = front
        left.setflags(write=False)
        right.setflags(write=False)
        _cache["pair"] = (left, right)
    return _cache["pair"]


def reference_disparity():
    """stereo_ref's block-matching map of the pair under ARGS, read-only"""
    if "disp" not in _cache:
        import stereo_ref
        left, right = pair()
        d = stereo_ref.disparity_ref(left, right, RADIUS, DMIN, NUM, lr=0, subpixel=0)["disparity"].copy()
        d.setflags(write=False)
        _cache["disp"] = d
    return _cache["disp"]


def occlusion_band():
    """the background pixels of the left view whose right-view position the square covers: D1 - D0 columns left of the square"""
    sx, sy, sw, sh = SQUARE
    band = np.zeros((H, W), bool)
    band[sy:sy + sh, sx - (D1 - D0):sx] = True
    return band
