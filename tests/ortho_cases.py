"""The ortho-image cases: height maps, frames, cameras and parameters for ssrlcv_hip_dsm_ortho.  Shared by
tests/test_ortho_cases.py (which proves on the numpy reference alone that every case exercises what it claims) and
tests/test_gpu_ortho.py (which holds the kernel to that reference).  Every reference result is computed once, shared and never
modified."""
import math
from collections import namedtuple

import numpy as np

import helpers as H
import dsm_cases as DC
import dsm_ref as D
import ortho_ref as R

f32 = np.float32
INF = float("inf")
CELL = 0.5
CAMERA_HEIGHT = 60.0
SPECIALS = np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7FFFFFFF, 0xFFC00000], np.uint32)   # +-inf, +-0, two other NaNs

Case = namedtuple("Case", "height frame views max_steps bias rule occlusion")   # occlusion: the case claims occluded and visible cells


def relief(w, h, seed, salted=False):
    """low noise, a tower 6 high, a wall 3 high and 5 % holes; salted: a few infinities, zeros of both signs and NaNs that are values"""
    rng = np.random.RandomState(seed)
    z = (rng.rand(h, w) * 0.2).astype(np.float32)
    if w >= 40 and h >= 30:
        z[h // 2 - 2:h // 2 + 3, w // 2 - 2:w // 2 + 3] = 6.0
        z[h // 8:h - h // 8, w // 5:w // 5 + 2] = 3.0
    b = D.bits(z).copy()
    b[rng.rand(h, w) < 0.05] = D.INVALID_BITS
    if salted:
        salt = rng.rand(h, w) < 0.02
        b[salt] = SPECIALS[rng.randint(0, len(SPECIALS), int(salt.sum()))]
    return b.view(np.float32)


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)


IMAGES = {"96x96": image(96, 96, 1), "70x50": image(70, 50, 2)}


def camera(pos, forward, size, fov, right=(1.0, 0.0, 0.0)):
    """one Image::Camera record at `pos` looking along `forward`, image x towards `right`"""
    import scene as S   # tools/, on the path through dsm_cases
    a3 = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    a1 = np.asarray(right, np.float64) - np.dot(right, a3) * a3
    a1 /= np.linalg.norm(a1)
    cam = np.zeros(1, H.CAMERA)
    cam["cam_pos"][0] = pos
    cam["cam_rot"][0] = S._rotation_to_euler(np.stack([a1, np.cross(a3, a1), a3], 1)).astype(np.float32)
    cam["fov"][0] = fov
    cam["foc"][0] = 0.16
    cam["dpix"][0] = 1.0           # not what the view is made from
    cam["ecef_offset"][0] = (1e6, 2e6, 3e6)   # nor is this
    cam["size"][0] = size
    return cam[0]


def view_of(cam, fr, img):
    """the reference's view of a camera record: ortho_ref.view_of_camera rounded to float32, as the host builder rounds it"""
    assert img.shape == (int(cam["size"][1]), int(cam["size"][0]))
    M, pos, eye = R.view_of_camera(cam, fr)
    return R.view(img, M, pos, eye)


def cameras(fr):
    """the cameras over the grid of an axis frame -> dict name -> (Image::Camera record, image)"""
    cx, cy = fr.w * float(fr.cell) / 2.0, fr.h * float(fr.cell) / 2.0
    reach = max(cx, cy)
    centre = np.array([cx, cy, 0.0])
    wide = 2.0 * math.atan(1.3 * reach / CAMERA_HEIGHT)   # the whole grid with a margin, seen from above
    big, small = IMAGES["96x96"], IMAGES["70x50"]
    c = {}

    def aimed(pos, img, fov=wide):
        return camera(pos, centre - pos, (img.shape[1], img.shape[0]), fov), img

    c["nadir"] = aimed(centre + (0.0, 0.0, CAMERA_HEIGHT), big)
    c["oblique30"] = aimed(centre + (CAMERA_HEIGHT * math.tan(math.radians(30)), 0.0, CAMERA_HEIGHT), big)
    c["oblique45"] = aimed(centre + (0.0, -CAMERA_HEIGHT, CAMERA_HEIGHT), small, 2.0 * math.atan(1.1 * reach / CAMERA_HEIGHT))
    # eye = (w + 33.5, h + 13.5): du = w + 33 - i and dv = h + 13 - j are integers, equal along the diagonals i - j = w - h + 20
    c["diagonal"] = aimed(np.array([(fr.w + 33.5) * CELL, (fr.h + 13.5) * CELL, CAMERA_HEIGHT]), big, 1.2 * wide)
    # 2 above the plane, inside the grid: L < 1 beneath it, fs > L ends the marches around it
    low = np.array([cx * 0.62 + 0.1, cy * 0.55 + 0.2, 2.0])
    c["low"] = camera(low, (0.0, 0.0, -1.0), (96, 96), 2.6), big
    c["below"] = camera(centre + (0.0, 0.0, -CAMERA_HEIGHT), (0.0, 0.0, 1.0), (96, 96), wide), big            # looks up at the grid from below
    c["away"] = camera(centre + (0.0, 0.0, CAMERA_HEIGHT), (0.0, 0.0, 1.0), (96, 96), wide), big              # above it, looking up: W <= 0
    c["grazing"] = aimed(centre + (200.0, 0.0, 12.0), big, 2.0 * math.atan(1.3 * reach / 200.0))   # the line of sight rises 0.03 a cell
    c["partial"] = aimed(centre + (reach / 3, 0.0, CAMERA_HEIGHT), small, wide / 3)
    return c


def _cases():
    c = {}
    fr = DC.axis_frame(67, 41, cell=CELL)
    z = relief(67, 41, 11)
    cams = cameras(fr)
    v = {name: view_of(cam, fr, img) for name, (cam, img) in cams.items()}
    for name in sorted(v):
        c["67x41/%s" % name] = Case(z, fr, [v[name]], 256, 0.05, R.FIRST, name in ("oblique30", "oblique45", "diagonal", "low"))
    for steps in (0, 1, 7, 256):
        c["67x41/steps%d" % steps] = Case(z, fr, [v["oblique45"]], steps, 0.0, R.FIRST, steps == 256)
    for bias in (0.0, 0.05, INF):
        c["67x41/bias%s" % bias] = Case(z, fr, [v["oblique30"]], 256, bias, R.FIRST, bias != INF)
    for bias in (0.0, 0.05):   # grazing rays: the noise itself hides cells, fewer of them with a bias
        c["67x41/grazing/bias%s" % bias] = Case(z, fr, [v["grazing"]], 256, bias, R.FIRST, True)
    three = [v["oblique45"], v["nadir"], v["diagonal"]]
    eight = [v["partial"], v["below"], v["oblique30"], v["nadir"], v["away"], v["oblique30"], v["diagonal"], v["low"]]   # one view twice
    for rule in (R.FIRST, R.MEDIAN):
        c["67x41/m3/rule%d" % rule] = Case(z, fr, three, 256, 0.05, rule, True)
        c["67x41/m8/rule%d" % rule] = Case(z, fr, eight, 256, 0.05, rule, True)
    c["67x41/salted/m3"] = Case(relief(67, 41, 12, salted=True), fr, three, 256, 0.0, R.MEDIAN, False)
    skew = D.frame(cell=CELL, w=67, h=41, **DC.SKEW)   # an affine frame: the march is still the defined result
    c["67x41/skew"] = Case(z, skew, [view_of(cams[n][0], skew, cams[n][1]) for n in ("oblique30", "nadir")], 256, 0.05, R.MEDIAN, False)
    one = DC.axis_frame(1, 1, cell=CELL)
    vone = {name: view_of(cam, one, img) for name, (cam, img) in cameras(one).items()}
    c["1x1/m1"] = Case(np.full((1, 1), 0.25, np.float32), one, [vone["nadir"]], 256, 0.0, R.FIRST, False)
    c["1x1/m3"] = Case(np.full((1, 1), 0.25, np.float32), one, [vone["away"], vone["oblique30"], vone["nadir"]], 7, 0.05, R.MEDIAN, False)
    c["1x1/hole"] = Case(D.INVALID_BITS.reshape(1, 1).view(np.float32), one, [vone["nadir"]], 7, 0.05, R.FIRST, False)
    big = DC.axis_frame(257, 131, cell=CELL)
    vbig = {name: view_of(cam, big, img) for name, (cam, img) in cameras(big).items()}
    for rule in (R.FIRST, R.MEDIAN):
        c["257x131/m3/rule%d" % rule] = Case(relief(257, 131, 13), big, [vbig["oblique45"], vbig["oblique30"], vbig["low"]], 256, 0.05, rule, True)
    return c


CASES = _cases()
_REF = {}


def reference(name):
    if name not in _REF:
        c = CASES[name]
        _REF[name] = R.ortho(c.height, c.frame, c.views, c.max_steps, c.bias, c.rule)
    return _REF[name]
