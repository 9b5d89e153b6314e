"""The rectification cases: the warp's case table, the mask's and the records' hand-made inputs, and the scene pair -- views
(0, 2) of tools/scene.py's PinholeRig at 192 px -- with its ground-truth disparities and the reference chain
(warp_ref x 2 -> stereo_ref.disparity_ref -> mask_ref).  Shared by tests/test_rectify_cases.py (which proves on the numpy
reference alone that the cases test something) and tests/test_gpu_rectify.py (which holds the kernels to that reference).
Every reference result is computed once, shared and never modified."""
import os
import sys
from collections import namedtuple

import numpy as np

import helpers as H
import rectify_ref as R

sys.path.insert(0, os.path.join(H.ROOT, "tools"))

f32 = np.float32
NAN, INF = float("nan"), float("inf")

# ---- sources: seeded random bytes, (w, h)
SOURCES = {"1x1": (1, 1), "1x7": (1, 7), "7x1": (7, 1), "2x2": (2, 2), "67x45": (67, 45)}


def source(name):
    w, h = SOURCES[name]
    return np.random.RandomState(1000 + 16 * w + h).randint(0, 256, size=(h, w)).astype(np.uint8)


def _h(*rows):
    return np.array(rows, np.float32).reshape(9)


IDENTITY = _h(1, 0, 0, 0, 1, 0, 0, 0, 1)


def quarter_turn(w):
    """the issue's quarter turn for an output w wide: sx = y, sy = (w - 1) - x"""
    return _h(0, 1, 0, -1, 0, w - 1, 0, 0, 1)


def rig_homographies(w, h, views=(0, 2)):
    """Hl, Hr of the rig's cameras with their size set to w x h (the builder takes the focal length in pixels from size.x)"""
    import scene
    from ssrlcv_amd import capi
    cams = scene.PinholeRig(3, 192).cameras[list(views)].copy()
    cams["size"] = (w, h)
    rect = capi.rectify_cameras(cams[0], cams[1])
    return rect["Hl"].copy(), rect["Hr"].copy()


HOMOGRAPHIES = {
    "identity": lambda: IDENTITY,
    "shift_int": lambda: _h(1, 0, 3, 0, 1, -2, 0, 0, 1),
    "shift_half": lambda: _h(1, 0, 0.5, 0, 1, 0.5, 0, 0, 1),
    "scale_0.37": lambda: _h(0.37, 0, 0, 0, 0.37, 0, 0, 0, 1),
    "scale_4.1": lambda: _h(4.1, 0, 0.3, 0, 4.1, -0.2, 0, 0, 1),
    "rig_Hl": lambda: rig_homographies(67, 45)[0],
    "rig_Hr": lambda: rig_homographies(67, 45)[1],
    "last_column": lambda: _h(1, 0, 2, 0, 1, 0, 0, 0, 1),            # output x = 64 lands exactly on sx = 66 = srcW - 1 of 67 x 45
    "w_changes_sign": lambda: _h(1, 0, 0, 0, 1, 0, -0.05, 0, 1),      # W = 1 - 0.05 x: positive up to x = 19
    "w_zero": lambda: _h(1, 0, 0, 0, 1, 0, -0.125, 0.25, 0.5),        # W = 0.5 - x / 8 + y / 4 is exactly 0 at (4, 0), (6, 1), (8, 2)
    "all_outside": lambda: _h(1, 0, 1000, 0, 1, -1000, 0, 0, 1),      # mapped, clamped: the corner pixel everywhere
    "all_behind": lambda: _h(1, 0, 0, 0, 1, 0, 0, 0, -1),             # W < 0 everywhere: all zero
    "nan_entry": lambda: _h(NAN, 0, 0, 0, 1, 0, 0, 0, 1),
    "nan_w": lambda: _h(1, 0, 0, 0, 1, 0, 0, NAN, 1),
    "inf_entry": lambda: _h(1, 0, INF, 0, 1, 0, 0, 0, 1),
    "minus_inf_entry": lambda: _h(1, 0, 0, 0, -INF, 0, 0, 0, 1),
    "inf_w": lambda: _h(1, 0, 0, 0, 1, 0, 0, 0, INF),
    "1e30_entry": lambda: _h(1e30, 0, 0, 0, 1, 0, 0, 0, 1),          # sx = 1e30 x: finite up to x = 340, clamped
    "1e30_w": lambda: _h(1, 0, 0, 0, 1, 0, 1e30, 1e30, 1),
    "1e30_squared": lambda: _h(1e30, 0, 0, 0, 1, 0, 0, 0, 1e-30),     # X / W overflows: not mapped but at x = 0
    "zoom_out": lambda: _h(0.031, 0.002, 0.4, -0.001, 0.042, 0.3, 1e-5, 2e-5, 1),   # a 2049 x 1025 output over the 67 x 45 source
}

WarpCase = namedtuple("WarpCase", "source hom dw dh")
WIDTHS = (1, 2, 3, 5, 63, 64, 65, 257)   # lane groups of four, a wave's 256 columns, tails, odd row pitches
HEIGHTS = (1, 3)


def _warp_cases():
    cases = {}
    for hom in HOMOGRAPHIES:   # every homography on the 67 x 45 source, past one wave and with an odd pitch
        if hom == "zoom_out":
            continue
        cases["67x45/%s/65x3" % hom] = WarpCase("67x45", hom, 65, 3)
    for dw in WIDTHS:          # every width and height under a homography that is no copy
        for dh in HEIGHTS:
            cases["67x45/rig_Hl/%dx%d" % (dw, dh)] = WarpCase("67x45", "rig_Hl", dw, dh)
    cases["67x45/last_column/257x3"] = WarpCase("67x45", "last_column", 257, 3)
    cases["67x45/w_changes_sign/257x1"] = WarpCase("67x45", "w_changes_sign", 257, 1)
    cases["67x45/1e30_entry/257x3"] = WarpCase("67x45", "1e30_entry", 257, 3)
    cases["67x45/quarter_turn/45x67"] = WarpCase("67x45", "quarter_turn", 45, 67)
    # more lanes than one launch holds (2048 blocks of 256): 514 lanes a row x 1025 rows = 526 850, so the grid-stride loop turns
    cases["67x45/zoom_out/2049x1025"] = WarpCase("67x45", "zoom_out", 2049, 1025)
    for src in ("1x1", "1x7", "7x1", "2x2"):   # the sources with no second column or row
        for hom in ("identity", "shift_half", "scale_0.37", "scale_4.1"):
            cases["%s/%s/5x3" % (src, hom)] = WarpCase(src, hom, 5, 3)
        cases["%s/shift_half/65x1" % src] = WarpCase(src, "shift_half", 65, 1)
    return cases


WARP_CASES = _warp_cases()


def homography(name, dw):
    return quarter_turn(dw) if name == "quarter_turn" else np.asarray(HOMOGRAPHIES[name](), np.float32)


_WARP_REF = {}


def warp_reference(name):
    """-> (source, H, reference output) of one warp case"""
    if name not in _WARP_REF:
        c = WARP_CASES[name]
        src, Hm = source(c.source), homography(c.hom, c.dw)
        _WARP_REF[name] = (src, Hm, R.warp_ref(src, Hm, c.dw, c.dh))
    return _WARP_REF[name]


# ---- the hand-made disparity map of the mask: a 40 x 24 map of a pair "rectified" by two translations of 40 x 24 sources
MASK_R = 2
MASK_SRC = (40, 24)
MASK_HL = _h(1, 0, 1, 0, 1, 0, 0, 0, 1)      # left source column = x + 1: the window of x = 37 reaches column 40, outside
MASK_HR = _h(1, 0, 2, 0, 1, 1, 0, 0, 1)      # right source column = x + 2, row = y + 1


def mask_map():
    """-> (disparity float32 24 x 40, cost uint32): valid pixels with integer and half-pixel disparities, invalid ones, and
    disparities that put a corner of the right box exactly on the source's last column (x - delta + 2.5 + 2 = 39) and half a
    pixel to either side of it"""
    h, w = MASK_SRC[1], MASK_SRC[0]
    rng = np.random.RandomState(7)
    disp = rng.randint(-3, 4, size=(h, w)).astype(np.float32)
    disp[rng.rand(h, w) < 0.3] += f32(0.5)
    disp[rng.rand(h, w) < 0.2] -= f32(0.25)
    bits = H.bits(disp).copy()
    bits[rng.rand(h, w) < 0.25] = R.NAN_BITS
    disp = bits.view(np.float32).copy()
    for x in range(4, 36):     # rows 10, 11, 12: the right box's last corner at 39 exactly, 39.5 (outside), 38.5 (inside)
        disp[10, x] = f32(x) - f32(34.5)
        disp[11, x] = f32(x) - f32(35.0)
        disp[12, x] = f32(x) - f32(34.0)
    cost = rng.randint(0, 5000, size=(h, w)).astype(np.uint32)
    cost[H.bits(disp) == R.NAN_BITS] = R.NO_COST
    return disp, cost


def big_mask_map():
    """-> (disparity float32 513 x 1025, Hl, Hr, (sw, sh)): more pixels (525 825) than one launch of the mask holds lanes
    (2048 blocks of 256), under two homographies with perspective"""
    h, w = 513, 1025
    rng = np.random.RandomState(17)
    disp = (rng.randint(-40, 41, size=(h, w)) * f32(0.25)).astype(np.float32)
    bits = H.bits(disp).copy()
    bits[rng.rand(h, w) < 0.1] = R.NAN_BITS
    Hl = _h(1.01, 0.01, -8, -0.01, 0.99, 4, 1e-6, -2e-6, 1)
    Hr = _h(0.99, -0.01, 6, 0.01, 1.01, -5, -2e-6, 1e-6, 1)
    return bits.view(np.float32).copy(), Hl, Hr, (w, h)


# ---- the records of the apply test
APPLY_H0 = _h(0.9, 0.1, 3, -0.1, 0.9, 2, 1e-3, 0, 1)
APPLY_H1 = _h(1, 0, 0, 0, 1, 0, -0.01, 0, 1)   # W = 1 - x / 100: a point at x >= 100 does not map


def apply_records(n=300):
    """Match records with 0xA5 in every padding byte: live ones, already-invalid ones, and ones whose second point has W <= 0"""
    rng = np.random.RandomState(11)
    raw = np.full(n * 40, 0xA5, np.uint8)
    m = raw.view(H.MATCH)
    m["invalid"] = (rng.rand(n) < 0.2).astype(np.uint8)
    m["invalid"][3] = 7   # any non-zero byte is invalid
    m["kp0_parent"], m["kp1_parent"] = 4, 9
    m["kp0_loc"] = (rng.rand(n, 2) * 150).astype(np.float32)
    m["kp1_loc"] = (rng.rand(n, 2) * 150).astype(np.float32)
    m["kp1_loc"][5] = (100.0, 3.0)   # W = 0 exactly
    m["invalid"][5] = 0
    return m


# ---- the scene pair
Chain = namedtuple("Chain", "size views r lr subpixel min_valid min_within_half max_error")
# floors, and beside them what the reference gave when the case was written (tests/test_rectify_cases.py prints them):
#   valid after the mask       >= 30 000      measured 32 982 of 36 864 (the mask removed 868)
#   within 0.5 px of the truth >= 99 %        measured 99.87 %
#   largest error              <= 1.5 px      measured below 1.0
CHAIN = Chain(192, (0, 2), 4, 1, 1, 30000, 0.99, 1.5)

_SCENE = {}


def scene_pair():
    """-> dict: left, right (uint8 numpy, rendered on the CPU whatever the machine), cams (the two Image::Camera records), rig,
    scene, rect (the library's host builder)"""
    if not _SCENE:
        import torch
        import scene
        from ssrlcv_amd import capi
        rig = scene.PinholeRig(3, CHAIN.size)
        sc = scene.Scene(CHAIN.size, rig.gsd, torch.device("cpu"))
        a, b = CHAIN.views
        cams = rig.cameras[[a, b]].copy()
        _SCENE.update(left=rig.render(sc, a).numpy(), right=rig.render(sc, b).numpy(), cams=cams, rig=rig, scene=sc,
                      rect=capi.rectify_cameras(cams[0], cams[1]))
    return _SCENE


def project(cam, M, pts):
    """float64 pixel coordinates and depth of world points (n, 3) in a pinhole camera: the inverse of generateBundle's ray"""
    f = float(cam["size"][0]) / 2.0 / np.tan(float(cam["fov"][0]) / 2.0)
    p = (pts - cam["cam_pos"].astype(np.float64)) @ M
    return f * p[:, 0] / p[:, 2] + cam["size"][0] / 2.0, f * p[:, 1] / p[:, 2] + cam["size"][1] / 2.0, p[:, 2]


def eval64(Hm, x, y):
    """a float32 homography evaluated in float64"""
    h = np.asarray(Hm, np.float64).reshape(9)
    W = h[6] * x + h[7] * y + h[8]
    return (h[0] * x + h[1] * y + h[2]) / W, (h[3] * x + h[4] * y + h[5]) / W


_TRUTH = {}


def truth():
    """-> dict: disparity (float64 h x w: the true disparity of every rectified-left pixel, rectified-left pixel -> Hl ->
    rig.ground_points -> right camera -> Gr), ground (h x w x 3 world points), seen (the pixel's source point lies inside the
    left image), dmin, D (the disparity range floor(min) - 2 .. ceil(max) + 2 over the seen pixels)"""
    if not _TRUTH:
        import torch
        s = scene_pair()
        n = CHAIN.size
        rect, rig = s["rect"], s["rig"]
        ys, xs = np.mgrid[0:n, 0:n].astype(np.float64)
        sx, sy = eval64(rect["Hl"], xs.ravel(), ys.ravel())
        seen = (sx >= 0) & (sx <= n - 1) & (sy >= 0) & (sy <= n - 1)
        ground = rig.ground_points(s["scene"], CHAIN.views[0], torch.from_numpy(sx), torch.from_numpy(sy))[0].numpy()
        u, v, _ = project(s["cams"][1], rig.M[CHAIN.views[1]], ground)
        xr, _ = eval64(rect["Gr"], u, v)
        d = xs.ravel() - xr
        lo, hi = int(np.floor(d[seen].min())) - 2, int(np.ceil(d[seen].max())) + 2
        _TRUTH.update(disparity=d.reshape(n, n), ground=ground.reshape(n, n, 3), seen=seen.reshape(n, n), dmin=lo, D=hi - lo + 1,
                      true_range=(float(d[seen].min()), float(d[seen].max())))
    return _TRUTH


_CHAIN_REF = {}


def chain_reference():
    """-> dict: left_r, right_r (warp_ref), stereo (stereo_ref.disparity_ref's dict), disparity, cost (after mask_ref)"""
    if not _CHAIN_REF:
        import stereo_ref as S
        s, t = scene_pair(), truth()
        n = CHAIN.size
        left_r = R.warp_ref(s["left"], s["rect"]["Hl"], n, n)
        right_r = R.warp_ref(s["right"], s["rect"]["Hr"], n, n)
        st = S.disparity_ref(left_r, right_r, CHAIN.r, t["dmin"], t["D"], lr=CHAIN.lr, subpixel=CHAIN.subpixel)
        disp, cost = R.mask_ref(st["disparity"], st["cost"], CHAIN.r, s["rect"]["Hl"], s["rect"]["Hr"], n, n)
        _CHAIN_REF.update(left_r=left_r, right_r=right_r, stereo=st, disparity=disp, cost=cost)
    return _CHAIN_REF
