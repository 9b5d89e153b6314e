"""The rectification contract of include/ssrlcv_hip.h ("rectification") restated in numpy float32, operation by operation: the
evaluation of a homography, the bilinear warp, the mask over a disparity map and the way back for Match records.  It shares no
code with csrc/rectify.hip.  numpy rounds every float32 product and sum on its own and contracts nothing, which is the
contract's arithmetic, so the GPU results are compared bit for bit."""
import numpy as np

import helpers as H

NAN_BITS = np.uint32(0x7FC00000)
NO_COST = np.uint32(0xFFFFFFFF)
f32 = np.float32


def eval_h(Hm, x, y):
    """-> (sx, sy, mapped) of the float32 points (x, y) under the 9 float32 entries Hm"""
    h = np.asarray(Hm, f32).reshape(9)
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    with np.errstate(all="ignore"):
        X = (h[0] * x + h[1] * y) + h[2]
        Y = (h[3] * x + h[4] * y) + h[5]
        W = (h[6] * x + h[7] * y) + h[8]
        sx = X / W
        sy = Y / W
    assert sx.dtype == np.float32 and W.dtype == np.float32
    mapped = (W > 0) & np.isfinite(sx) & np.isfinite(sy)
    return sx, sy, mapped


def inside(Hm, x, y, sw, sh):
    sx, sy, mapped = eval_h(Hm, x, y)
    with np.errstate(invalid="ignore"):
        return mapped & (sx >= 0) & (sx <= f32(sw - 1)) & (sy >= 0) & (sy <= f32(sh - 1))


def warp_ref(src, Hm, dw, dh):
    """uint8 (sh, sw) -> uint8 (dh, dw)"""
    sh, sw = src.shape
    ys, xs = np.mgrid[0:dh, 0:dw]
    sx, sy, mapped = eval_h(Hm, xs.astype(f32), ys.astype(f32))
    sx = np.where(mapped, sx, f32(0))
    sy = np.where(mapped, sy, f32(0))
    sx = np.minimum(np.maximum(sx, f32(0)), f32(sw - 1))
    sy = np.minimum(np.maximum(sy, f32(0)), f32(sh - 1))
    x0 = np.minimum(np.floor(sx).astype(np.int64), max(sw - 2, 0))
    y0 = np.minimum(np.floor(sy).astype(np.int64), max(sh - 2, 0))
    x1 = np.minimum(x0 + 1, sw - 1)
    y1 = np.minimum(y0 + 1, sh - 1)
    fx = sx - x0.astype(f32)
    fy = sy - y0.astype(f32)
    assert np.array_equal(fx.astype(np.float64), sx.astype(np.float64) - x0) and (fx >= 0).all() and (fx <= 1).all()   # exact
    assert np.array_equal(fy.astype(np.float64), sy.astype(np.float64) - y0) and (fy >= 0).all() and (fy <= 1).all()
    S = src.astype(f32)
    a, b, c, d = S[y0, x0], S[y0, x1], S[y1, x0], S[y1, x1]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    v = top + fy * (bot - top)
    assert v.dtype == np.float32 and (v >= 0).all() and (v <= 255).all()
    out = np.floor(v + f32(0.5)).astype(np.uint8)
    out[~mapped] = 0
    return out


def mask_ref(disparity, cost, r, Hl, Hr, sw, sh):
    """-> (disparity, cost or None) after ssrlcv_hip_stereo_mask_rectified; the inputs are not modified"""
    h, w = disparity.shape
    bits = H.bits(disparity).copy()
    valid = bits != NAN_BITS
    ys, xs = np.mgrid[0:h, 0:w]
    xm, xp = (xs - r).astype(f32), (xs + r).astype(f32)
    ym, yp = (ys - r).astype(f32), (ys + r).astype(f32)
    keep = inside(Hl, xm, ym, sw, sh) & inside(Hl, xp, ym, sw, sh) & inside(Hl, xm, yp, sw, sh) & inside(Hl, xp, yp, sw, sh)
    delta = np.where(valid, disparity, f32(0)).astype(f32)
    xr = xs.astype(f32) - delta
    half = f32(r) + f32(0.5)
    um, up = xr - half, xr + half
    keep &= inside(Hr, um, ym, sw, sh) & inside(Hr, up, ym, sw, sh) & inside(Hr, um, yp, sw, sh) & inside(Hr, up, yp, sw, sh)
    drop = valid & ~keep
    bits[drop] = NAN_BITS
    out_cost = None
    if cost is not None:
        out_cost = cost.copy()
        out_cost[drop] = NO_COST
    return bits.view(np.float32), out_cost


def apply_ref(matches, H0, H1):
    """-> the records after ssrlcv_hip_matches_apply_homography (a copy: padding bytes and parents as they were)"""
    out = np.ascontiguousarray(matches).view(np.uint8).copy().view(H.MATCH)   # the raw bytes: a field-wise copy drops padding
    live = matches["invalid"] == 0
    ok = np.ones(len(matches), bool)
    new = {}
    for k, Hm in ((0, H0), (1, H1)):
        if Hm is None:
            continue
        loc = matches["kp%d_loc" % k]
        sx, sy, mapped = eval_h(Hm, loc[:, 0], loc[:, 1])
        ok &= mapped
        new[k] = np.stack([sx, sy], 1)
    for k, v in new.items():
        sel = live & ok
        out["kp%d_loc" % k][sel] = v[sel]
    out["invalid"][live & ~ok] = 1
    return out
