"""The dense-stereo contract of include/ssrlcv_hip.h ("dense stereo") restated in numpy, item by item.  It shares no code
with csrc/stereo.hip: the costs come from an integral image of the absolute differences, one disparity at a time, into a cost
volume; step 5 and the points are float32 arithmetic.  Everything here is exact, so the GPU results are compared bit for bit."""
import numpy as np

import helpers as H

NAN_BITS = np.uint32(0x7FC00000)
NO_COST = np.uint32(0xFFFFFFFF)
BIG = np.int64(1) << 40  # "not a candidate" inside the volume


def cost_volume(left, right, r, dmin, D):
    """C[k, y, x] (int64) = item 1's cost at d = dmin + k, BIG where it is not defined"""
    h, w = left.shape
    C = np.full((D, h, w), BIG, np.int64)
    if w < 2 * r + 1 or h < 2 * r + 1:
        return C
    L, R = left.astype(np.int64), right.astype(np.int64)
    for k in range(D):
        d = dmin + k
        x0, x1 = max(r, r + d), min(w - 1 - r, w - 1 - r + d)  # centres whose two windows are inside
        if x0 > x1:
            continue
        ad = np.zeros((h, w), np.int64)
        a, b = x0 - r, x1 + r + 1  # the columns those windows cover
        ad[:, a:b] = np.abs(L[:, a:b] - R[:, a - d:b - d])
        I = np.zeros((h + 1, w + 1), np.int64)
        I[1:, 1:] = ad.cumsum(0).cumsum(1)
        ys = np.arange(r, h - r)[:, None]
        xs = np.arange(x0, x1 + 1)[None, :]
        C[k, r:h - r, x0:x1 + 1] = I[ys + r + 1, xs + r + 1] - I[ys - r, xs + r + 1] - I[ys + r + 1, xs - r] + I[ys - r, xs - r]
    return C


def right_volume(C, dmin):
    """CR[k, y, x'] = C[k, y, x' + d]: the costs the right winner of x' chooses from (item 4)"""
    D, h, w = C.shape
    CR = np.full_like(C, BIG)
    for k in range(D):
        d = dmin + k
        lo, hi = max(0, -d), min(w, w - d)  # x' with 0 <= x' + d < w
        if lo < hi:
            CR[k, :, lo:hi] = C[k, :, lo + d:hi + d]
    return CR


def disparity_ref(left, right, r, dmin, D, max_cost=0xFFFFFFFF, lr=-1, subpixel=0):
    """-> dict: disparity (float32 h x w), cost (uint32), plus what tests/test_stereo_cases.py looks at: k (int winners, -1
    none), valid_before_lr, tied (the minimum is reached by more than one candidate), off (float32 offsets)"""
    h, w = left.shape
    C = cost_volume(left, right, r, dmin, D)
    k = C.argmin(0)                      # first occurrence: the smallest d among equal costs
    cbest = C.min(0)
    has = cbest < BIG
    tied = has & ((C == cbest[None]).sum(0) > 1)
    valid = has & (cbest <= max_cost)    # item 3
    before_lr = valid.copy()
    if lr >= 0:                          # item 4
        CR = right_volume(C, dmin)
        kR = CR.argmin(0)
        ys, xs = np.nonzero(valid)
        xr = xs - (dmin + k[ys, xs])
        assert (CR.min(0)[ys, xr] < BIG).all()  # dR(x - d*, y) has at least the candidate d*
        keep = np.abs(kR[ys, xr] - k[ys, xs]) <= lr
        valid[ys[~keep], xs[~keep]] = False
    off = np.zeros((h, w), np.float32)
    if subpixel:                         # item 5
        ys, xs = np.nonzero(has & (k >= 1) & (k <= D - 2))
        kk = k[ys, xs]
        cm, c0, cp = C[kk - 1, ys, xs], C[kk, ys, xs], C[kk + 1, ys, xs]
        ok = (cm < BIG) & (cp < BIG)
        den = cm - 2 * c0 + cp
        ok &= den != 0
        num32 = (cm - cp)[ok].astype(np.float32)
        den32 = (2 * den)[ok].astype(np.float32)
        off[ys[ok], xs[ok]] = num32 / den32
    disp = (dmin + k).astype(np.float32) + off
    disp_bits = np.where(valid, disp.view(np.uint32), NAN_BITS).astype(np.uint32)
    cost = np.where(valid, cbest, np.int64(NO_COST)).astype(np.uint32)
    return dict(disparity=disp_bits.view(np.float32), cost=cost, k=np.where(has, k, -1), valid=valid, valid_before_lr=before_lr,
                has=has, tied=tied, off=off)


def matches_ref(disparity, step, left_id, right_id):
    """the valid pixels with x % step == 0 and y % step == 0 in raster order, as Match records"""
    h, w = disparity.shape
    valid = disparity.view(np.uint32) != NAN_BITS
    sel = np.zeros_like(valid)
    sel[::step, ::step] = valid[::step, ::step]
    ys, xs = np.nonzero(sel)  # raster order
    out = np.zeros(len(ys), H.MATCH)
    out["kp0_parent"] = left_id
    out["kp1_parent"] = right_id
    out["kp0_loc"][:, 0] = xs.astype(np.float32)
    out["kp0_loc"][:, 1] = ys.astype(np.float32)
    out["kp1_loc"][:, 0] = xs.astype(np.float32) - disparity[ys, xs]
    out["kp1_loc"][:, 1] = ys.astype(np.float32)
    return out


def points_ref(matches, foc, baseline, doffset, cx, cy):
    """upstream's stereo_disparity in float32, in the contract's order"""
    f32 = np.float32
    foc, baseline, doffset, cx, cy = f32(foc), f32(baseline), f32(doffset), f32(cx), f32(cy)
    x0, y0, x1 = matches["kp0_loc"][:, 0], matches["kp0_loc"][:, 1], matches["kp1_loc"][:, 0]
    s = (x0 - x1) + doffset
    good = (matches["invalid"] == 0) & (s > 0)
    with np.errstate(all="ignore"):
        Z = (foc * baseline) / s
        X = ((x0 - cx) * Z) / foc
        Y = ((y0 - cy) * Z) / foc
    out = np.zeros((len(matches), 3), np.float32)
    out[good, 0], out[good, 1], out[good, 2] = X[good], Y[good], Z[good]
    return out
