"""The semi-global-matching contract of include/ssrlcv_hip.h ("semi-global matching") restated in numpy, item by item.  The
SAD costs and the right view's gather come from tests/stereo_ref.py (cost_volume, right_volume); everything else is here.  It
shares no code with csrc/stereo.hip: the volumes are int64 and whole, a path pass walks the image line by line with every path
of the direction at once.  Everything is exact, so the GPU results are compared bit for bit."""
import numpy as np

import stereo_ref as R

NAN_BITS, NO_COST, BIG = R.NAN_BITS, R.NO_COST, R.BIG

# item 2: bit i of `paths` -> (dx, dy)
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]


def matching_cost(C, r, clamp):
    """item 1: M[v, u, k] (int64) over the interior (hi, wi, D); candidate[v, u, k]"""
    D, h, w = C.shape
    Ci = C[:, r:h - r, r:w - r].transpose(1, 2, 0)
    cand = Ci < BIG
    return np.where(cand, np.minimum(Ci, clamp), clamp).astype(np.int64), cand


def step(M, Lq, P1, P2):
    """item 3 for n pixels at once: M, Lq (n, D) -> L (n, D)"""
    m = Lq.min(1, keepdims=True)
    best = np.minimum(Lq, m + P2)
    up = np.full_like(Lq, BIG)
    up[:, 1:] = Lq[:, :-1] + P1
    dn = np.full_like(Lq, BIG)
    dn[:, :-1] = Lq[:, 1:] + P1
    return M + np.minimum(best, np.minimum(up, dn)) - m


def path_cost(M, dx, dy, P1, P2):
    """item 3: L_i over the interior for one direction.  Lines (rows for dy != 0, columns else) are visited in the
    direction's order; a pixel whose predecessor is outside the interior starts its path with M."""
    if dy == 0:  # the same walk on the transposed volume
        return path_cost(M.transpose(1, 0, 2), 0, dx, P1, P2).transpose(1, 0, 2)
    hi, wi, D = M.shape
    L = np.empty_like(M)
    us = np.arange(wi)
    has = (us - dx >= 0) & (us - dx < wi)          # columns whose predecessor column exists
    for v in (range(hi) if dy > 0 else range(hi - 1, -1, -1)):
        L[v] = M[v]
        if 0 <= v - dy < hi and has.any():
            L[v, us[has]] = step(M[v, us[has]], L[v - dy, us[has] - dx], P1, P2)
    return L


def aggregate(M, P1, P2, paths):
    """item 4: S over the interior, and the largest L met (for the bound of item 3)"""
    S = np.zeros_like(M)
    lmax = 0
    for i, (dx, dy) in enumerate(DIRECTIONS):
        if (paths >> i) & 1:
            L = path_cost(M, dx, dy, P1, P2)
            assert L.min() >= 0
            lmax = max(lmax, int(L.max()))
            S += L
    return S, lmax


def sgm_ref(left, right, r, dmin, D, clamp, P1, P2, paths=0xFF, lr=-1, subpixel=0):
    """-> dict: disparity (float32 h x w), cost (uint32), plus what tests/test_sgm_cases.py looks at: k (int winners, -1
    none), has, valid, valid_before_lr, off, lmax, clamped (share of the defined costs the clamp cut)"""
    h, w = left.shape
    assert P1 <= P2 and 1 <= paths <= 0xFF and bin(paths).count("1") * (clamp + P2) <= 65535
    C = R.cost_volume(left, right, r, dmin, D)
    Sv = np.full((D, h, w), BIG, np.int64)       # S where d is a candidate, BIG elsewhere: what the winners choose from
    lmax, clamped = 0, 0.0
    if w >= 2 * r + 1 and h >= 2 * r + 1:
        M, cand = matching_cost(C, r, clamp)
        S, lmax = aggregate(M, P1, P2, paths)
        assert S.max() <= bin(paths).count("1") * (clamp + P2)
        Sv[:, r:h - r, r:w - r] = np.where(cand, S, BIG).transpose(2, 0, 1)
        if cand.any():
            clamped = float((C[:, r:h - r, r:w - r].transpose(1, 2, 0)[cand] > clamp).mean())
    k = Sv.argmin(0)                             # item 5: first occurrence = the smallest d among equal S
    sbest = Sv.min(0)
    has = sbest < BIG
    valid = has.copy()
    before_lr = valid.copy()
    if lr >= 0:                                  # item 6
        SR = R.right_volume(Sv, dmin)
        kR = SR.argmin(0)
        ys, xs = np.nonzero(valid)
        xr = xs - (dmin + k[ys, xs])
        assert (SR.min(0)[ys, xr] < BIG).all()
        keep = np.abs(kR[ys, xr] - k[ys, xs]) <= lr
        valid[ys[~keep], xs[~keep]] = False
    off = np.zeros((h, w), np.float32)
    if subpixel:                                 # item 7
        ys, xs = np.nonzero(has & (k >= 1) & (k <= D - 2))
        kk = k[ys, xs]
        sm, s0, sp = Sv[kk - 1, ys, xs], Sv[kk, ys, xs], Sv[kk + 1, ys, xs]
        ok = (sm < BIG) & (sp < BIG)
        den = sm - 2 * s0 + sp
        ok &= den != 0
        num32 = (sm - sp)[ok].astype(np.float32)
        den32 = (2 * den)[ok].astype(np.float32)
        off[ys[ok], xs[ok]] = num32 / den32
    disp = (dmin + k).astype(np.float32) + off
    bits = np.where(valid, disp.view(np.uint32), NAN_BITS).astype(np.uint32)
    cost = np.where(valid, sbest, np.int64(NO_COST)).astype(np.uint32)
    return dict(disparity=bits.view(np.float32), cost=cost, k=np.where(has, k, -1), has=has, valid=valid, valid_before_lr=before_lr,
                off=off, lmax=lmax, clamped=clamped)
