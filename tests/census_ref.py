"""The census-cost contract of include/ssrlcv_hip.h ("census cost") restated in numpy, item by item.  It shares no code with
csrc/stereo.hip: the codes are built one bit plane at a time, the Hamming distances come from a loop over the 64 bits, the
block sums from an integral image, one disparity at a time, into a whole cost volume.  What the contract takes over from
"dense stereo" and "semi-global matching" is taken over here too: stereo_ref.right_volume and sgm_ref.matching_cost /
aggregate work on a volume, and one winners() serves both forms.  Everything is exact, so the GPU results are compared bit for
bit."""
import numpy as np

import sgm_ref as G
import stereo_ref as R

NAN_BITS, NO_COST, BIG = R.NAN_BITS, R.NO_COST, R.BIG


def bits(c):
    """n of the contract: the bits of a (2c + 1)^2 code"""
    return (2 * c + 1) ** 2 - 1


def census(img, c):
    """item 1: T (uint64 h x w), 0 where the window leaves the image"""
    h, w = img.shape
    code = np.zeros((h, w), np.uint64)
    if w < 2 * c + 1 or h < 2 * c + 1:
        return code
    I = img.astype(np.int64)
    centre = I[c:h - c, c:w - c]
    b = 0
    for j in range(-c, c + 1):
        for i in range(-c, c + 1):
            if i == 0 and j == 0:
                continue
            darker = I[c + j:h - c + j, c + i:w - c + i] < centre
            code[c:h - c, c:w - c] |= darker.astype(np.uint64) << np.uint64(b)
            b += 1
    assert b == bits(c)
    return code


def popcount(v):
    """item 2's count, bit by bit"""
    v = v.copy()
    n = np.zeros(v.shape, np.int64)
    for _ in range(64):
        n += (v & np.uint64(1)).astype(np.int64)
        v >>= np.uint64(1)
    return n


def cost_volume(left, right, c, r, dmin, D):
    """C[k, y, x] (int64) = item 3's cost at d = dmin + k, BIG where it is not defined"""
    h, w = left.shape
    rho = c + r
    C = np.full((D, h, w), BIG, np.int64)
    if w < 2 * rho + 1 or h < 2 * rho + 1:
        return C
    TL, TR = census(left, c), census(right, c)
    for k in range(D):
        d = dmin + k
        x0, x1 = max(rho, rho + d), min(w - 1 - rho, w - 1 - rho + d)  # centres whose two footprints are inside
        if x0 > x1:
            continue
        a, b = x0 - r, x1 + r + 1  # the columns their aggregation windows cover
        ham = np.zeros((h, w), np.int64)
        ham[:, a:b] = popcount(TL[:, a:b] ^ TR[:, a - d:b - d])
        I = np.zeros((h + 1, w + 1), np.int64)
        I[1:, 1:] = ham.cumsum(0).cumsum(1)
        ys = np.arange(rho, h - rho)[:, None]
        xs = np.arange(x0, x1 + 1)[None, :]
        C[k, rho:h - rho, x0:x1 + 1] = I[ys + r + 1, xs + r + 1] - I[ys - r, xs + r + 1] - I[ys + r + 1, xs - r] + I[ys - r, xs - r]
    return C


def winners(V, dmin, max_cost=0xFFFFFFFF, lr=-1, subpixel=0):
    """items 2-6 of "dense stereo" (5-8 of "semi-global matching") over a volume V[k, y, x], BIG where d is no candidate
    -> dict: disparity (float32 h x w), cost (uint32), k (int winners, -1 none), has, valid, valid_before_lr, tied, off"""
    D, h, w = V.shape
    k = V.argmin(0)                      # first occurrence: the smallest d among equal costs
    best = V.min(0)
    has = best < BIG
    tied = has & ((V == best[None]).sum(0) > 1)
    valid = has & (best <= max_cost)
    before_lr = valid.copy()
    if lr >= 0:
        VR = R.right_volume(V, dmin)
        kR = VR.argmin(0)
        ys, xs = np.nonzero(valid)
        xr = xs - (dmin + k[ys, xs])
        assert (VR.min(0)[ys, xr] < BIG).all()
        keep = np.abs(kR[ys, xr] - k[ys, xs]) <= lr
        valid[ys[~keep], xs[~keep]] = False
    off = np.zeros((h, w), np.float32)
    both = np.zeros((h, w), bool)        # both neighbours of the winner are candidates
    if D >= 3:
        ys, xs = np.nonzero(has & (k >= 1) & (k <= D - 2))
        kk = k[ys, xs]
        cm, c0, cp = V[kk - 1, ys, xs], V[kk, ys, xs], V[kk + 1, ys, xs]
        ok = (cm < BIG) & (cp < BIG)
        both[ys[ok], xs[ok]] = True
        if subpixel:
            den = cm - 2 * c0 + cp
            ok &= den != 0
            num32 = (cm - cp)[ok].astype(np.float32)
            den32 = (2 * den)[ok].astype(np.float32)
            off[ys[ok], xs[ok]] = num32 / den32
    disp = (dmin + k).astype(np.float32) + off
    disp_bits = np.where(valid, disp.view(np.uint32), NAN_BITS).astype(np.uint32)
    cost = np.where(valid, best, np.int64(NO_COST)).astype(np.uint32)
    return dict(disparity=disp_bits.view(np.float32), cost=cost, k=np.where(has, k, -1), has=has, valid=valid, valid_before_lr=before_lr,
                tied=tied, off=off, both=both)


def census_disparity_ref(left, right, c, r, dmin, D, max_cost=0xFFFFFFFF, lr=-1, subpixel=0):
    """ssrlcv_hip_stereo_census_u8; also `volume`, the costs the winners were chosen from"""
    C = cost_volume(left, right, c, r, dmin, D)
    out = winners(C, dmin, max_cost, lr, subpixel)
    out["volume"] = C
    return out


def census_sgm_ref(left, right, c, r, dmin, D, clamp, P1, P2, paths=0xFF, lr=-1, subpixel=0):
    """ssrlcv_hip_stereo_sgm_census_u8; also lmax and clamped (the share of the defined costs the clamp cut)"""
    h, w = left.shape
    rho = c + r
    assert P1 <= P2 and 1 <= paths <= 0xFF and bin(paths).count("1") * (clamp + P2) <= 65535
    C = cost_volume(left, right, c, r, dmin, D)
    Sv = np.full((D, h, w), BIG, np.int64)
    lmax, clamped = 0, 0.0
    if w >= 2 * rho + 1 and h >= 2 * rho + 1:
        M, cand = G.matching_cost(C, rho, clamp)
        S, lmax = G.aggregate(M, P1, P2, paths)
        assert S.max() <= bin(paths).count("1") * (clamp + P2)
        Sv[:, rho:h - rho, rho:w - rho] = np.where(cand, S, BIG).transpose(2, 0, 1)
        if cand.any():
            clamped = float((C[:, rho:h - rho, rho:w - rho].transpose(1, 2, 0)[cand] > clamp).mean())
    out = winners(Sv, dmin, 0xFFFFFFFF, lr, subpixel)
    out["lmax"], out["clamped"] = lmax, clamped
    return out
