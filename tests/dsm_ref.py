"""The contract of include/ssrlcv_hip.h "surface model" restated in numpy, operation by operation.  Every float32 element-wise
operation of numpy is the IEEE one, so this is exact: tests/test_gpu_dsm.py holds the kernels of csrc/dsm.hip to it bit for bit,
and tests/test_dsm_cases.py proves on it alone that the cases of tests/dsm_cases.py test something."""
from collections import namedtuple

import numpy as np

INVALID_BITS = np.uint32(0x7FC00000)
NONE = np.uint32(0xFFFFFFFF)
f32 = np.float32

MAX, MIN = 0, 1                          # rasterize's rule
FUSE_MIN, FUSE_MEDIAN, FUSE_MAX = 0, 1, 2

Frame = namedtuple("Frame", "origin ex ey ez cell w h")


def frame(origin, ex, ey, ez, cell, w, h):
    v = lambda a: np.asarray(a, np.float32).reshape(3).copy()  # noqa: E731
    return Frame(v(origin), v(ex), v(ey), v(ez), f32(cell), int(w), int(h))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def key(a):
    """k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF of the bits as an int32: the float order as a total integer order, -0 below +0"""
    b = bits(a).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7FFFFFFF)


def _along(q, e):
    return ((q[:, 0] * e[0]) + (q[:, 1] * e[1])) + (q[:, 2] * e[2])


def locate(points, fr):
    """item 1 up to the cell -> dict(a, b, z, u, v float32 (n,), fi, fj float32, inside bool (n,), cell int64 (n,), -1 outside
    or skipped)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = p - fr.origin[None, :]
        a, b, z = _along(q, fr.ex), _along(q, fr.ey), _along(q, fr.ez)
        u, v = a / fr.cell, b / fr.cell
        fi, fj = np.floor(u), np.floor(v)
        usable = np.isfinite(p).all(1) & ~(p == 0).all(1)   # -0 == 0: either sign of zero
        inside = usable & (fi >= 0) & (fi < f32(fr.w)) & (fj >= 0) & (fj < f32(fr.h)) & np.isfinite(z)
    cell = np.full(len(p), -1, np.int64)
    cell[inside] = fj[inside].astype(np.int64) * fr.w + fi[inside].astype(np.int64)
    return dict(a=a, b=b, z=z, u=u, v=v, fi=fi, fj=fj, inside=inside, cell=cell)


def rasterize(points, fr, rule):
    """item 1 -> (height float32 (h, w), source uint32 (h, w), count uint32 (h, w))"""
    loc = locate(points, fr)
    cells = fr.w * fr.h
    height = np.full(cells, INVALID_BITS, np.uint32)
    source = np.full(cells, NONE, np.uint32)
    idx = np.nonzero(loc["inside"])[0]
    count = np.bincount(loc["cell"][idx], minlength=cells).astype(np.uint32) if cells else np.zeros(0, np.uint32)
    if len(idx):
        k = key(loc["z"][idx])
        # the winner of a cell comes first: the greatest (least) key, then the smallest index
        order = np.lexsort((idx, -k if rule == MAX else k, loc["cell"][idx]))
        c = loc["cell"][idx][order]
        first = np.concatenate([[True], c[1:] != c[:-1]])
        win = idx[order][first]
        height[c[first]] = bits(loc["z"])[win]
        source[c[first]] = win.astype(np.uint32)
    return height.view(np.float32).reshape(fr.h, fr.w), source.reshape(fr.h, fr.w), count.reshape(fr.h, fr.w)


def fuse(maps, min_views, max_spread, rule):
    """item 2 -> (out float32 (h, w), views uint8 (h, w))"""
    stack = np.stack([bits(m) for m in maps])                 # (m, h, w)
    valid = stack != INVALID_BITS
    n = valid.sum(0)
    k = np.where(valid, key(stack.view(np.float32)), np.int64(1) << 40)   # the invalid entries behind every value
    order = np.argsort(k, axis=0, kind="stable")
    ranked = np.take_along_axis(stack, order, 0)              # the valid entries by key, then the invalid ones
    last = np.maximum(n - 1, 0)[None]
    lo, hi = ranked[0].view(np.float32), np.take_along_axis(ranked, last, 0)[0].view(np.float32)
    with np.errstate(all="ignore"):
        agree = (hi - lo) <= f32(max_spread)                  # false for a NaN
    want = {FUSE_MIN: np.zeros_like(last), FUSE_MEDIAN: np.maximum(n - 1, 0)[None] // 2, FUSE_MAX: last}[rule]
    picked = np.take_along_axis(ranked, want, 0)[0]
    out = np.where((n >= min_views) & (n > 0) & agree, picked, INVALID_BITS).astype(np.uint32)
    return out.view(np.float32), n.astype(np.uint8)


def points(height, fr):
    """item 3 -> float32 (count, 3): the valid cells in raster order"""
    hb = bits(height).reshape(fr.h, fr.w)
    jj, ii = np.nonzero(hb != INVALID_BITS)
    z = hb[jj, ii].view(np.float32)
    with np.errstate(all="ignore"):
        a = (ii.astype(np.float32) + f32(0.5)) * fr.cell
        b = (jj.astype(np.float32) + f32(0.5)) * fr.cell
        out = np.stack([((fr.origin[k] + (a * fr.ex[k])) + (b * fr.ey[k])) + (z * fr.ez[k]) for k in range(3)], 1)
    return out.astype(np.float32).reshape(-1, 3)
