"""The contract of include/ssrlcv_hip.h "surface accuracy" restated in numpy, operation by operation.  The difference is float32
element-wise numpy, every operation the IEEE one; the quantiles are np.sort over the keys; the sums are the contract's shape in
float64 -- the reshape (-1, 16, 256), sequential adds over the middle axis, halving folds.  tests/test_gpu_accuracy.py holds
csrc/accuracy.hip to it bit for bit, and tests/test_accuracy_cases.py proves on it alone that the cases test something."""
import numpy as np

import dsm_ref as D

INVALID_BITS = D.INVALID_BITS
INVALID = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
f32 = np.float32
TILE = 4096

RECORD = np.dtype([("n", "<u4"), ("valid", "<u4"), ("finite", "<u4"), ("reserved", "<u4"), ("sum", "<f8"), ("sumSq", "<f8"), ("min", "<f4"),
                   ("max", "<f4"), ("quantile", "<f4", (8,))])
assert RECORD.itemsize == 72


def difference(points, height, fr, cells=None):
    """item 1 -> float32 (n,).  cells None: CELL mode; otherwise the uint8 (h - 1, w - 1) bytes of the reference's mesh at step 1"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    hb = D.bits(height).reshape(fr.h, fr.w)
    hf = hb.view(np.float32)
    out = np.full(n, INVALID_BITS, np.uint32)
    loc = D.locate(p, fr)   # the skip rules and a, b, z, u, v of "surface model" item 1
    with np.errstate(all="ignore"):
        usable = np.isfinite(p).all(1) & ~(p == 0).all(1) & np.isfinite(loc["z"])
        z = loc["z"]
        if cells is None:
            fi, fj = np.floor(loc["u"]), np.floor(loc["v"])
            inside = usable & (fi >= 0) & (fi < f32(fr.w)) & (fj >= 0) & (fj < f32(fr.h))
            idx = np.nonzero(inside)[0]
            i, j = fi[idx].astype(np.int64), fj[idx].astype(np.int64)
            r = hf[j, i]
            ok = (hb[j, i] != INVALID_BITS) & np.isfinite(r)
            out[idx[ok]] = D.bits(z[idx[ok]] - r[ok])
            return out.view(np.float32)
        if fr.w < 2 or fr.h < 2:
            return out.view(np.float32)
        cells = np.asarray(cells, np.uint8).reshape(fr.h - 1, fr.w - 1)
        uu, vv = loc["u"] - f32(0.5), loc["v"] - f32(0.5)
        fi, fj = np.floor(uu), np.floor(vv)
        inside = usable & (fi >= 0) & (fi < f32(fr.w - 1)) & (fj >= 0) & (fj < f32(fr.h - 1))
        idx = np.nonzero(inside)[0]
        i, j = fi[idx].astype(np.int64), fj[idx].astype(np.int64)
        s, t = (uu[idx] - fi[idx]).astype(np.float32), (vv[idx] - fj[idx]).astype(np.float32)
        za, zb, zc, zd = hf[j, i], hf[j, i + 1], hf[j + 1, i], hf[j + 1, i + 1]
        byte = cells[j, i]
        bc = (byte & 4) != 0
        one = f32(1)
        ad0, bc0 = t >= s, (s + t) <= one
        r_ad0 = za + ((t * (zc - za)) + (s * (zd - zc)))
        r_ad1 = za + ((s * (zb - za)) + (t * (zd - zb)))
        r_bc0 = za + ((s * (zb - za)) + (t * (zc - za)))
        r_bc1 = zd + (((one - s) * (zc - zd)) + ((one - t) * (zb - zd)))
        first = np.where(bc, bc0, ad0)
        r = np.where(bc, np.where(bc0, r_bc0, r_bc1), np.where(ad0, r_ad0, r_ad1)).astype(np.float32)
        emitted = np.where(first, byte & 1, byte & 2) != 0
        ok = emitted & np.isfinite(r)
        out[idx[ok]] = D.bits(z[idx[ok]] - r[ok])
    return out.view(np.float32)


def transformed(values, center=0.0, absolute=False):
    """-> (y float32 (n,): every entry minus center, |.| with absolute; valid bool (n,); part bool (n,): valid and y finite)"""
    x = np.ascontiguousarray(values, np.float32).reshape(-1)
    valid = D.bits(x) != INVALID_BITS
    with np.errstate(all="ignore"):
        y = (x - f32(center)).astype(np.float32)
        if absolute:
            y = np.abs(y)
    return y, valid, valid & np.isfinite(y)


def _fold(lanes):
    """(tiles, 256) float64 lane sums -> (tiles,): acc[l] += acc[l + half], half = 128 .. 1"""
    acc = lanes.copy()
    half = 128
    while half >= 1:
        acc[:, :half] = acc[:, :half] + acc[:, half:2 * half]
        half //= 2
    return acc[:, 0].copy()


def shaped_sum(d):
    """float64 (m,) -> its sum in the contract's shape: tiles of 4096 padded with +0.0, lane l adding entries l + 256 r in order
    from +0.0, the lanes folded by halves, the tile sums by the same shape again until one is left"""
    d = np.asarray(d, np.float64).reshape(-1)
    if len(d) == 0:
        return np.float64(0.0)
    while True:
        tiles = (len(d) + TILE - 1) // TILE
        padded = np.zeros(tiles * TILE, np.float64)
        padded[:len(d)] = d
        rows = padded.reshape(tiles, 16, 256)
        lanes = np.zeros((tiles, 256), np.float64)
        for r in range(16):
            lanes = lanes + rows[:, r, :]
        d = _fold(lanes)
        if len(d) == 1:
            return d[0]


def stats(values, center=0.0, absolute=False, quantiles=()):
    """item 2 -> a RECORD scalar"""
    x = np.ascontiguousarray(values, np.float32).reshape(-1)
    rec = np.zeros((), RECORD)
    rec["min"] = rec["max"] = INVALID
    rec["quantile"] = INVALID
    if len(x) == 0:
        return rec
    y, valid, part = transformed(x, center, absolute)
    rec["n"], rec["valid"], rec["finite"] = len(x), int(valid.sum()), int(part.sum())
    d = np.where(part, y.astype(np.float64), 0.0)
    rec["sum"], rec["sumSq"] = shaped_sum(d), shaped_sum(d * d)
    m = int(part.sum())
    if m:
        b = D.bits(y[part]).view(np.int32)
        ranked = np.sort(np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)))    # key order: -0 below +0
        value = lambda k: np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)  # noqa: E731  the key is its own inverse
        rec["min"], rec["max"] = value(ranked[0]), value(ranked[-1])
        q = np.full(8, INVALID, np.float32)
        for k, parts in enumerate(quantiles):
            q[k] = value(ranked[int(parts) * (m - 1) // 10000])
        rec["quantile"] = q
    return rec


def report(diff):
    """pipeline.surface_accuracy's fields from the reference's statistics of the same differences"""
    signed = stats(diff, quantiles=(5000,))
    n, m = int(signed["n"]), int(signed["finite"])
    nan = float("nan")
    if m:
        bias = float(signed["quantile"][0])
        mad = float(stats(diff, center=bias, absolute=True, quantiles=(5000,))["quantile"][0])
        le = [float(v) for v in stats(diff, absolute=True, quantiles=(6827, 9000, 9500))["quantile"][:3]]
        mean, rms = float(np.float64(signed["sum"]) / np.float64(m)), float(np.sqrt(np.float64(signed["sumSq"]) / np.float64(m)))
    else:
        bias, mad, le, mean, rms = nan, nan, [nan] * 3, nan, nan
    return {"n": n, "coverage": m / n if n else nan, "bias": bias, "nmad": float(np.float64(1.4826) * np.float64(mad)), "mean": mean, "rms": rms,
            "le68": le[0], "le90": le[1], "le95": le[2], "min": float(signed["min"]), "max": float(signed["max"])}
