"""include/ssrlcv_hip.h "terrain filter", restated in numpy: grey-scale morphology of a height map in the total order of the
integer key, the progressive morphological filter on top of it and the map - map difference.  Maps are float32 (H, W);
everything but the one subtraction is decided on the uint32 bit patterns.  The window minima are separable -- rows, then columns
-- and each is a minimum over shifted copies of a line padded with "nothing", the shifts doubled so that a large radius stays
cheap; nothing here is shared with the kernels' running minima.  tests/test_terrain_cases.py holds it to a plain double loop over
the clipped 2-D window."""
import numpy as np

INVALID = 0x7FC00000
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
GROUND, NO_CELL = 0, 255
_NOTHING = np.int64(1) << 40          # above every key


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def keys(bits):
    """the integer key of the median filter, k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF, as int64: the float order made total"""
    b = np.ascontiguousarray(bits, np.uint32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)).astype(np.int64)


def bits_from_keys(k):
    """the key is its own inverse"""
    k = np.asarray(k, np.int64).astype(np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).view(np.uint32)


def effective_radius(radius, w, h):
    return min(int(radius), max(w, h) - 1)


def _line_minimum(k, r, axis):
    """min over [x - r, x + r] clipped at the line's ends, along `axis` of the int64 array k"""
    n = k.shape[axis]
    r = min(r, n - 1)                 # a window clipped at the line is the window of the smaller radius
    if r == 0:
        return k
    k = np.moveaxis(k, axis, -1)
    pad = np.full(k.shape[:-1] + (r,), _NOTHING, np.int64)
    m = np.concatenate([pad, k, pad], axis=-1)      # m[..., i] covers the padded cells [i, i + span)
    length, span = 2 * r + 1, 1
    while 2 * span <= length:
        m = np.minimum(m[..., :-span], m[..., span:])
        span *= 2
    out = np.minimum(m[..., :n], m[..., length - span:length - span + n])
    return np.moveaxis(out, -1, axis)


def _select(bits, r, largest):
    """the smallest (largest) key among the valid cells of the clipped window -> bits, INVALID where the window holds none"""
    valid = bits != INVALID
    k = keys(bits)
    k = np.where(valid, -k if largest else k, _NOTHING)
    k = _line_minimum(_line_minimum(k, r, 1), r, 0)
    none = k == _NOTHING
    out = bits_from_keys(np.where(none, 0, -k if largest else k))
    out[none] = INVALID
    return out


def morphology_bits(bits, radius, op):
    h, w = bits.shape
    assert radius >= 1 and op in (ERODE, DILATE, OPEN, CLOSE) and w > 0 and h > 0
    r = effective_radius(radius, w, h)
    if op == ERODE:
        return _select(bits, r, False)
    if op == DILATE:
        return _select(bits, r, True)
    out = _select(_select(bits, r, op == CLOSE), r, op == OPEN)
    out[bits == INVALID] = INVALID    # holes stay holes
    return out


def morphology(a, radius, op):
    """-> float32 (H, W) holding input bits or the invalid pattern"""
    return morphology_bits(bits_of(a), radius, op).view(np.float32)


def terrain(height, radii, thresholds):
    """-> dict(terrain float32, level uint8, opened float32, flagged: the number of cells each level flagged first)"""
    assert 1 <= len(radii) == len(thresholds) <= 8
    assert all(r >= 1 for r in radii) and all(b > a for a, b in zip(radii, radii[1:]))
    src = bits_of(height)
    valid = src != INVALID
    level = np.where(valid, GROUND, NO_CELL).astype(np.uint8)
    z = src
    for k, (r, t) in enumerate(zip(radii, thresholds), 1):
        t = np.float32(t)
        assert np.isfinite(t) and t >= 0
        o = morphology_bits(z, r, OPEN)
        with np.errstate(invalid="ignore", over="ignore"):
            d = z.view(np.float32) - o.view(np.float32)           # float32; never stored
            flagged = valid & (d > t)                             # false for a NaN
        level[flagged & (level == GROUND)] = k
        z = o
    out = src.copy()
    out[level != GROUND] = INVALID
    return {"terrain": out.view(np.float32), "level": level, "opened": z.view(np.float32),
            "flagged": [int((level == k).sum()) for k in range(1, len(radii) + 1)]}


def subtract(a, b):
    """a - b in float32 where both are valid and the result is a number; the invalid pattern elsewhere"""
    ua, ub = bits_of(a), bits_of(b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (ua.view(np.float32) - ub.view(np.float32)).astype(np.float32)
    out = d.view(np.uint32).copy()
    out[(ua == INVALID) | (ub == INVALID) | np.isnan(d)] = INVALID
    return out.view(np.float32)


def schedule(cell, max_radius, slope, initial, maximum, radii=None):
    """Zhang's schedule restated: radii 1, 2, 4, ... with max_radius last; t_1 = initial, t_k = min(initial + slope cell 2 (r_k -
    r_{k-1}), maximum) in double, rounded to float32 once"""
    if radii is None:
        radii, r = [], 1
        while r < max_radius:
            radii.append(r)
            r *= 2
        radii.append(int(max_radius))
    thresholds = [np.float32(initial)] + [np.float32(min(float(initial) + float(slope) * float(cell) * 2.0 * (b - a), float(maximum)))
                                          for a, b in zip(radii, radii[1:])]
    return list(radii), thresholds
