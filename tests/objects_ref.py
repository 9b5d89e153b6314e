"""The numpy restatement of include/ssrlcv_hip.h "surface objects", item by item: what tests/test_gpu_objects.py holds the kernels
of csrc/objects.hip to, byte for byte.  The components are speckle_ref.components_ref's, by import; everything else is a sum, a
minimum or a maximum over the cells of a component.  objects_loop() says the same with a plain Python loop over cells and Python
integers, and tests/test_objects_cases.py holds the one to the other.  measures() restates ssrlcv_object_measures_host in numpy
float64, operation by operation in the header's order.

A map is a float32 array (h, w); a cell is valid iff its bits are not 0x7FC00000."""
import numpy as np

import speckle_ref as S

INVALID = S.INVALID_BITS
NONE = 0xFFFFFFFF
RECORD = np.dtype([("label", "<u4"), ("cells", "<u4"), ("minX", "<u4"), ("minY", "<u4"), ("maxX", "<u4"), ("maxY", "<u4"),
                   ("perimeter", "<u4"), ("clipped", "<u4"), ("peakIndex", "<u4"), ("peak", "<f4"), ("low", "<f4"), ("reserved", "<u4"),
                   ("sumX", "<u8"), ("sumY", "<u8"), ("sumXX", "<u8"), ("sumXY", "<u8"), ("sumYY", "<u8"), ("sumQ", "<i8"), ("sumQQ", "<u8")])
assert RECORD.itemsize == 104
MEASURES = ("area", "perimeterLength", "compactness", "centroidX", "centroidY", "world0", "world1", "world2", "meanHeight", "volume",
            "rmsHeight", "mxx", "mxy", "myy", "lambdaMajor", "lambdaMinor", "axisX", "axisY", "elongation")
CLIP = np.float32(65536.0)


def members(d, min_height):
    """item 1 -> bool (h, w)"""
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return S.valid_mask(d) & (d >= np.float32(min_height))      # false for a NaN


def member_map(d, min_height):
    """the map item 2 labels: v at members, the invalid pattern everywhere else"""
    out = S.bits(d).copy()
    out[~members(d, min_height)] = INVALID
    return out.view(np.float32)


def quantise(d, scale):
    """item 5, as "shift search" quantises -> (takes part: bool, q: int64, 0 where the cell does not take part)"""
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = d * np.float32(scale)                                    # one float32 multiplication
        ok = np.abs(t) <= CLIP                                       # false for a NaN
    q = np.zeros(d.shape, np.int64)
    q[ok] = np.rint(t[ok]).astype(np.int64)                          # ties to even
    return ok, q


def key_bits(key):
    """the order key's own inverse: int64 keys -> uint32 bits"""
    key = np.asarray(key, np.int64)
    return np.where(key >= 0, key, key ^ 0x7FFFFFFF).astype(np.int32).view(np.uint32)


def _labelled(d, min_height, max_diff, min_cells):
    """items 2-3 -> (member, label map with NONE at non-members, kept labels ascending, sizes map)"""
    member = members(d, min_height)
    labels, sizes = S.components_ref(member_map(d, min_height), max_diff)
    flat = labels.reshape(-1)
    roots = np.nonzero(flat == np.arange(flat.size, dtype=np.uint32))[0]
    kept = roots[sizes.reshape(-1)[roots] >= max(int(min_cells), 1)]
    return member, labels, kept.astype(np.uint32), sizes


def objects(d, min_height, max_diff=np.inf, scale=256.0, min_cells=1):
    """items 1-5 -> dict(count, ids uint32 (h, w), records RECORD (count,)): every kept object, whatever a capacity would be"""
    d = np.ascontiguousarray(d, np.float32)
    h, w = d.shape
    if h == 0 or w == 0:
        return {"count": 0, "ids": np.zeros((h, w), np.uint32), "records": np.zeros(0, RECORD)}
    member, labels, kept, _ = _labelled(d, min_height, max_diff, min_cells)
    count = len(kept)
    number = np.full(h * w + 1, NONE, np.uint32)                    # of a label; the last entry serves NONE
    number[kept] = np.arange(count, dtype=np.uint32)
    ids = number[np.minimum(labels, np.uint32(h * w))]
    records = np.zeros(count, RECORD)
    inside = ids != NONE
    k = ids[inside].astype(np.int64)
    ys, xs = np.nonzero(inside)
    ys, xs = ys.astype(np.uint64), xs.astype(np.uint64)
    index = (ys * np.uint64(w) + xs).astype(np.int64)
    records["label"] = kept
    records["cells"] = np.bincount(k, minlength=count)
    for name, value, at in (("minX", xs, np.minimum), ("minY", ys, np.minimum), ("maxX", xs, np.maximum), ("maxY", ys, np.maximum)):
        acc = np.full(count, NONE if at is np.minimum else 0, np.int64)
        at.at(acc, k, value.astype(np.int64))
        records[name] = acc
    for name, value in (("sumX", xs), ("sumY", ys), ("sumXX", xs * xs), ("sumXY", xs * ys), ("sumYY", ys * ys)):
        acc = np.zeros(count, np.uint64)
        np.add.at(acc, k, value)
        records[name] = acc
    # perimeter: the sides whose other side lies outside the map or is not a cell of the same object
    padded = np.full((h + 2, w + 2), NONE, np.uint32)
    padded[1:-1, 1:-1] = labels
    sides = np.zeros((h, w), np.int64)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        sides += padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != labels
    acc = np.zeros(count, np.int64)
    np.add.at(acc, k, sides[inside])
    records["perimeter"] = acc
    # peak and low: the largest and the smallest order key; the smallest index among the cells that hold the peak
    key = S.order_key(d)[inside]
    top, bottom = np.full(count, -(1 << 40), np.int64), np.full(count, 1 << 40, np.int64)
    np.maximum.at(top, k, key)
    np.minimum.at(bottom, k, key)
    holds = key == top[k]
    first = np.full(count, h * w, np.int64)
    np.minimum.at(first, k[holds], index[holds])
    records["peak"] = key_bits(top).view(np.float32)
    records["low"] = key_bits(bottom).view(np.float32)
    records["peakIndex"] = first
    ok, q = quantise(d, scale)
    ok, q = ok[inside], q[inside]
    records["clipped"] = np.bincount(k[~ok], minlength=count)
    sum_q, sum_qq = np.zeros(count, np.int64), np.zeros(count, np.uint64)
    np.add.at(sum_q, k[ok], q[ok])
    np.add.at(sum_qq, k[ok], (q[ok] * q[ok]).astype(np.uint64))
    records["sumQ"], records["sumQQ"] = sum_q, sum_qq
    return {"count": count, "ids": ids, "records": records}


def objects_loop(d, min_height, max_diff=np.inf, scale=256.0, min_cells=1):
    """the same by a plain loop over the cells, Python integers throughout"""
    d = np.ascontiguousarray(d, np.float32)
    h, w = d.shape
    ids = np.full((h, w), NONE, np.uint32)
    if h == 0 or w == 0:
        return {"count": 0, "ids": ids, "records": np.zeros(0, RECORD)}
    member, labels, kept, _ = _labelled(d, min_height, max_diff, min_cells)
    number = {int(label): i for i, label in enumerate(kept.tolist())}
    keys, bits = S.order_key(d).tolist(), S.bits(d).tolist()
    lab = labels.tolist()
    scale32 = np.float32(scale)
    acc = [dict(label=int(label), cells=0, minX=NONE, minY=NONE, maxX=0, maxY=0, perimeter=0, clipped=0, peakIndex=NONE, peakKey=None, peakBits=0,
                lowKey=None, lowBits=0, sumX=0, sumY=0, sumXX=0, sumXY=0, sumYY=0, sumQ=0, sumQQ=0) for label in kept.tolist()]
    for y in range(h):
        for x in range(w):
            if lab[y][x] not in number:                              # a non-member (NONE) or a member of a dropped object
                continue
            i = number[lab[y][x]]
            ids[y, x] = i
            r = acc[i]
            r["cells"] += 1
            r["minX"], r["minY"], r["maxX"], r["maxY"] = min(r["minX"], x), min(r["minY"], y), max(r["maxX"], x), max(r["maxY"], y)
            r["sumX"] += x
            r["sumY"] += y
            r["sumXX"] += x * x
            r["sumXY"] += x * y
            r["sumYY"] += y * y
            for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if not (0 <= nx < w and 0 <= ny < h) or lab[ny][nx] != lab[y][x]:
                    r["perimeter"] += 1
            if r["peakKey"] is None or keys[y][x] > r["peakKey"]:    # raster order: an equal key keeps the earlier index
                r["peakKey"], r["peakBits"], r["peakIndex"] = keys[y][x], bits[y][x], y * w + x
            if r["lowKey"] is None or keys[y][x] < r["lowKey"]:
                r["lowKey"], r["lowBits"] = keys[y][x], bits[y][x]
            with np.errstate(invalid="ignore", over="ignore"):
                t = d[y, x] * scale32
            if np.abs(t) <= CLIP:
                q = int(np.rint(t))
                r["sumQ"] += q
                r["sumQQ"] += q * q
            else:
                r["clipped"] += 1
    records = np.zeros(len(acc), RECORD)
    for i, r in enumerate(acc):
        for name in RECORD.names:
            if name in ("peak", "low"):
                records[name].view(np.uint32)[i] = r[name + "Bits"]
            elif name != "reserved":
                records[name][i] = r[name]
    return {"count": len(acc), "ids": ids, "records": records}


def truncated(result, capacity):
    """item 3: the first min(count, capacity) records; count and ids do not depend on the capacity"""
    return dict(result, records=result["records"][:min(result["count"], int(capacity))])


class Frame:
    """the fields of ssrlcv_dsm_frame the measures read, as float32"""

    def __init__(self, origin=(0, 0, 0), ex=(1, 0, 0), ey=(0, 1, 0), ez=(0, 0, 1), cell=1.0, w=0, h=0):
        self.origin, self.ex, self.ey, self.ez = (np.asarray(v, np.float32) for v in (origin, ex, ey, ez))
        self.cell, self.w, self.h = np.float32(cell), int(w), int(h)


def measures(record, frame, scale):
    """item 7 -> dict of float64, the header's expressions in the header's order"""
    f64, sqrt = np.float64, np.sqrt
    u = lambda name: f64(int(record[name]))  # noqa: E731  an integer to double, rounded to nearest even above 2^53
    with np.errstate(all="ignore"):
        c, s = f64(frame.cell), f64(np.float32(scale))
        n, cc = u("cells"), c * c
        m = {"area": n * cc, "perimeterLength": u("perimeter") * c}
        m["compactness"] = (f64(12.566370614359172) * m["area"]) / (m["perimeterLength"] * m["perimeterLength"])
        cx, cy = u("sumX") / n, u("sumY") / n
        m["centroidX"], m["centroidY"] = cx, cy
        a, b = (cx + f64(0.5)) * c, (cy + f64(0.5)) * c
        for k in range(3):
            m["world%d" % k] = (f64(frame.origin[k]) + a * f64(frame.ex[k])) + b * f64(frame.ey[k])
        part = f64(int(record["cells"]) - int(record["clipped"]))
        mean_q = u("sumQ") / part
        m["meanHeight"] = mean_q / s
        m["volume"] = (u("sumQ") / s) * cc
        var = u("sumQQ") / part - mean_q * mean_q
        m["rmsHeight"] = sqrt(f64(0.0) if var < 0 else var) / s
        m["mxx"], m["mxy"], m["myy"] = u("sumXX") / n - cx * cx, u("sumXY") / n - cx * cy, u("sumYY") / n - cy * cy
        t, d = f64(0.5) * (m["mxx"] + m["myy"]), f64(0.5) * (m["mxx"] - m["myy"])
        r = sqrt(d * d + m["mxy"] * m["mxy"])
        m["lambdaMajor"] = t + r
        low = t - r
        m["lambdaMinor"] = f64(0.0) if low < 0 else low
        vx, vy = (d + r, m["mxy"]) if d >= 0 else (m["mxy"], r - d)
        if vx < 0:
            vx, vy = -vx, -vy
        g = sqrt(vx * vx + vy * vy)
        m["axisX"], m["axisY"] = (vx / g, vy / g) if g > 0 else (f64(1.0), f64(0.0))
        m["elongation"] = sqrt(m["lambdaMajor"] / m["lambdaMinor"]) if m["lambdaMinor"] > 0 else f64(np.inf) if m["lambdaMajor"] > 0 else f64(1.0)
    return {name: f64(m[name]) for name in MEASURES}
