"""The shift search (include/ssrlcv_hip.h "shift search") restated in numpy, for tests/test_shift_cases.py, test_shift_host.py and
test_gpu_shift.py.  search() works shift by shift on two slices of the quantised maps, in int64, and keeps the three sums as
Python integers; loop() is the same contract cell by cell, for the small cases; pick() is the host pick in float64 scalars, one
rounding an operation."""
import numpy as np

INVALID = -(1 << 31)                 # the key of an invalid cell
NO_GATE = 0xFFFFFFFF
MAX_RADIUS = 32
HEAD = np.dtype([("validMoving", "<u4"), ("validReference", "<u4"), ("clippedMoving", "<u4"), ("clippedReference", "<u4")])
ENTRY = np.dtype([("n", "<u4"), ("reserved", "<u4"), ("sum", "<i8"), ("sumSq", "<u8")])


def quantise(a, scale):
    """-> (int64 keys, INVALID where the cell is invalid; how many cells are valid; how many are clipped)"""
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        t = (a * np.float32(scale)).astype(np.float32)
        ok = np.abs(t) <= np.float32(65536.0)                                     # false for a NaN
    q = np.full(a.shape, INVALID, np.int64)
    q[ok] = np.rint(t[ok]).astype(np.int64)                                        # ties to even
    return q, int(ok.sum()), int((~ok & np.isfinite(a)).sum())


def window(extent, s):
    """the cells x of 0 .. extent - 1 with 0 <= x + s < extent, as (lo, hi); hi <= lo when there is none"""
    return max(0, -s), min(extent, extent - s)


def search(moving, reference, scale, stride=1, center=(0, 0), radius=8, center_q=0, gate_q=NO_GATE):
    """-> (head: a HEAD record, entries: ENTRY (2S + 1, 2S + 1), [ky + S, kx + S])"""
    g, S = int(stride), int(radius)
    qm, vm, cm = quantise(np.asarray(moving)[::g, ::g], scale)
    qr, vr, cr = quantise(np.asarray(reference)[::g, ::g], scale)
    h, w = qm.shape
    head = np.zeros((), HEAD)
    head["validMoving"], head["validReference"], head["clippedMoving"], head["clippedReference"] = vm, vr, cm, cr
    entries = np.zeros((2 * S + 1, 2 * S + 1), ENTRY)
    for ky in range(-S, S + 1):
        sy = int(center[1]) + ky
        y0, y1 = window(h, sy)
        if y1 <= y0:
            continue
        for kx in range(-S, S + 1):
            sx = int(center[0]) + kx
            x0, x1 = window(w, sx)
            if x1 <= x0:
                continue
            a, b = qm[y0:y1, x0:x1], qr[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
            d = (a - b)[(a != INVALID) & (b != INVALID)]
            if gate_q != NO_GATE:
                d = d[np.abs(d - int(center_q)) <= int(gate_q)]
            e = entries[ky + S, kx + S]
            e["n"], e["sum"], e["sumSq"] = len(d), int(d.sum()), int((d * d).sum())   # |d| <= 2^17 and at most 2^28 of them
    return head, entries


def loop(moving, reference, scale, stride=1, center=(0, 0), radius=8, center_q=0, gate_q=NO_GATE):
    """the contract cell by cell, in Python integers"""
    g, S = int(stride), int(radius)
    moving, reference = np.asarray(moving, np.float32), np.asarray(reference, np.float32)
    H, W = moving.shape
    w, h = -(-W // g), -(-H // g)

    def key(a, i, j):
        x = a[j * g, i * g]
        with np.errstate(all="ignore"):
            t = np.float32(x * np.float32(scale))
        if not abs(t) <= np.float32(65536.0):
            return None, bool(np.isfinite(x))
        return int(np.rint(t)), False
    counts = [0, 0, 0, 0]
    keys = {}
    for which, a in enumerate((moving, reference)):
        for j in range(h):
            for i in range(w):
                q, clipped = key(a, i, j)
                keys[which, i, j] = q
                counts[which] += q is not None
                counts[2 + which] += clipped
    head = np.zeros((), HEAD)
    head["validMoving"], head["validReference"], head["clippedMoving"], head["clippedReference"] = counts
    entries = np.zeros((2 * S + 1, 2 * S + 1), ENTRY)
    for ky in range(-S, S + 1):
        for kx in range(-S, S + 1):
            sx, sy = int(center[0]) + kx, int(center[1]) + ky
            n = s1 = s2 = 0
            for y in range(h):
                for x in range(w):
                    if not (0 <= x + sx < w and 0 <= y + sy < h):
                        continue
                    a, b = keys[0, x, y], keys[1, x + sx, y + sy]
                    if a is None or b is None:
                        continue
                    d = a - b
                    if gate_q != NO_GATE and abs(d - int(center_q)) > int(gate_q):
                        continue
                    n, s1, s2 = n + 1, s1 + d, s2 + d * d
            e = entries[ky + S, kx + S]
            e["n"], e["sum"], e["sumSq"] = n, s1, s2
    return head, entries


def table_bytes(head, entries):
    """the table as the device lays it out: the 16-byte head, then the entries by ky, then kx"""
    return np.concatenate([np.frombuffer(head.tobytes(), np.uint8), np.frombuffer(np.ascontiguousarray(entries).tobytes(), np.uint8)])


def scores(entries, min_overlap):
    """-> (v float64 (2S + 1, 2S + 1), candidate bool): mean = sum / n, v = sumSq / n - mean mean, each operation rounded once"""
    side = entries.shape[0]
    v, cand = np.zeros((side, side), np.float64), np.zeros((side, side), bool)
    least = max(int(min_overlap), 1)
    for j in range(side):
        for i in range(side):
            n = int(entries[j, i]["n"])
            if n < least:
                continue
            cand[j, i] = True
            mean = np.float64(float(int(entries[j, i]["sum"]))) / np.float64(n)
            v[j, i] = np.float64(float(int(entries[j, i]["sumSq"]))) / np.float64(n) - mean * mean
    return v, cand


def pick(entries, scale, stride=1, center=(0, 0), min_overlap=0):
    """the host pick -> dict(shift, sub, bias, variance, second, n, candidates, k: (kx, ky)) or None without a candidate"""
    side = entries.shape[0]
    S = (side - 1) // 2
    v, cand = scores(entries, min_overlap)
    best = None
    for j in range(side):
        for i in range(side):
            if not cand[j, i]:
                continue
            k = (v[j, i], (i - S) ** 2 + (j - S) ** 2, j, i)
            if best is None or k < best:
                best = k
    if best is None:
        return None
    j, i = best[2], best[3]

    def step(minus, plus):
        if minus is None or plus is None or not cand[minus] or not cand[plus]:
            return np.float64(0.0)
        den = (v[minus] - v[j, i]) + (v[plus] - v[j, i])
        if not den > 0:
            return np.float64(0.0)
        s = np.float64(0.5) * (v[minus] - v[plus]) / den
        return np.float64(min(max(s, -0.5), 0.5))
    sx = step((j, i - 1) if i > 0 else None, (j, i + 1) if i < side - 1 else None)
    sy = step((j - 1, i) if j > 0 else None, (j + 1, i) if j < side - 1 else None)
    far = cand.copy()
    far[max(0, j - 1):j + 2, max(0, i - 1):i + 2] = False
    sc = np.float64(np.float32(scale))
    s2 = sc * sc
    n = int(entries[j, i]["n"])
    mean = np.float64(float(int(entries[j, i]["sum"]))) / np.float64(n)
    g = int(stride)
    return {"shift": (g * (int(center[0]) + i - S), g * (int(center[1]) + j - S)), "sub": (float(sx * np.float64(g)), float(sy * np.float64(g))),
            "bias": float(mean / sc), "variance": float(v[j, i] / s2), "second": float(v[far].min() / s2) if far.any() else float("inf"),
            "n": n, "candidates": int(cand.sum()), "k": (i - S, j - S)}


def level_gate(moving, reference, g, center, gate, scale):
    """pipeline._shift_gate restated: (centerQ, gateQ or None) from the lower median and gate x NMAD of the differences of the
    sampled maps at the shift `center`"""
    import accuracy_ref as A
    import terrain_ref as T
    m, r = np.asarray(moving, np.float32)[::g, ::g], np.asarray(reference, np.float32)[::g, ::g]
    h, w = m.shape
    (x0, x1), (y0, y1) = window(w, center[0]), window(h, center[1])
    if x1 <= x0 or y1 <= y0:
        return 0, None
    d = T.subtract(m[y0:y1, x0:x1], r[y0 + center[1]:y1 + center[1], x0 + center[0]:x1 + center[0]]).reshape(-1)
    signed = A.stats(d, quantiles=(5000,))
    if int(signed["finite"]) == 0:
        return 0, None
    median = np.float32(signed["quantile"][0])
    mad = A.stats(d, center=median, absolute=True, quantiles=(5000,))["quantile"][0]
    center_q = int(np.rint(np.float64(median) * np.float64(scale)))
    gate_q = int(np.floor(np.float64(gate) * (np.float64(1.4826) * np.float64(mad)) * np.float64(scale)))
    return max(-(1 << 18), min(1 << 18, center_q)), max(0, min(gate_q, NO_GATE - 1))


def levels(moving, reference, cell, radius=8, strides=(4, 1), gate=3.0, scale=None, min_overlap=0.25):
    """pipeline.surface_shift_search on two maps, restated -> dict(shift, bias, variance, second, levels: per level dict(params,
    result: pick()'s, head, entries)); None when a level has no candidate"""
    scale = float(np.float32(64.0 / float(cell) if scale is None else scale))
    best, out = (0, 0), []
    for k, g in enumerate(strides):
        center = (0, 0) if k == 0 else tuple(int(np.floor(b / g + 0.5)) for b in best)
        S = int(radius) if k == 0 else -(-strides[k - 1] // g) + 1
        center_q, gate_q = (0, None) if gate is None else level_gate(moving, reference, g, center, gate, scale)
        params = dict(scale=scale, stride=g, center=center, radius=S, center_q=center_q, gate_q=NO_GATE if gate_q is None else gate_q)
        head, entries = search(moving, reference, **params)
        res = pick(entries, scale, g, center, int(float(min_overlap) * int(head["validMoving"])))
        if res is None:
            return None
        best = res["shift"]
        out.append(dict(params=params, result=res, head=head, entries=entries))
    return {"shift": (best[0] + res["sub"][0], best[1] + res["sub"][1]), "bias": res["bias"], "variance": res["variance"], "second": res["second"],
            "levels": out}
