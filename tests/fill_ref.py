"""include/ssrlcv_hip.h "hole filling", restated in numpy: a plain ray walk per hole and direction and a sort.  Slow on purpose:
nothing here is shared with the kernels' carries.  Maps are float32 (H, W); everything is decided on the uint32 bit patterns.

The keyword-only switches of fill() are DELIBERATE DEFECTS, off by default: tests/test_fill_cases.py turns each on to prove
that the cases of tests/fill_cases.py would see a kernel that had it."""
import numpy as np

INVALID = 0x7FC00000
NO_LIMIT = 0xFFFFFFFF
MIN, MEDIAN = 0, 1
# "semi-global matching" item 2: direction i carries values along (dx, dy); its source lies at p - t (dx, dy)
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]


def bits_of(disp):
    return np.ascontiguousarray(disp, np.float32).view(np.uint32)


def key(b):
    """the integer key of the median filter: the float order made total, -0 below +0"""
    b = int(np.int32(np.uint32(b)))
    return b if b >= 0 else b ^ 0x7FFFFFFF


def popcount(paths):
    return bin(paths).count("1")


def hit(bits, x, y, dx, dy, max_gap):
    """the first measured pixel among (x, y) - t (dx, dy), t = 1 .. max_gap, inside the image -> its bits, or None"""
    h, w = bits.shape
    t = 1
    while t <= max_gap:
        px, py = x - t * dx, y - t * dy
        if not (0 <= px < w and 0 <= py < h):
            return None
        if bits[py, px] != INVALID:
            return int(bits[py, px])
        t += 1
    return None


def fill(disp, paths, max_gap, min_hits, rule, *, reverse=False, transpose=False, gap_off=0, upper=False, float_order=False,
         chained=False, ignore_min_hits=False):
    """-> (out float32 (H, W), filled uint8 (H, W))"""
    assert 1 <= paths <= 0xFF and 1 <= min_hits <= popcount(paths) and rule in (MIN, MEDIAN)
    src = bits_of(disp)
    h, w = src.shape
    out = src.copy()
    filled = np.zeros((h, w), np.uint8)
    look = out if chained else src            # defect: filled pixels become sources, in raster order
    gap = max(0, min(max_gap + gap_off, max(w, h)))   # no ray is longer than the image
    for y in range(h):
        for x in range(w):
            if src[y, x] != INVALID:
                continue
            hits = []
            for i, (dx, dy) in enumerate(DIRECTIONS):
                if not paths >> i & 1:
                    continue
                if reverse:                   # defect: the source looked for downstream
                    dx, dy = -dx, -dy
                if transpose and dx and dy:   # defect: the diagonals of the transposed image: (+1, -1) and (-1, +1) change places
                    dx, dy = dy, dx
                b = hit(look, x, y, dx, dy, gap)
                if b is not None:
                    hits.append(b)
            n = len(hits)
            if n == 0 or (n < min_hits and not ignore_min_hits):
                continue
            if float_order:                   # defect: -0 == +0 and a NaN compares false with everything
                hits = _float_sorted(hits)
            else:
                hits.sort(key=key)
            rank = 0 if rule == MIN else (n // 2 if upper else (n - 1) // 2)
            out[y, x] = hits[rank]
            filled[y, x] = 1
    return out.view(np.float32), filled


def _float_sorted(hits):
    """an insertion sort with the float comparison `<`, as a kernel that compared floats would order them"""
    vals = [np.uint32(b).view(np.float32) for b in hits]
    order = []
    for b, v in zip(hits, vals):
        at = len(order)
        while at > 0 and v < order[at - 1][1]:
            at -= 1
        order.insert(at, (b, v))
    return [b for b, _ in order]
