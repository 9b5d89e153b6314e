"""The numpy restatement of include/ssrlcv_hip.h "disparity post-filters", item by item: what tests/test_gpu_speckle.py holds the
kernels of csrc/disparity_filter.hip to, bit for bit.  Plain and slow on purpose: a flood fill with an explicit stack, a sort.

A map is a float32 array (h, w); a pixel is valid iff its bits are not 0x7FC00000 (INVALID_BITS) -- other NaNs and the
infinities are valid pixels."""
import numpy as np

INVALID_BITS = 0x7FC00000
NO_LABEL = 0xFFFFFFFF


def invalid_value():
    return np.array([INVALID_BITS], np.uint32).view(np.float32)[0]


def bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def valid_mask(d):
    return bits(d) != INVALID_BITS


def _links(d, max_diff):
    """item 1 -> (right, down): right[y, x] = (x, y) is linked to (x + 1, y); down[y, x] = (x, y) is linked to (x, y + 1)"""
    d = np.ascontiguousarray(d, np.float32)
    v = valid_mask(d)
    md = np.float32(max_diff)
    h, w = d.shape
    right = np.zeros((h, w), bool)
    down = np.zeros((h, w), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        # one float32 subtraction; <= is false for a NaN
        right[:, :-1] = v[:, :-1] & v[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= md)
        down[:-1, :] = v[:-1, :] & v[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= md)
    return right, down


def components_ref(d, max_diff):
    """items 1-2 -> (labels uint32 (h, w), sizes uint32 (h, w))"""
    d = np.ascontiguousarray(d, np.float32)
    h, w = d.shape
    labels = np.full((h, w), NO_LABEL, np.uint32)
    sizes = np.zeros((h, w), np.uint32)
    if h == 0 or w == 0:
        return labels, sizes
    v = valid_mask(d)
    right, down = _links(d, max_diff)
    right, down, v = right.tolist(), down.tolist(), v.tolist()
    seen = [[False] * w for _ in range(h)]
    for y0 in range(h):
        for x0 in range(w):
            if not v[y0][x0] or seen[y0][x0]:
                continue
            # raster order: the first pixel met of a component is its smallest raster index
            seen[y0][x0] = True
            stack, members = [(x0, y0)], []
            while stack:
                x, y = stack.pop()
                members.append((x, y))
                if x + 1 < w and right[y][x] and not seen[y][x + 1]:
                    seen[y][x + 1] = True
                    stack.append((x + 1, y))
                if x > 0 and right[y][x - 1] and not seen[y][x - 1]:
                    seen[y][x - 1] = True
                    stack.append((x - 1, y))
                if y + 1 < h and down[y][x] and not seen[y + 1][x]:
                    seen[y + 1][x] = True
                    stack.append((x, y + 1))
                if y > 0 and down[y - 1][x] and not seen[y - 1][x]:
                    seen[y - 1][x] = True
                    stack.append((x, y - 1))
            xs = np.array([m[0] for m in members])
            ys = np.array([m[1] for m in members])
            labels[ys, xs] = y0 * w + x0
            sizes[ys, xs] = len(members)
    return labels, sizes


def speckles_ref(d, cost, max_diff, max_size):
    """item 3 -> (disparity, cost or None): copies, the components of at most max_size pixels invalidated"""
    d = np.ascontiguousarray(d, np.float32).copy()
    _, sizes = components_ref(d, max_diff)
    remove = valid_mask(d) & (sizes <= np.uint32(max_size))
    d.view(np.uint32)[remove] = INVALID_BITS
    if cost is not None:
        cost = np.ascontiguousarray(cost, np.uint32).copy()
        cost[remove] = 0xFFFFFFFF
    return d, cost


def order_key(d):
    """k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF on the bits as int32 (int64 here, so that a padding key above every real one exists)"""
    b = bits(d).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7FFFFFFF)


def median_ref(d, radius):
    """item 4 -> a new map: the lower median of the valid pixels of the clipped (2 radius + 1)^2 window; holes stay holes"""
    d = np.ascontiguousarray(d, np.float32)
    h, w = d.shape
    m = int(radius)
    assert m in (1, 2)
    out = np.full((h, w), invalid_value(), np.float32)
    if h == 0 or w == 0:
        return out
    v = valid_mask(d)
    PAD = 1 << 40                      # above every key: the missing entries sort last
    keys = np.where(v, order_key(d), PAD)
    padded = np.full((h + 2 * m, w + 2 * m), PAD, np.int64)
    padded[m:m + h, m:m + w] = keys
    stack = np.stack([padded[j:j + h, i:i + w] for j in range(2 * m + 1) for i in range(2 * m + 1)], axis=-1)
    n = (stack != PAD).sum(axis=-1)
    stack = np.sort(stack, axis=-1)
    rank = np.maximum(n - 1, 0) // 2
    key = np.take_along_axis(stack, rank[..., None], axis=-1)[..., 0]
    key = np.where(v, key, 0)
    b = np.where(key >= 0, key, key ^ 0x7FFFFFFF).astype(np.int32)   # k is its own inverse
    res = b.view(np.uint32)
    out.view(np.uint32)[v] = res[v]
    return out
