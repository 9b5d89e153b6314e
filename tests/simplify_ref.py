"""numpy restatement of include/ssrlcv_hip.h "surface simplification": the error map and the simplified mesh of a height map,
vectorised level by level over the padded domain [0, S]^2.  The GPU kernels (csrc/simplify.hip) are held to it bit for bit
(tests/test_gpu_simplify.py); tests/test_simplify_cases.py holds IT to a plain recursive bintree walk and to the mesh's
properties."""
import numpy as np

INVALID_BITS = np.uint32(0x7FC00000)
NONE = np.uint32(0xFFFFFFFF)
INF = np.float32(np.inf)


def invalid():
    return np.array([INVALID_BITS], np.uint32).view(np.float32)[0]


def levels(w, h):
    """L: the smallest integer with 2^L >= max(w - 1, h - 1, 1)"""
    m, L = max(w - 1, h - 1, 1), 0
    while (1 << L) < m:
        L += 1
    return L


def _padded(height):
    """the height map on the domain: (present bool, heights float32, both (S + 1, S + 1)), L, S"""
    h, w = height.shape
    L = levels(w, h)
    S = 1 << L
    present = np.zeros((S + 1, S + 1), bool)
    hp = np.zeros((S + 1, S + 1), np.float32)
    present[:h, :w] = height.view(np.uint32) != INVALID_BITS
    hp[:h, :w] = height
    return present, hp, L, S


def _grid(xs, ys):
    x, y = np.meshgrid(xs, ys)
    return x.ravel().astype(np.int64), y.ravel().astype(np.int64)


def _families(k, S):
    """the split nodes of level k in three families: (x, y, (ax, ay), (bx, by), [(cx, cy) of the two apexes, ascending in
    (y, x)], children [(x, y), ...], is_d).  Apexes and children may lie outside the domain: the caller masks them."""
    u = 1 << k
    odd, even = np.arange(u, S, 2 * u), np.arange(0, S + 1, 2 * u)
    v = u // 2
    diag = [(-v, -v), (v, -v), (-v, v), (v, v)] if k > 0 else []
    # A-nodes with tz(x) < tz(y): the edge runs along x
    x, y = _grid(odd, even)
    yield x, y, (x - u, y), (x + u, y), [(x, y - u), (x, y + u)], [(x + dx, y + dy) for dx, dy in diag], False
    # A-nodes with tz(y) < tz(x)
    x, y = _grid(even, odd)
    yield x, y, (x, y - u), (x, y + u), [(x - u, y), (x + u, y)], [(x + dx, y + dy) for dx, dy in diag], False
    # D-nodes
    x, y = _grid(odd, odd)
    main = (((x - u) // (2 * u) + (y - u) // (2 * u)) % 2) == 0
    sx = np.where(main, u, -u)  # a = (x - sx, y - u), b = (x + sx, y + u)
    yield (x, y, (x - sx, y - u), (x + sx, y + u), [(x + sx, y - u), (x - sx, y + u)],
           [(x - u, y), (x + u, y), (x, y - u), (x, y + u)], True)


def _inside(p, S):
    return (p[0] >= 0) & (p[0] <= S) & (p[1] >= 0) & (p[1] <= S)


def _take(arr, p, S, fill):
    ok = _inside(p, S)
    out = np.full(p[0].shape, fill, arr.dtype)
    out[ok] = arr[p[1][ok], p[0][ok]]
    return out, ok


def errors(height):
    """item 1: float32 (h, w)"""
    height = np.ascontiguousarray(height, np.float32)
    h, w = height.shape
    if h == 0 or w == 0:
        return np.zeros((h, w), np.float32)
    present, hp, L, S = _padded(height)
    E = np.full((S + 1, S + 1), INF, np.float32)
    with np.errstate(all="ignore"):
        for k in range(L):
            for fam in _families(k, S):  # the A-nodes read the D-nodes of k - 1, the D-nodes (the last family) the A-nodes of k
                _level(E, present, hp, S, fam)
    return E[:h, :w].copy()  # a split node outside the grid is not present: +inf


def _level(E, present, hp, S, fam):
    x, y, a, b, apexes, children, _ = fam
    ok = present[y, x] & present[a[1], a[0]] & present[b[1], b[0]]
    for c in apexes:
        pc, exists = _take(present, c, S, False)
        ok &= pc | ~exists
    mid = (hp[a[1], a[0]] + hp[b[1], b[0]]) * np.float32(0.5)
    d = np.abs(hp[y, x] - mid).astype(np.float32)
    e = np.where(ok & (d < INF), d, INF).astype(np.float32)
    for c in children:
        ec, exists = _take(E, c, S, np.float32(0))
        e = np.maximum(e, np.where(exists, ec, np.float32(0)))
    E[y, x] = e


def mesh(height, error, tolerance, node_index=None):
    """items 2 and 3 -> dict(faces uint32 (T, 3): new vertex indices, in the contract's order; nodes int64 (T, 3, 2): the same
    corners as (x, y); vertex_index uint32 (h, w); kept uint32 (V,))"""
    height = np.ascontiguousarray(height, np.float32)
    h, w = height.shape
    tol = np.float32(tolerance)
    assert np.isfinite(tol)
    empty = {"faces": np.zeros((0, 3), np.uint32), "nodes": np.zeros((0, 3, 2), np.int64),
             "vertex_index": np.full((h, w), NONE, np.uint32), "kept": np.zeros(0, np.uint32)}
    if h == 0 or w == 0:
        return empty
    present, _, L, S = _padded(height)
    E = np.full((S + 1, S + 1), INF, np.float32)
    E[:h, :w] = error
    recs = []  # (my2, mx2, c, a, b) column blocks

    def add(my2, mx2, c, a, b, keep):
        if keep.any():
            recs.append(np.stack([my2[keep], mx2[keep], c[1][keep], c[0][keep], a[1][keep], a[0][keep], b[1][keep], b[0][keep]], 1))

    for k in range(L):
        for x, y, a, b, apexes, _, is_d in _families(k, S):
            in_grid = (x < w) & (y < h)
            em = E[y, x] <= tol
            root = is_d and k == L - 1
            for c in apexes:
                ec, exists = _take(E, c, S, INF)
                add(2 * y, 2 * x, c, a, b, in_grid & exists & em & (root | ~(ec <= tol)))
    if w > 1 and h > 1:
        i, j = _grid(np.arange(w - 1), np.arange(h - 1))
        main = ((i + j) % 2) == 0
        a = (np.where(main, i, i + 1), j)
        b = (np.where(main, i + 1, i), j + 1)
        for c in ((np.where(main, i + 1, i), j), (np.where(main, i, i + 1), j + 1)):
            keep = present[a[1], a[0]] & present[b[1], b[0]] & present[c[1], c[0]]
            if L != 0:
                keep &= ~(E[c[1], c[0]] <= tol)
            add(2 * j + 1, 2 * i + 1, c, a, b, keep)
    if not recs:
        return empty
    r = np.concatenate(recs, 0)
    r = r[np.lexsort((r[:, 3], r[:, 2], r[:, 1], r[:, 0]))]
    cy, cx, ay, ax, by, bx = (r[:, q] for q in range(2, 8))
    cross = (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)
    first = cross < 0  # (c, a, b), else (c, b, a)
    nodes = np.empty((len(r), 3, 2), np.int64)
    nodes[:, 0, 0], nodes[:, 0, 1] = cx, cy
    nodes[:, 1, 0], nodes[:, 1, 1] = np.where(first, ax, bx), np.where(first, ay, by)
    nodes[:, 2, 0], nodes[:, 2, 1] = np.where(first, bx, ax), np.where(first, by, ay)
    raster = nodes[:, :, 1] * w + nodes[:, :, 0]
    flag = np.zeros(w * h, bool)
    flag[raster.ravel()] = True
    vertex_index = np.full(w * h, NONE, np.uint32)
    vertex_index[flag] = np.arange(int(flag.sum()), dtype=np.uint32)
    where = np.flatnonzero(flag)
    kept = where.astype(np.uint32) if node_index is None else np.ascontiguousarray(node_index).view(np.uint32).ravel()[where]
    return {"faces": vertex_index[raster], "nodes": nodes, "vertex_index": vertex_index.reshape(h, w), "kept": kept}


def full_node_index(height):
    """the vertexIndex of ssrlcv_hip_disparity_mesh at step 1: a valid node's rank among the valid nodes in raster order"""
    valid = (np.ascontiguousarray(height, np.float32).view(np.uint32) != INVALID_BITS).ravel()
    out = np.full(valid.shape, NONE, np.uint32)
    out[valid] = np.arange(int(valid.sum()), dtype=np.uint32)
    return out.reshape(height.shape)
