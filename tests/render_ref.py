"""The contract of include/ssrlcv_hip.h "mesh render" restated in numpy, operation by operation: float32 step by step, every
product, sum and division a numpy float32 operation of its own (the IEEE one), the edge functions in integers that are asserted
to fit int32.  tests/test_gpu_render.py holds csrc/render.hip to it byte for byte, and tests/test_render_cases.py proves on it
alone that the cases of tests/render_cases.py test something.  The triangles are set up one at a time in Python integers and
then walk their boxes side by side; the winner is a running maximum of the packed word, which is what an atomicMax leaves
whatever the order."""
from collections import namedtuple

import numpy as np

import mesh_ref as M

f32, u32, u64, i64 = np.float32, np.uint32, np.uint64, np.int64
INVALID_BITS = u32(0x7FC00000)
NONE = u32(0xFFFFFFFF)
DRAWN, TOO_LARGE, UNUSABLE = 0, 1, 2          # the slots of counts
MAX_W = f32(2.0 ** 60)
MAX_S = f32(1048576.0)

View = namedtuple("View", "M pos w h")        # M float32 (9,), pos float32 (3,); the image is w x h


def view(M9, pos, w, h):
    return View(np.asarray(M9, f32).reshape(9).copy(), np.asarray(pos, f32).reshape(3).copy(), int(w), int(h))


def project(points, v):
    """"vertex" -> (fx, fy int64 holding int32 values, iw float32, usable bool), one entry a vertex"""
    P = np.asarray(points, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = [P[:, k] - v.pos[k] for k in range(3)]
        X = (v.M[0] * d[0] + v.M[1] * d[1]) + v.M[2] * d[2]
        Y = (v.M[3] * d[0] + v.M[4] * d[1]) + v.M[5] * d[2]
        W = (v.M[6] * d[0] + v.M[7] * d[1]) + v.M[8] * d[2]
        sx, sy = X / W, Y / W
        iw = f32(1.0) / W
        usable = np.isfinite(P).all(1) & (W > 0) & (W <= MAX_W) & np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= MAX_S) & (np.abs(sy) <= MAX_S)
        usable &= np.isfinite(iw)
        qx, qy = np.rint(sx * f32(256.0)), np.rint(sy * f32(256.0))      # ties to even
    assert sx.dtype == f32 and iw.dtype == f32 and qx.dtype == f32
    fx, fy = np.zeros(len(P), i64), np.zeros(len(P), i64)
    fx[usable], fy[usable] = qx[usable].astype(i64), qy[usable].astype(i64)
    return fx, fy, iw, usable


def int32(x):
    assert np.all(np.abs(x) < 2 ** 31), "an edge value left int32"
    return x


def edge(ax, ay, bx, by, cx, cy):
    """E(a, b; c) = (b.x - a.x) (c.y - a.y) - (b.y - a.y) (c.x - a.x), every intermediate inside int32"""
    return int32(int32(int32(bx - ax) * int32(cy - ay)) - int32(int32(by - ay) * int32(cx - ax)))


def triangles(vertex_index, cells, loop=False):
    """every emitted triangle in id order -> list of (id, (ip, iq, ir)): the vertexIndex entries of its corners p, q, r.  loop:
    visit every cell in turn, the plain form; without it only the cells that emit one, in the same raster order (a grid of
    millions of cells that holds a few quads; tests/test_large_cases.py holds the two forms to each other)"""
    out = []
    gw = vertex_index.shape[1]
    if loop:
        visit = ((j, i) for j in range(cells.shape[0]) for i in range(cells.shape[1]))
    else:
        visit = zip(*(a.tolist() for a in np.nonzero(np.asarray(cells) & 3)))
    for j, i in visit:
        byte = int(cells[j, i])
        for t, tri in enumerate(M.TRIANGLES[bool(byte & 4)]):
            if byte >> t & 1:
                out.append((2 * (j * (gw - 1) + i) + t, tuple(int(vertex_index[j + dj, i + di]) for di, dj in tri)))
    return out


def weights(ep, eq, er, a):
    """lp, lq, lr: (float)E / (float)A, the conversions rounding to nearest even"""
    fa = np.asarray(a).astype(f32)
    with np.errstate(all="ignore"):
        return np.asarray(ep).astype(f32) / fa, np.asarray(eq).astype(f32) / fa, np.asarray(er).astype(f32) / fa


def setup(tri, n, fx, fy, usable, span, w, h):
    """"triangle" up to the pixel range -> (slot of counts or None, (xs, ys, |A|, sign, x0, x1, y0, y1) if drawn)"""
    if any(k >= n for k in tri) or not all(usable[k] for k in tri):
        return UNUSABLE, None
    xs, ys = [int(fx[k]) for k in tri], [int(fy[k]) for k in tri]
    if max(xs) - min(xs) > span or max(ys) - min(ys) > span:
        return TOO_LARGE, None
    A = int(edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2]))
    if A == 0:
        return UNUSABLE, None
    x0, x1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, w - 1)       # python's // floors, for negative coordinates too
    y0, y1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, h - 1)
    if x0 > x1 or y0 > y1:
        return None, None
    return DRAWN, xs + ys + [abs(A), 1 if A > 0 else -1, x0, x1, y0, y1]


def edges_at(T, cx, cy):
    """Ep, Eq, Er at pixel centres (cx, cy) in fixed point, negated where A < 0.  T: rows of setup's numbers, one a centre"""
    px, qx, rx, py, qy, ry, sign = T[:, 0], T[:, 1], T[:, 2], T[:, 3], T[:, 4], T[:, 5], T[:, 7]
    return edge(qx, qy, rx, ry, cx, cy) * sign, edge(rx, ry, px, py, cx, cy) * sign, edge(px, py, qx, qy, cx, cy) * sign


def render(points, grey, vertex_index, cells, v, max_extent, order=None, on_cover=None):
    """ssrlcv_hip_mesh_render -> dict: depth uint32 bits (h, w), triangle uint32 (h, w), shade uint8 (h, w), counts uint32 (3,).
    order: a permutation of the triangle list's positions, the order they are visited in.  on_cover(ids, xs, ys, v): called with
    covered pixels, the triangles that cover them and their float32 v, until every covered centre of every drawn triangle was
    named once.  The drawn triangles walk their boxes side by side, an offset from the box's corner at a time."""
    assert 1 <= max_extent <= 64
    P = np.asarray(points, f32).reshape(-1, 3)
    n = len(P)
    g = np.zeros(n, f32) if grey is None else np.asarray(grey, np.uint8).astype(f32)
    fx, fy, iw, usable = project(P, v)
    acc = np.zeros((v.h, v.w), u64)
    counts = np.zeros(3, u32)
    tris = triangles(vertex_index, cells) if n and cells.size else []
    rows, corners, ids = [], [], []
    for k in (range(len(tris)) if order is None else order):
        tid, tri = tris[k]
        slot, s = setup(tri, n, fx, fy, usable, 256 * max_extent, v.w, v.h)
        if slot is not None:
            counts[slot] += 1
        if s is not None:
            rows.append(s), corners.append(tri), ids.append(tid)
    T = np.array(rows, i64).reshape(-1, 12)            # px qx rx py qy ry |A| sign x0 x1 y0 y1
    corners, ids = np.array(corners, i64).reshape(-1, 3), np.array(ids, i64)
    x0, x1, y0, y1 = T[:, 8], T[:, 9], T[:, 10], T[:, 11]
    for dy in range(int((y1 - y0).max()) + 1 if len(T) else 0):
        for dx in range(int((x1 - x0).max()) + 1):
            at = np.nonzero((x0 + dx <= x1) & (y0 + dy <= y1))[0]
            if not len(at):
                continue
            px, py = x0[at] + dx, y0[at] + dy
            ep, eq, er = edges_at(T[at], px * 256, py * 256)
            cov = (ep >= 0) & (eq >= 0) & (er >= 0)
            if not cov.any():
                continue
            at, px, py = at[cov], px[cov], py[cov]
            lp, lq, lr = weights(ep[cov], eq[cov], er[cov], T[at, 6])
            vv = ((lp * iw[corners[at, 0]]) + (lq * iw[corners[at, 1]])) + (lr * iw[corners[at, 2]])
            assert vv.dtype == f32 and (vv > 0).all() and (vv.view(u32) >= 0x00800000).all()      # positive, never subnormal, no NaN
            key = (vv.view(u32).astype(u64) << u64(32)) | (u64(0xFFFFFFFF) - ids[at].astype(u64))
            np.maximum.at(acc, (py, px), key)             # what atomicMax leaves, whatever the order
            if on_cover:
                on_cover(ids[at], px, py, vv)
    # resolve
    hit = acc != 0
    vbits = (acc >> u64(32)).astype(u32)
    won = (u64(0xFFFFFFFF) - (acc & u64(0xFFFFFFFF))).astype(u32)
    depth = np.full((v.h, v.w), INVALID_BITS, u32)
    with np.errstate(all="ignore"):
        depth[hit] = (f32(1.0) / vbits[hit].view(f32)).view(u32)
    triangle = np.where(hit, won, NONE).astype(u32)
    shade = np.zeros((v.h, v.w), np.uint8)
    if hit.any():
        row_of = {int(t): k for k, t in enumerate(ids)}
        py, px = np.nonzero(hit)
        at = np.array([row_of[int(t)] for t in won[py, px]], i64)
        lp, lq, lr = weights(*edges_at(T[at], px * 256, py * 256), T[at, 6])
        val = ((lp * g[corners[at, 0]]) + (lq * g[corners[at, 1]])) + (lr * g[corners[at, 2]])
        assert val.dtype == f32
        shade[py, px] = np.clip(np.floor(val + f32(0.5)), 0, 255).astype(np.uint8)
    return dict(depth=depth, triangle=triangle, shade=shade, counts=counts)


def residual(image, shade, depth_bits):
    """ssrlcv_hip_image_residual -> uint32 bits (h, w)"""
    out = (np.asarray(image, np.uint8).astype(f32) - np.asarray(shade, np.uint8).astype(f32)).view(u32).copy()
    out[depth_bits == INVALID_BITS] = INVALID_BITS
    return out


def stats(res_bits):
    """what pipeline.surface_photo_check reports of a residual map, in float64 on the host -> dict coverage, median, nmad, rms.  The
    quantiles are the lower ones of ssrlcv_hip_difference_stats: rank (m - 1) / 2 of the sorted values."""
    valid = res_bits != INVALID_BITS
    x = np.sort(res_bits[valid].view(f32).astype(np.float64))
    m = len(x)
    if m == 0:
        return dict(coverage=0.0, median=float("nan"), nmad=float("nan"), rms=float("nan"))
    med = x[(m - 1) // 2]
    dev = np.sort(np.abs((x.astype(f32) - f32(med)).astype(np.float64)))
    return dict(coverage=m / res_bits.size, median=float(med), nmad=1.4826 * float(dev[(m - 1) // 2]), rms=float(np.sqrt((x * x).sum() / m)))
