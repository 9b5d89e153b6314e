"""The contract of include/ssrlcv_hip.h "surface registration" restated in numpy, operation by operation.  The per-point part is
float32 element-wise numpy, every operation the IEEE one; the lookup is dsm_ref.locate and accuracy_ref.difference on the posed
points, the slopes are read from the same corners; the 36 sums are accuracy_ref.shaped_sum, float64 products of float32 values
being exact.  tests/test_gpu_register.py holds csrc/register.hip to it bit for bit, and tests/test_register_cases.py proves on it
alone that the cases test something.  The host steps (solve, compose) and the loop of pipeline.surface_register are restated in
float64."""
import numpy as np

import accuracy_ref as A
import dsm_ref as D
import mesh_ref as M

f32 = np.float32
TILE = A.TILE
INF = float("inf")

POSE = np.dtype([("m", "<f4", (12,)), ("pivot", "<f4", (3,))])
RECORD = np.dtype([("n", "<u4"), ("inside", "<u4"), ("used", "<u4"), ("reserved", "<u4"), ("jtj", "<f8", (28,)), ("jte", "<f8", (7,)), ("ee", "<f8")])
assert POSE.itemsize == 60 and RECORD.itemsize == 304
PAIRS = [(i, j) for i in range(7) for j in range(i, 7)]     # the order of jtj
DOF = {"shift": 0x07, "rigid": 0x3F, "similarity": 0x7F}


def pose(matrix=None, translation=(0, 0, 0), pivot=(0, 0, 0)):
    """-> a POSE scalar: p' = matrix p + translation"""
    g = np.zeros((), POSE)
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = np.eye(3) if matrix is None else np.asarray(matrix, np.float64)
    m[:, 3] = translation
    g["m"], g["pivot"] = m.reshape(12), np.asarray(pivot, np.float32)
    return g


def skipped(p):
    """the rasterize rule: a component that is not finite, or (0, 0, 0) with either sign of zero"""
    return ~np.isfinite(p).all(1) | (p == 0).all(1)


def transform(points, g):
    """item 2 -> float32 (n, 3): the row expression; a skipped point is copied bit for bit"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    m = np.asarray(g["m"], np.float32)
    out = p.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = (((m[4 * r] * p[:, 0]) + (m[4 * r + 1] * p[:, 1])) + (m[4 * r + 2] * p[:, 2])) + m[4 * r + 3]
    skip = skipped(p)
    out.view(np.uint32)[skip] = p.view(np.uint32)[skip]
    return out


def slopes(posed, height, fr, cells):
    """-> (rs, rt, kind) of the triangle under every posed point: kind 0..3 = a-d T0, a-d T1, b-c T0, b-c T1, -1 outside the mesh.
    The same corners as accuracy_ref.difference reads"""
    n = len(posed)
    rs, rt, kind = np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, -1, np.int64)
    if fr.w < 2 or fr.h < 2:
        return rs, rt, kind
    hf = np.ascontiguousarray(height, np.float32).reshape(fr.h, fr.w)
    cells = np.asarray(cells, np.uint8).reshape(fr.h - 1, fr.w - 1)
    loc = D.locate(posed, fr)
    with np.errstate(all="ignore"):
        uu, vv = loc["u"] - f32(0.5), loc["v"] - f32(0.5)
        fi, fj = np.floor(uu), np.floor(vv)
        inside = ~skipped(posed) & np.isfinite(loc["z"]) & (fi >= 0) & (fi < f32(fr.w - 1)) & (fj >= 0) & (fj < f32(fr.h - 1))
        idx = np.nonzero(inside)[0]
        i, j = fi[idx].astype(np.int64), fj[idx].astype(np.int64)
        s, t = (uu[idx] - fi[idx]).astype(np.float32), (vv[idx] - fj[idx]).astype(np.float32)
        za, zb, zc, zd = hf[j, i], hf[j, i + 1], hf[j + 1, i], hf[j + 1, i + 1]
        bc = (cells[j, i] & 4) != 0
        first = np.where(bc, (s + t) <= f32(1), t >= s)
        k = np.where(bc, 2, 0) + np.where(first, 0, 1)
        rs[idx] = np.choose(k, [zd - zc, zb - za, zb - za, zd - zc])
        rt[idx] = np.choose(k, [zc - za, zd - zb, zc - za, zd - zb])
        kind[idx] = k
    return rs, rt, kind


def rows(points, g, height, fr, cells, center=0.0, gate=INF):
    """item 1 per point -> dict(posed, d, kind, G, J float32 (n, 7), e, inside, used)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    q = transform(p, g)
    with np.errstate(all="ignore"):
        d = A.difference(q, height, fr, cells)
        d.view(np.uint32)[skipped(p)] = D.INVALID_BITS          # a skipped p has no p'
        inside = D.bits(d) != D.INVALID_BITS
        rs, rt, kind = slopes(q, height, fr, cells)
        gu, gv = rs / fr.cell, rt / fr.cell
        G = np.stack([(fr.ez[k] - (gu * fr.ex[k])) - (gv * fr.ey[k]) for k in range(3)], 1).astype(np.float32)
        length = np.sqrt(((G[:, 0] * G[:, 0]) + (G[:, 1] * G[:, 1])) + (G[:, 2] * G[:, 2]))
        N = G / length[:, None]
        e = d / length
        L = q - np.asarray(g["pivot"], np.float32)[None, :]
        J = np.empty((len(p), 7), np.float32)
        J[:, :3] = N
        J[:, 3] = (L[:, 1] * N[:, 2]) - (L[:, 2] * N[:, 1])
        J[:, 4] = (L[:, 2] * N[:, 0]) - (L[:, 0] * N[:, 2])
        J[:, 5] = (L[:, 0] * N[:, 1]) - (L[:, 1] * N[:, 0])
        J[:, 6] = ((L[:, 0] * N[:, 0]) + (L[:, 1] * N[:, 1])) + (L[:, 2] * N[:, 2])
        used = inside & (np.abs(d - f32(center)) <= f32(gate)) & np.isfinite(J).all(1) & np.isfinite(e)
    return dict(posed=q, d=d, kind=np.where(inside, kind, -1), G=G, J=J, e=e, inside=inside, used=used)


def _shaped(index, values, n):
    """the contract's sum of an array of n entries that is +0.0 except values at index: only the tiles that hold an entry are
    summed in full -- a tile of +0.0 sums to +0.0 -- and the tile sums go through the same shape again"""
    tiles = (n + TILE - 1) // TILE
    sums = np.zeros(tiles, np.float64)
    tile = index // TILE
    for t in np.unique(tile):
        dense = np.zeros(TILE, np.float64)
        sel = tile == t
        dense[index[sel] - t * TILE] = values[sel]
        sums[t] = A.shaped_sum(dense)
    return sums[0] if tiles == 1 else A.shaped_sum(sums)


def terms(points, g, height, fr, cells, center=0.0, gate=INF):
    """item 1 -> a RECORD scalar.  Only the points that are not skipped are looked at (n may be 2^24 and more)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros((), RECORD)
    n = len(p)
    if n == 0:
        return rec
    keep = np.nonzero(~skipped(p))[0]
    r = rows(p[keep], g, height, fr, cells, center, gate)
    rec["n"], rec["inside"], rec["used"] = n, int(r["inside"].sum()), int(r["used"].sum())
    index = keep[r["used"]]
    J, e = r["J"][r["used"]].astype(np.float64), r["e"][r["used"]].astype(np.float64)
    rec["jtj"] = [_shaped(index, J[:, i] * J[:, j], n) for (i, j) in PAIRS]
    rec["jte"] = [_shaped(index, J[:, i] * e, n) for i in range(7)]
    rec["ee"] = _shaped(index, e * e, n)
    return rec


# ---- the host steps, in float64
def normal_matrix(rec, damping=0.0):
    H = np.zeros((7, 7), np.float64)
    for k, (i, j) in enumerate(PAIRS):
        H[i, j] = H[j, i] = rec["jtj"][k]
    H[np.diag_indices(7)] *= 1.0 + damping
    return H


def step(rec, mask, damping=0.0):
    """-> delta float64 (7,): H delta = -jte over the masked unknowns by numpy.linalg.solve; None where the system has no answer"""
    idx = [k for k in range(7) if mask >> k & 1]
    if int(rec["used"]) == 0:
        return None
    H = normal_matrix(rec, damping)[np.ix_(idx, idx)]
    if not (np.diag(H) > 0).all() or np.linalg.cond(H) > 2.0 ** 30:
        return None
    delta = np.zeros(7, np.float64)
    delta[idx] = np.linalg.solve(H, -np.asarray(rec["jte"], np.float64)[idx])
    return delta


def rotation(w):
    """the exact rotation of a rotation vector (Rodrigues)"""
    w = np.asarray(w, np.float64)
    theta = np.sqrt(w @ w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    a, b = (1.0, 0.5) if theta < 2.0 ** -26 else (np.sin(theta) / theta, 0.5 * (np.sin(theta / 2) / (theta / 2)) ** 2)
    return np.eye(3) + a * K + b * (K @ K)


def compose64(g, delta):
    """-> (M float64 (3, 3), T float64 (3,)) of the pose after the step p'' = pivot + (1 + ds) R(dw) (p' - pivot) + dt, unrounded"""
    m = np.asarray(g["m"], np.float64).reshape(3, 4)
    c = np.asarray(g["pivot"], np.float64)
    sR = (1.0 + delta[6]) * rotation(delta[3:6])
    return sR @ m[:, :3], c + sR @ (m[:, 3] - c) + np.asarray(delta[:3], np.float64)


def compose(g, delta):
    Mx, T = compose64(g, delta)
    out = pose(Mx, T, g["pivot"])
    return out


def apply64(g, p):
    m = np.asarray(g["m"], np.float64).reshape(3, 4)
    return np.asarray(p, np.float64) @ m[:, :3].T + m[:, 3]


def box_corners(points):
    """the 8 corners of the bounding box of the points the skip rule keeps, float64 (8, 3); (0, 3) without a point"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    p = p[~skipped(p)].astype(np.float64)
    if len(p) == 0:
        return np.zeros((0, 3))
    lo, hi = p.min(0), p.max(0)
    return np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)


def moved(before, after, corners):
    """the largest displacement of a corner between two poses"""
    if len(corners) == 0:
        return 0.0
    return float(np.sqrt(((apply64(after, corners) - apply64(before, corners)) ** 2).sum(1)).max())


def gate_of(d, factor):
    """-> (center, gate) float32 from the differences: the lower median and factor x NMAD; None without a finite difference"""
    signed = A.stats(d, quantiles=(5000,))
    if int(signed["finite"]) == 0:
        return None
    center = f32(signed["quantile"][0])
    mad = A.stats(d, center=center, absolute=True, quantiles=(5000,))["quantile"][0]
    return center, f32(np.float64(factor) * (np.float64(1.4826) * np.float64(mad)))


def register(points, height, fr, max_jump=None, dof="rigid", iterations=8, gate=3.0, initial=None, damping=0.0, tolerance=1e-3):
    """pipeline.surface_register restated -> dict(pose, converged, history)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    mask = DOF.get(dof, dof)
    cells = M.mesh(height, 1, INF if max_jump is None else max_jump)[1]
    g = pose() if initial is None else initial.copy()
    q = transform(p, g)
    has = D.bits(A.difference(q, height, fr, cells)) != D.INVALID_BITS
    has &= ~skipped(p)
    g["pivot"] = q[has].astype(np.float64).mean(0).astype(np.float32) if has.any() else 0
    corners, history, converged = box_corners(p), [], False
    for _ in range(iterations):
        center, width = f32(0), f32(INF)
        if gate is not None:
            d = A.difference(transform(p, g), height, fr, cells)
            d.view(np.uint32)[skipped(p)] = D.INVALID_BITS
            cg = gate_of(d, gate)
            if cg is None:
                break
            center, width = cg
        rec = terms(p, g, height, fr, cells, center, width)
        delta = step(rec, mask, damping)
        used = int(rec["used"])
        history.append(dict(used=used, inside=int(rec["inside"]), rms=float(np.sqrt(rec["ee"] / used)) if used else float("nan"), center=float(center),
                            gate=float(width), delta=None if delta is None else delta.tolist(), terms=rec))
        if delta is None:
            break
        nxt = compose(g, delta)
        small = moved(g, nxt, corners) <= tolerance * float(fr.cell)
        g = nxt
        if small:
            converged = True
            break
    return dict(pose=g, converged=converged, history=history)
