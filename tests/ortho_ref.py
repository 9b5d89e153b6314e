"""The contract of include/ssrlcv_hip.h "ortho-image" restated in numpy, operation by operation.  Every float32 element-wise
operation of numpy is the IEEE one, so this is exact: tests/test_gpu_ortho.py holds csrc/ortho.hip to it byte for byte, and
tests/test_ortho_cases.py proves on it alone that the cases of tests/ortho_cases.py test something.  The march runs on all cells
at once, a step at a time, with the cells still marching as a mask; no early stop, no batches: the plain form."""
from collections import namedtuple

import numpy as np

from dsm_ref import INVALID_BITS, bits, frame  # noqa: F401  (frame: the cases build theirs through this module)

f32 = np.float32
FIRST, MEDIAN = 0, 1
NO_VIEW = np.uint8(0xFF)

View = namedtuple("View", "image M pos eye")   # image uint8 (h, w); M float32 (9,); pos, eye float32 (3,)


def view(image, M, pos, eye):
    return View(np.ascontiguousarray(image, np.uint8), np.asarray(M, np.float32).reshape(9).copy(), np.asarray(pos, np.float32).reshape(3).copy(),
                np.asarray(eye, np.float32).reshape(3).copy())


def euler_matrix(rot):
    """rotatePoint's matrix Rz(z) Ry(y) Rx(x) in float64 of float32 angles"""
    x, y, z = (float(f32(a)) for a in rot)
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx], [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], np.float64)


def view_of_camera(cam, fr):
    """ssrlcv_dsm_ortho_view_host in float64 -> (M (9,), pos (3,), eye (3,)) float64, before the rounding to float32.  cam: one
    helpers.CAMERA record"""
    foc, fovx = float(cam["foc"]), float(cam["fov"][0])
    sx, sy = float(cam["size"][0]), float(cam["size"][1])
    dpix = foc * np.tan(fovx / 2.0) / (sx / 2.0)
    fpx = foc / dpix
    K = np.array([[fpx, 0, sx / 2.0], [0, fpx, sy / 2.0], [0, 0, 1.0]])
    Rt = euler_matrix(cam["cam_rot"]).T
    M = np.array([[K[i][0] * Rt[0][j] + K[i][1] * Rt[1][j] + K[i][2] * Rt[2][j] for j in range(3)] for i in range(3)])   # the builder's order
    pos = np.asarray(cam["cam_pos"], np.float64)
    q = pos - fr.origin.astype(np.float64)
    cell = float(fr.cell)
    dot = lambda e: (q[0] * float(e[0]) + q[1] * float(e[1])) + q[2] * float(e[2])  # noqa: E731
    eye = np.array([dot(fr.ex) / cell, dot(fr.ey) / cell, dot(fr.ez)])
    return M.reshape(9), pos, eye


def bilinear(image, sx, sy):
    """the sample of ssrlcv_hip_warp_homography_u8 (tests/rectify_ref.py warp_ref) at float32 positions inside the image"""
    sh, sw = image.shape
    sx = np.minimum(np.maximum(sx, f32(0)), f32(sw - 1))
    sy = np.minimum(np.maximum(sy, f32(0)), f32(sh - 1))
    x0 = np.minimum(np.floor(sx).astype(np.int64), max(sw - 2, 0))
    y0 = np.minimum(np.floor(sy).astype(np.int64), max(sh - 2, 0))
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    fx, fy = sx - x0.astype(f32), sy - y0.astype(f32)
    S = image.astype(f32)
    a, b, c, d = S[y0, x0], S[y0, x1], S[y1, x0], S[y1, x1]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    v = top + fy * (bot - top)
    assert v.dtype == np.float32
    return np.floor(v + f32(0.5)).astype(np.uint8)


def project(P, v):
    """-> (sx, sy float32, inside bool): MAPPED and INSIDE"""
    h, w = v.image.shape
    with np.errstate(all="ignore"):
        d = [P[k] - v.pos[k] for k in range(3)]
        X = (v.M[0] * d[0] + v.M[1] * d[1]) + v.M[2] * d[2]
        Y = (v.M[3] * d[0] + v.M[4] * d[1]) + v.M[5] * d[2]
        W = (v.M[6] * d[0] + v.M[7] * d[1]) + v.M[8] * d[2]
        sx, sy = X / W, Y / W
        inside = (W > 0) & np.isfinite(sx) & np.isfinite(sy) & (sx >= 0) & (sx <= f32(w - 1)) & (sy >= 0) & (sy <= f32(h - 1))
    assert sx.dtype == np.float32
    return sx, sy, inside


def march(height, ii, jj, z, eye, max_steps, bias):
    """the visibility of cells (ii, jj) of heights z from `eye` -> (visible bool, steps int: the last step a cell's march took)"""
    h, w = height.shape
    hb = bits(height)
    bias = f32(bias)
    n = len(z)
    visible = np.zeros(n, bool)
    steps = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        ci, cj = ii.astype(f32) + f32(0.5), jj.astype(f32) + f32(0.5)
        du, dv, dz = eye[0] - ci, eye[1] - cj, eye[2] - z
        above = dz > 0
        L = np.maximum(np.abs(du), np.abs(dv))
        done = ~above | (L < 1) | (max_steps == 0)
        visible[above & done] = True
        su, sv, sz = du / L, dv / L, dz / L
        s = 0
        while not done.all() and s < max_steps:
            s += 1
            fs = f32(s)
            act = np.nonzero(~done)[0]
            steps[act] = s
            past = fs > L[act]
            u, v, zr = ci[act] + fs * su[act], cj[act] + fs * sv[act], z[act] + fs * sz[act]
            fi, fj = np.floor(u), np.floor(v)
            inside = (fi >= 0) & (fi < f32(w)) & (fj >= 0) & (fj < f32(h))
            leave = past | ~inside
            visible[act[leave]] = True
            done[act[leave]] = True
            act, zr = act[~leave], zr[~leave]
            at = hb[fj[~leave].astype(np.int64), fi[~leave].astype(np.int64)]
            occluded = (at != INVALID_BITS) & (at.view(np.float32) > zr + bias)
            done[act[occluded]] = True
        visible[~done] = True   # out of steps
    return visible, steps


def ortho(height, fr, views, max_steps, bias, rule):
    """-> dict(ortho, seen, which uint8 (h, w); inside, sees bool (m, h, w): the cell projects into view k, view k sees it; steps
    int (m, h, w): the marches' lengths)"""
    height = np.ascontiguousarray(height, np.float32).reshape(fr.h, fr.w)
    m = len(views)
    assert 1 <= m <= 8
    hb = bits(height)
    with np.errstate(all="ignore"):
        valid = (hb != INVALID_BITS) & np.isfinite(height)
    jj, ii = np.nonzero(valid)
    z = height[jj, ii]
    n = len(z)
    sees, within = np.zeros((m, n), bool), np.zeros((m, n), bool)
    grey = np.zeros((m, n), np.uint8)
    steps = np.zeros((m, n), np.int64)
    with np.errstate(all="ignore"):
        a = (ii.astype(f32) + f32(0.5)) * fr.cell
        b = (jj.astype(f32) + f32(0.5)) * fr.cell
        P = [((fr.origin[k] + (a * fr.ex[k])) + (b * fr.ey[k])) + (z * fr.ez[k]) for k in range(3)]
    for k, v in enumerate(views):
        sx, sy, inside = project(P, v)
        within[k] = inside
        idx = np.nonzero(inside)[0]
        vis, st = march(height, ii[idx], jj[idx], z[idx], v.eye, max_steps, bias)
        sees[k, idx], steps[k, idx] = vis, st
        idx = idx[vis]
        grey[k, idx] = bilinear(v.image, sx[idx], sy[idx])
    count = sees.sum(0)
    if rule == FIRST:
        pick = np.argmax(sees, 0)
        chosen = grey[pick, np.arange(n)]
    else:
        ranked = np.sort(np.where(sees, grey.astype(np.int64), 1000), 0)   # the seeing views' bytes first
        chosen = ranked[np.maximum(count - 1, 0) // 2, np.arange(n)].astype(np.uint8)
    has = sees & (grey == chosen[None])
    which = np.where(count > 0, np.argmax(has, 0), 0xFF).astype(np.uint8)
    chosen = np.where(count > 0, chosen, 0).astype(np.uint8)
    out = dict(ortho=np.zeros((fr.h, fr.w), np.uint8), seen=np.zeros((fr.h, fr.w), np.uint8), which=np.full((fr.h, fr.w), NO_VIEW, np.uint8),
               inside=np.zeros((m, fr.h, fr.w), bool), sees=np.zeros((m, fr.h, fr.w), bool), steps=np.zeros((m, fr.h, fr.w), np.int64))
    out["ortho"][jj, ii] = chosen
    out["seen"][jj, ii] = (sees.astype(np.int64) << np.arange(m)[:, None]).sum(0).astype(np.uint8)
    out["which"][jj, ii] = which
    out["inside"][:, jj, ii] = within
    out["sees"][:, jj, ii] = sees
    out["steps"][:, jj, ii] = steps
    return out
