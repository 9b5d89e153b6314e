"""Float64 numpy restatement of the fundamental-matrix RANSAC conventions of include/ssrlcv_hip.h (sample hash,
normalisation, 7-point solver, Sampson test, least-squares refit, pose from F) and the synthetic two-view scene the
tests recover.  The reference holds no fixture for this path (parity unpinned): the GPU is held to this file, and this
file to the synthetic ground truth (tests/test_ransac_host.py)."""
import numpy as np

import helpers as H

M64 = (1 << 64) - 1


def sample_indices(seed, h, n):
    """the 7 distinct match indices of sample h, or None after 64 draws"""
    out = []
    for j in range(64):
        z = (seed + ((h << 32) + j + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        i = ((z >> 32) * n) >> 32
        if i not in out:
            out.append(i)
            if len(out) == 7:
                return out
    return None


def draws_needed(seed, samples, n, cap=128):
    """-> int array[samples]: the draw (1-based) on which sample h gets its 7th distinct index, 0 if not within `cap`
    draws (the contract stops at 64).  The hash of sample_indices vectorised; n <= 64 (the seen set is a bit mask)."""
    assert 7 <= n <= 64
    with np.errstate(over="ignore"):
        h = np.arange(samples, dtype=np.uint64)[:, None]
        j = np.arange(cap, dtype=np.uint64)[None, :]
        z = np.uint64(seed) + ((h << np.uint64(32)) + j + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        idx = ((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)
    seen = np.zeros(samples, np.uint64)
    got = np.zeros(samples, np.int64)
    done = np.zeros(samples, np.int64)
    for d in range(cap):
        bit = np.uint64(1) << idx[:, d]
        new = (seen & bit) == 0
        seen |= bit
        got += new
        done[(got == 7) & (done == 0)] = d + 1
    return done


def split(matches):
    q = matches["kp0_loc"].astype(np.float64)
    t = matches["kp1_loc"].astype(np.float64)
    return q, t, matches["invalid"] == 0


def normalisation(q, t, valid):
    """-> (cq, ct, s): centres of the two bounding boxes of the valid locations, common scale 2 / largest extent"""
    qv, tv = q[valid], t[valid]
    lo_q, hi_q, lo_t, hi_t = qv.min(0), qv.max(0), tv.min(0), tv.max(0)
    ext = max((hi_q - lo_q).max(), (hi_t - lo_t).max())
    return 0.5 * (lo_q + hi_q), 0.5 * (lo_t + hi_t), 2.0 / ext


def T_of(c, s):
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def to_pixel(Fn, cq, ct, s):
    F = T_of(ct, s).T @ Fn @ T_of(cq, s)
    F = F / np.linalg.norm(F)
    f = F.reshape(-1)
    return F * (1.0 if f[np.argmax(np.abs(f))] >= 0 else -1.0)


def to_normalised(F, cq, ct, s):
    Fn = np.linalg.inv(T_of(ct, s)).T @ np.asarray(F, np.float64).reshape(3, 3) @ np.linalg.inv(T_of(cq, s))
    n = np.linalg.norm(Fn)
    return Fn / n if n > 0 else Fn


def rows(q, t):
    x, y, u, v = q[:, 0], q[:, 1], t[:, 0], t[:, 1]
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)


def householder_null(A):
    """-> (F1, F2): the null-space pair of the 7x9 system as the kernel builds it: Householder reflections from the right,
    A H_0 ... H_6 = [L | 0], F1 = H_0 ... H_6 e_7, F2 = H_0 ... H_6 e_8 (the basis fixes what "ascending roots" orders)"""
    A = np.array(A, np.float64)
    V = np.zeros((7, 9))
    for k in range(7):
        nrm = np.sqrt(np.sum(A[k, k:] ** 2))
        if nrm == 0:
            continue
        V[k, k:] = A[k, k:]
        V[k, k] += -nrm if A[k, k] < 0 else nrm
        vv = np.sum(V[k, k:] ** 2)
        A[k:, k:] -= np.outer(2 * (A[k:, k:] @ V[k, k:]) / vv, V[k, k:])
        V[k] /= np.sqrt(vv)
    N = np.eye(9)[7:].copy()
    for k in range(6, -1, -1):
        N -= 2 * np.outer(N @ V[k], V[k])
    return N[0].reshape(3, 3), N[1].reshape(3, 3)


def solve7(qn, tn, householder=False):
    """-> (list of normalised F, near_double_root): real roots of det(a F1 + (1 - a) F2) in ascending order; F1, F2 the
    last two right singular vectors, or with `householder` the kernel's own basis (householder_null)"""
    if householder:
        F1, F2 = householder_null(rows(qn, tn))
    else:
        _, _, vt = np.linalg.svd(rows(qn, tn))
        F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    d = [np.linalg.det(F2 + a * (F1 - F2)) for a in (0.0, 1.0, -1.0, 2.0)]
    c0, c2 = d[0], 0.5 * (d[1] + d[2]) - d[0]
    c3 = (d[3] - 4 * c2 - c0 - (d[1] - d[2])) / 6
    c1 = 0.5 * (d[1] - d[2]) - c3
    big = max(abs(c0), abs(c1), abs(c2), abs(c3))
    near = False
    if abs(c3) <= 1e-12 * big:
        r = np.roots([c2, c1, c0]) if abs(c2) > 1e-12 * big else np.roots([c1, c0])
        roots = sorted(x.real for x in r if abs(x.imag) == 0)
    else:
        a, b, c = c2 / c3, c1 / c3, c0 / c3
        Q, R = (a * a - 3 * b) / 9, (2 * a ** 3 - 9 * a * b + 27 * c) / 54
        near = abs(R * R - Q ** 3) <= 1e-6 * max(R * R, abs(Q ** 3))
        roots = sorted(x.real for x in np.roots([1, a, b, c]) if abs(x.imag) <= 1e-9 * (1 + abs(x)))
    return [r * F1 + (1 - r) * F2 for r in roots], near


def sampson_d2(F, q, t):
    F = np.asarray(F, np.float64).reshape(3, 3)
    qh = np.concatenate([q, np.ones((len(q), 1))], 1)
    th = np.concatenate([t, np.ones((len(t), 1))], 1)
    Fq, Ft = qh @ F.T, th @ F
    r = np.sum(th * Fq, 1)
    den = Fq[:, 0] ** 2 + Fq[:, 1] ** 2 + Ft[:, 0] ** 2 + Ft[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, r * r / den, np.inf)


def inliers(F, q, t, valid, thr):
    return (sampson_d2(F, q, t) < thr * thr) & valid


def rank2(F):
    u, s, vt = np.linalg.svd(F)
    return u @ np.diag([s[0], s[1], 0.0]) @ vt


def ransac(matches, samples, thr, seed=0):
    """-> (pixel F, inlier mask) by the library's conventions, all in float64"""
    q, t, valid = split(matches)
    cq, ct, s = normalisation(q, t, valid)
    qn, tn = (q - cq) * s, (t - ct) * s
    best, best_count = None, 0
    for h in range(samples):
        idx = sample_indices(seed, h, len(matches))
        if idx is None or not valid[idx].all():
            continue
        for Fn in solve7(qn[idx], tn[idx])[0]:
            F = to_pixel(Fn, cq, ct, s)
            c = int(inliers(F, q, t, valid, thr).sum())
            if c > best_count:
                best, best_count = F, c
    if best is None:
        return np.zeros((3, 3)), np.zeros(len(matches), bool)
    m = inliers(best, q, t, valid, thr)
    _, _, vt = np.linalg.svd(rows(qn[m], tn[m]))
    refit = to_pixel(rank2(vt[8].reshape(3, 3)), cq, ct, s)
    mr = inliers(refit, q, t, valid, thr)
    return (refit, mr) if mr.sum() >= m.sum() else (best, m)


def best_slot(counts):
    """-> (slot, count): the lowest slot with the largest count; (None, 0) when every count is 0 (no best)"""
    counts = np.asarray(counts)
    c = int(counts.max()) if len(counts) else 0
    return (int(np.argmax(counts)), c) if c > 0 else (None, 0)


def refit(matches, mask):
    """the contract's refit of the masked matches: the 9x9 normal matrix A^T A in normalised coordinates, the
    eigenvector of its smallest eigenvalue, rank 2 through the 3x3 SVD, back to pixels (ransac() states it by SVD)"""
    q, t, valid = split(matches)
    cq, ct, s = normalisation(q, t, valid)
    m = np.asarray(mask, bool) & valid
    A = rows((q[m] - cq) * s, (t[m] - ct) * s)
    _, V = np.linalg.eigh(A.T @ A)
    return to_pixel(rank2(V[:, 0].reshape(3, 3)), cq, ct, s)


def sampson_gap(Fa, Fb, q, t):
    """max over the matches of | Sampson distance under Fa - under Fb | in pixels (float64)"""
    return float(np.max(np.abs(np.sqrt(sampson_d2(Fa, q, t)) - np.sqrt(sampson_d2(Fb, q, t)))))


# ------------------------------------------------------------------ camera model of pose_residual (csrc/pose.hip)
def rot(a):
    x, y, z = a
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], [-sy, cy * sx, cy * cx]])


def K_of(cam):
    c = np.asarray(cam).reshape(-1)[0]
    return np.array([[c["foc"] / c["dpix"][0], 0, c["size"][0] / 2.0], [0, c["foc"] / c["dpix"][1], c["size"][1] / 2.0],
                     [0, 0, 1]], np.float64)


def F_of_pose(Rp, C, Kq, Kt):
    """F of a target camera with rotation Rp (target ray -> query frame) and centre C in the query frame"""
    R, tt = Rp.T, -Rp.T @ C
    tx = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]])
    return np.linalg.inv(Kt).T @ tx @ R @ np.linalg.inv(Kq)


def F_of_cameras(cams):
    """F between the two cameras of a fixture (world rotations cam_rot, positions cam_pos)"""
    R0, R1 = rot(cams["cam_rot"][0].astype(np.float64)), rot(cams["cam_rot"][1].astype(np.float64))
    C = R0.T @ (cams["cam_pos"][1].astype(np.float64) - cams["cam_pos"][0].astype(np.float64))
    return F_of_pose(R0.T @ R1, C, K_of(cams[0:1]), K_of(cams[1:2]))


def pose_from_F(F, q, t, use, Kq, Kt):
    """-> (Rp, unit C) of the four decompositions of E = Kt^T F Kq, the one with most positive depth pairs"""
    E = Kt.T @ np.asarray(F, np.float64).reshape(3, 3) @ Kq
    u, _, vt = np.linalg.svd(E)
    if np.linalg.det(u) < 0:
        u = -u
    if np.linalg.det(vt) < 0:
        vt = -vt
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    qr = (np.linalg.inv(Kq) @ np.concatenate([q[use], np.ones((use.sum(), 1))], 1).T).T
    tr = (np.linalg.inv(Kt) @ np.concatenate([t[use], np.ones((use.sum(), 1))], 1).T).T
    best, votes = None, -1
    for R in (u @ W @ vt, u @ W.T @ vt):
        for sgn in (1.0, -1.0):
            Rp, C = R.T, -R.T @ (sgn * u[:, 2])
            d2 = tr @ Rp.T
            a, b, c = np.sum(qr * qr, 1), np.sum(qr * d2, 1), np.sum(d2 * d2, 1)
            e, f = qr @ C, d2 @ C
            det = b * b - a * c
            lq, lt = (b * f - c * e) / det, (a * f - b * e) / det
            v = int(np.sum((lq > 0) & (lt > 0)))
            if v > votes:
                best, votes = (Rp, C / np.linalg.norm(C)), v
    return best


def axis_rotations(R):
    """getAxisRotations (host/matrix_util.hpp) in float64: (roll, pitch, yaw) of R = rot((roll, pitch, yaw))"""
    x = np.arctan2(R[2, 1], R[2, 2])
    return np.array([x, np.arctan2(-R[2, 0], R[2, 2] / np.cos(x)), np.arctan2(R[1, 0], R[0, 0])])


def pose6(F, matches, mask, cams):
    """the whole output of ssrlcv_hip_pose_from_fmatrix in float64: pose_from_F over the valid matches with mask != 0
    (mask None: every valid match), getAxisRotations of Rp, unit C times |target.cam_pos - query.cam_pos| / 1000"""
    q, t, valid = split(matches)
    use = valid if mask is None else valid & (np.asarray(mask) != 0)
    Rp, C = pose_from_F(F, q, t, use, K_of(cams[0:1]), K_of(cams[1:2]))
    d = cams["cam_pos"][1].astype(np.float64) - cams["cam_pos"][0].astype(np.float64)
    return np.concatenate([axis_rotations(Rp), C * np.linalg.norm(d) / 1000.0])


def rotation_error_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def angle_deg(a, b):
    return np.degrees(np.arccos(np.clip(np.dot(a, b) / np.linalg.norm(a) / np.linalg.norm(b), -1, 1)))


# ------------------------------------------------------------------ synthetic two-view scene
TRUE_ANGLES = np.array([0.10, -0.10, 0.08])  # roll, pitch, yaw: about 9.3 degrees
TRUE_C = np.array([3.6, 0.9, 1.2])           # baseline ~3.9 against a mean depth of 20: about 1/5
# the poses the pose tests recover: (roll, pitch, yaw), target centre C in the query frame
POSES = {"default": (TRUE_ANGLES, TRUE_C), "yaw": ((0.10, -0.10, 2.5), TRUE_C), "pitch": ((0.10, -0.6, 0.08), TRUE_C),
         "forward": (TRUE_ANGLES, (0.0, 0.0, 3.0)), "backward": (TRUE_ANGLES, (0.0, 0.0, -3.0)),
         "sideways": (TRUE_ANGLES, (4.0, 0.0, 0.0)), "vertical": (TRUE_ANGLES, (0.0, 4.0, 0.0)),
         "short": (TRUE_ANGLES, 0.2 * TRUE_C / np.linalg.norm(TRUE_C))}  # a baseline of 1/100 of the mean depth


def synthetic_cameras(C=TRUE_C):
    cams = np.zeros(2, H.CAMERA)
    f_pix = 2048.0 / np.tan(np.radians(20.0))  # 4096 px across 40 degrees
    cams["foc"] = 0.05
    cams["dpix"] = 0.05 / f_pix
    cams["fov"] = np.radians(40.0)
    cams["size"] = 4096
    cams["cam_pos"][1] = 1000.0 * np.asarray(C)  # LM_optimize's unit: the pose position is 1/1000 of the cameras'
    return cams


def synthetic(n, seed=1, outliers=0.4, noise=0.5, angles=TRUE_ANGLES, C=TRUE_C):
    """-> (MATCH[n], cameras, truth dict(Rp, C, inlier)): points with depth 10..30 seen by both cameras, 0.5 px noise,
    a fraction `outliers` of the target locations replaced by uniform ones; the target camera has rotation
    rot(angles) and centre C in the query frame"""
    rng = np.random.default_rng(seed)
    C = np.asarray(C, np.float64)
    cams = synthetic_cameras(C)
    Kq, Kt = K_of(cams[0:1]), K_of(cams[1:2])
    Rp = rot(np.asarray(angles, np.float64))
    q_all, t_all = np.zeros((0, 2)), np.zeros((0, 2))
    while len(q_all) < n:
        m = 2 * n + 64
        z = rng.uniform(10.0, 30.0, m)
        X = np.stack([rng.uniform(-1, 1, m) * z * 0.4, rng.uniform(-1, 1, m) * z * 0.4, z], 1)
        Xt = (X - C) @ Rp  # Rp^T (X - C)
        ok = Xt[:, 2] > 0
        qh, th = X @ Kq.T, Xt @ Kt.T
        q, t = qh[:, :2] / qh[:, 2:], th[:, :2] / th[:, 2:]
        ok &= np.all((q >= 0) & (q < 4096) & (t >= 0) & (t < 4096), 1)
        q_all, t_all = np.concatenate([q_all, q[ok]]), np.concatenate([t_all, t[ok]])
    q, t = q_all[:n] + rng.normal(0, noise, (n, 2)), t_all[:n] + rng.normal(0, noise, (n, 2))
    bad = rng.random(n) < outliers
    t[bad] = rng.uniform(0, 4096, (int(bad.sum()), 2))
    mt = np.zeros(n, H.MATCH)
    mt["kp0_loc"], mt["kp1_loc"] = q.astype(np.float32), t.astype(np.float32)
    mt["kp0_parent"], mt["kp1_parent"] = 0, 1
    return mt, cams, {"Rp": Rp, "C": C.copy(), "inlier": ~bad}
