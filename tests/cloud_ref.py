"""numpy restatement of the point-cloud contract of include/ssrlcv_hip.h (ssrlcv_hip_knn, _neighbor_distance_filter,
_point_normals), the reference the GPU tests hold csrc/cloud.hip to.

k-NN: the k points j != i smallest by (d2, j), d2 = (dx*dx + dy*dy) + dz*dz in float32 with dx = p[j] - p[i].  Candidates
come from scipy's cKDTree (float64) with a margin and are re-ranked by the exact float32 key; a row whose margin does not
prove the answer (ties at the edge of the candidate list, or a k-th d2 so small that float32 products underflow and the
float64 distances no longer bound the float32 ones) is redone by brute force.  Without scipy every row is brute force.
Non-finite points get (UINT32_MAX, +inf) rows and are nobody's neighbour.  knn_brute is the contract itself at every
scale: the edge-case tests (tests/cloud_cases.py) use it alone."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))  # scene.py

try:
    from scipy.spatial import cKDTree
except ImportError:  # pragma: no cover - scipy is optional: the chunked brute force answers everything then
    cKDTree = None

NONE = np.uint32(0xFFFFFFFF)
UNDERFLOW_GUARD = np.float32(2.0 ** -100)   # a d2 at or above it has a relative float32 error below 1e-6 (see knn)


def finite_mask(p):
    return np.isfinite(p).all(1)


def d2_f32(q, c):
    """the contract's float32 d2 of queries q [..., 3] to candidates c [..., 3] (broadcast), dx = c - q"""
    q = q.astype(np.float32, copy=False)
    c = c.astype(np.float32, copy=False)
    with np.errstate(over="ignore", under="ignore"):  # +inf and subnormal / zero d2 are inside the contract
        dx, dy, dz = c[..., 0] - q[..., 0], c[..., 1] - q[..., 1], c[..., 2] - q[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def _keys(d2, j):
    """(d2, j) as one uint64 key (d2 >= 0 orders like its bits)"""
    return (d2.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)


def _take_k(keys, k):
    """the k smallest keys of each row, ascending -> (indices uint32, d2 float32)"""
    if keys.shape[1] > k:
        part = np.partition(keys, k - 1, axis=1)[:, :k]
    else:
        part = keys
    part = np.sort(part, axis=1)
    if part.shape[1] < k:  # fewer than k other finite points
        pad = np.full((part.shape[0], k - part.shape[1]), np.uint64(0x7F800000FFFFFFFF), np.uint64)
        part = np.concatenate([part, pad], 1)
    idx = (part & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    d2 = (part >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def knn_brute(p, k, rows=None, chunk=None):
    """plain float32 brute force over all finite points -> (nbr uint32 [len(rows), k], d2 float32)"""
    p = np.ascontiguousarray(p, np.float32)
    fin = np.nonzero(finite_mask(p))[0].astype(np.uint32)
    rows = np.arange(len(p)) if rows is None else np.asarray(rows)
    P = p[fin]
    chunk = chunk or max(1, 2 ** 24 // max(len(fin), 1))
    nbr = np.full((len(rows), k), NONE, np.uint32)
    d2 = np.full((len(rows), k), np.inf, np.float32)
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        ok = finite_mask(p[r])
        if not ok.any():
            continue
        rr = r[ok]
        dd = d2_f32(p[rr][:, None, :], P[None, :, :])
        keys = _keys(dd, np.broadcast_to(fin, dd.shape))
        keys[fin[None, :] == rr[:, None]] = np.uint64(0xFFFFFFFFFFFFFFFF)  # j != i
        i_, d_ = _take_k(keys, k)
        d_[i_ == NONE] = np.inf
        sel = np.nonzero(ok)[0] + a
        nbr[sel], d2[sel] = i_, d_
    return nbr, d2


def knn(p, k, margin=None):
    """the contract's k-NN -> (nbr uint32 [n, k], d2 float32 [n, k])"""
    p = np.ascontiguousarray(p, np.float32)
    n = len(p)
    fin = np.nonzero(finite_mask(p))[0]
    if cKDTree is None or len(fin) <= k + 1:
        return knn_brute(p, k)
    margin = margin if margin is not None else 8 + k // 2
    kq = min(k + 1 + margin, len(fin))
    tree = cKDTree(p[fin].astype(np.float64))
    dist, loc = tree.query(p[fin].astype(np.float64), k=kq, workers=16)
    cand = fin[loc].astype(np.uint32)                                      # [nf, kq] original indices
    dd = d2_f32(p[fin][:, None, :], p[cand])
    keys = _keys(dd, cand)
    keys[cand == fin[:, None].astype(np.uint32)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    nb, d2 = _take_k(keys, k)
    nbr = np.full((n, k), NONE, np.uint32)
    out_d2 = np.full((n, k), np.inf, np.float32)
    nbr[fin], out_d2[fin] = nb, d2
    # proof of the margin: every point outside the candidates is at least as far (float64) as the last candidate; its
    # float32 d2 is within 1e-6 relative of the float64 one WHERE THAT IS AT LEAST 2^-100 (the largest of the three
    # products is then normal, and the two that may be subnormal add at most 2 * 2^-150).  Below, products underflow and
    # the float32 order is no longer the spatial one.  A row whose k-th key is not clearly below the last candidate's
    # distance, or is below 2^-100, is redone.
    if kq < len(fin):
        last = dist[:, -1] ** 2
        unsure = ~(d2[:, -1].astype(np.float64) * (1 + 1e-5) < last * (1 - 1e-5)) | ~(d2[:, -1] >= UNDERFLOW_GUARD)
        if unsure.any():
            bn, bd = knn_brute(p, k, rows=fin[unsure])
            nbr[fin[unsure]], out_d2[fin[unsure]] = bn, bd
    return nbr, out_d2


def mean_distance(d2, k):
    """m_i = (sqrtf(d2_1) + ... + sqrtf(d2_k)) / k, sequential float32"""
    s = np.zeros(len(d2), np.float32)
    for t in range(k):
        s = s + np.sqrt(d2[:, t].astype(np.float32))
    return s / np.float32(k)


def filter_stats(m, sigma):
    """(mu, std, t) in float64 over the finite m_i (population std); all zero when there is none"""
    f = m[np.isfinite(m)].astype(np.float64)
    if len(f) == 0:
        return 0.0, 0.0, 0.0
    mu = f.sum() / len(f)
    std = np.sqrt(((f - mu) ** 2).sum() / len(f))
    return mu, std, mu + sigma * std


def filter_mask(m, t):
    return np.isfinite(m) & (m.astype(np.float64) <= t)


def covariances(p, nbr):
    """the float64 covariance (times k + 1) of every row with a finite centre and k neighbours below n -> (row indices,
    cov [m, 3, 3]); shifted by p_i first, so k + 1 coincident points give exactly zero"""
    p = np.asarray(p, np.float32)
    ok = finite_mask(p) & (nbr < len(p)).all(1)
    idx = np.nonzero(ok)[0]
    P = p.astype(np.float64)
    grp = np.concatenate([P[idx][:, None, :], P[nbr[idx].astype(np.int64)]], 1)   # [m, k + 1, 3]
    grp = grp - P[idx][:, None, :]
    c = grp - grp.mean(1, keepdims=True)
    return idx, np.einsum("mia,mib->mab", c, c)


def normals(p, nbr, k, viewpoint):
    """-> (normals float64 [n, 3] (oriented, (0,0,0) where the contract says so), relative eigengap (l2 - l1) / l3)"""
    p = np.asarray(p, np.float32)
    n = len(p)
    out = np.zeros((n, 3))
    gap = np.zeros(n)
    idx, cov = covariances(p, nbr)
    if len(idx) == 0:
        return out, gap
    P = p.astype(np.float64)
    w, v = np.linalg.eigh(cov)
    e = v[:, :, 0]
    vp = np.asarray(viewpoint, np.float64)
    sgn = np.where(((vp - P[idx]) * e).sum(1) < 0, -1.0, 1.0)
    e = e * sgn[:, None]
    zero = np.abs(cov).sum((1, 2)) == 0
    e[zero] = 0
    out[idx] = e
    with np.errstate(divide="ignore", invalid="ignore"):
        gap[idx] = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return out, gap


# ---------------------------------------------------------------- synthetic clouds
def terrain_cloud(n, outlier_frac=0.01, seed=5, ecef=True, device=None):
    """n points on the tools/scene.py terrain patch (km; at the fixture's ECEF offset when `ecef`), a fraction of them
    displaced along the vertical by 1-5 km (either sign) -> (points float32 [n, 3], outlier bool [n], up vector)"""
    import torch
    import scene
    rng = np.random.default_rng(seed)
    dev = torch.device(device or "cpu")
    sc = scene.Scene(64, 0.01, device=dev)
    a = (rng.random(n) - 0.5) * scene.PATCH_KM
    b = (rng.random(n) - 0.5) * scene.PATCH_KM
    h = sc.height(torch.from_numpy(a).float().to(dev), torch.from_numpy(b).float().to(dev)).double().cpu().numpy()
    O = scene.FIXTURE_ECEF
    up = O / np.linalg.norm(O)
    e1 = np.cross(-up, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(-up, e1)
    centre = up * scene.EARTH_RADIUS_KM if ecef else np.zeros(3)
    out = rng.random(n) < outlier_frac
    h = h + np.where(out, (1 + 4 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1, 1), 0.0)
    pts = centre + a[:, None] * e1 + b[:, None] * e2 + h[:, None] * up
    return pts.astype(np.float32), out, up


def self_test(seed=1):
    """the kd-tree path against plain brute force on small clouds (ties, duplicates, non-finite points included)"""
    rng = np.random.default_rng(seed)
    clouds = [rng.random((600, 3)).astype(np.float32),
              np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32),
              np.repeat(rng.random((150, 3)).astype(np.float32), 3, 0)]
    bad = rng.random((500, 3)).astype(np.float32)
    bad[::37] = np.nan
    bad[5, 1] = np.inf
    clouds.append(bad)
    clouds.append(rng.random((600, 3)).astype(np.float32) * np.float32(2.0 ** -70))  # products underflow: index order
    for p in clouds:
        for k in (1, 8, 16):
            a = knn(p, k)
            b = knn_brute(p, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    return True
