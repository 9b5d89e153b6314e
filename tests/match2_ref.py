"""numpy restatement of the two-nearest / ratio / mutual contract of include/ssrlcv_hip.h (section M, PARITY UNPINNED), and
the synthetic feature pairs the tests of it share.  Nothing here touches the GPU or the library."""
import concurrent.futures
import functools

import numpy as np

import helpers as H

OUT_DMATCH, OUT_UINT2_PAIR, OUT_MATCH = 0, 1, 2
OUT_DTYPE = {OUT_DMATCH: H.DMATCH, OUT_UINT2_PAIR: H.UINT2_PAIR, OUT_MATCH: H.MATCH}
NONE = np.uint32(0xFFFFFFFF)


def keys(qv, tv):
    """int64 [nq, nt]: (distance << 32) | (f mod 32) << 27 | f // 32 of every pair; distance = exact squared L2."""
    q = qv.astype(np.int64)
    t = tv.astype(np.int64)
    # the products through a float64 matmul (BLAS): integers below 2^24, every partial sum exact
    dot = (qv.astype(np.float64) @ tv.astype(np.float64).T).astype(np.int64)
    d = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * dot
    f = np.arange(len(tv), dtype=np.int64)
    return (d << 32) | ((f & 31) << 27) | (f >> 5)


def key_index(k):
    lo = k & 0xFFFFFFFF
    return ((lo & 0x07FFFFFF) << 5) | (lo >> 27)


def _two_smallest_keys(q, t32, tn):
    """the two smallest keys of every row of q against the targets, without forming every key: float32 distances (integers
    below 2^24: every sum exact), the second-smallest distance d2 of a row by selection, exact keys only where d <= d2"""
    q32 = q.astype(np.float32)
    d = (q32 * q32).sum(1)[:, None] + tn[None, :]
    d -= 2.0 * (q32 @ t32.T)
    d2 = np.partition(d, 1, axis=1)[:, 1]
    r, f = np.nonzero(d <= d2[:, None])  # row-major: r ascending; at least two per row
    k = (d[r, f].astype(np.int64) << 32) | ((f.astype(np.int64) & 31) << 27) | (f.astype(np.int64) >> 5)
    order = np.lexsort((k, r))
    r, k = r[order], k[order]
    first = np.searchsorted(r, np.arange(len(q)))
    return np.stack([k[first], k[first + 1]], 1)


def knn2(qv, tv, chunk=256, fast=None):
    """-> (index uint32 [nq, 2], distance float32 [nq, 2]); a missing neighbour is (UINT32_MAX, +inf).  Small inputs go
    through keys() literally; large ones (fast, default from 2^24 pairs) through _two_smallest_keys, chunks on 8 threads."""
    nq, nt = len(qv), len(tv)
    idx = np.full((nq, 2), NONE, np.uint32)
    dist = np.full((nq, 2), np.inf, np.float32)
    if nt == 0:
        return idx, dist
    if fast is None:
        fast = nq * nt >= (1 << 24)
    fast = fast and nt >= 2
    if fast:
        t32 = tv.astype(np.float32)
        tn = (t32 * t32).sum(1)

    def rows(q0):
        if fast:
            two = _two_smallest_keys(qv[q0:q0 + chunk], t32, tn)
        else:
            k = keys(qv[q0:q0 + chunk], tv)
            two = k if nt == 1 else np.sort(np.partition(k, 1, axis=1)[:, :2], axis=1)
        for j in range(two.shape[1]):
            idx[q0:q0 + chunk, j] = key_index(two[:, j]).astype(np.uint32)
            dist[q0:q0 + chunk, j] = (two[:, j] >> 32).astype(np.float32)

    starts = range(0, nq, chunk)
    if not fast:
        for q0 in starts:
            rows(q0)
    else:  # numpy's element-wise passes run on one core each and release the GIL: chunks side by side
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(rows, starts))
    return idx, dist


def decide(qv, tv, ratio, absolute, mutual, nn=None, back=None):
    """-> (keep bool [nq], neighbour 1 uint32 [nq], d1 float32 [nq] (absolute where there is no neighbour)).
    nn = knn2(qv, tv) and back = knn2(tv, qv)[0][:, 0], when the caller has them already."""
    idx, dist = nn if nn is not None else knn2(qv, tv)
    found = idx[:, 0] != NONE
    absolute = np.float32(absolute)
    d1 = np.where(found, dist[:, 0], absolute).astype(np.float32)
    keep = found & ~(d1 >= absolute)
    if ratio > 0:
        r2 = np.float32(ratio) * np.float32(ratio)
        has2 = idx[:, 1] != NONE
        with np.errstate(invalid="ignore"):
            rhs = (r2 * np.where(has2, dist[:, 1], np.float32(0))).astype(np.float32)
        keep &= ~has2 | (d1 < rhs)
    if mutual and len(tv):
        if back is None:
            back = knn2(tv, qv)[0][:, 0]  # neighbour 1 of every target among all queries
        j = np.where(found, idx[:, 0], 0).astype(np.int64)
        keep &= back[j] == np.arange(len(qv), dtype=np.uint32)
    return keep, idx[:, 0], d1


def match_ratio(qf, tf, query_id, target_id, ratio, absolute, mutual, out_kind, nn=None, back=None):
    """The records ssrlcv_hip_match_ratio_u8x128 writes (qf, tf: helpers.FEATURE arrays)."""
    keep, j, d1 = decide(qf["values"], tf["values"], ratio, absolute, mutual, nn, back)
    nq = len(qf)
    out = np.zeros(nq, OUT_DTYPE[out_kind])
    q = np.arange(nq, dtype=np.uint32)
    if out_kind == OUT_UINT2_PAIR:
        out["a"][:, 0] = query_id
        out["a"][:, 1] = q
        out["b"][:, 0] = np.where(keep, target_id, query_id)
        out["b"][:, 1] = np.where(keep, j, q)
        return out
    out["invalid"] = ~keep
    jj = np.where(keep, j, 0).astype(np.int64)
    out["kp0_parent"] = np.where(keep, query_id, 0)
    out["kp1_parent"] = np.where(keep, target_id, 0)
    out["kp0_loc"] = np.where(keep[:, None], qf["loc"], np.float32(0))
    if len(tf):
        out["kp1_loc"] = np.where(keep[:, None], tf["loc"][jj], np.float32(0))
    if out_kind == OUT_DMATCH:
        out["distance"] = d1
    return out


def survivors(records, out_kind):
    """what validateMatches / compact_matches leaves, in order"""
    if out_kind == OUT_UINT2_PAIR:
        keep = ~((records["a"] == records["b"]).all(1))
    else:
        keep = records["invalid"] == 0
    # whole records, padding bytes included (indexing a structured array copies its fields only)
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(len(records), records.dtype.itemsize)
    return np.ascontiguousarray(raw[keep]).reshape(-1).view(records.dtype)


def features(values, image_id, seed):
    f = np.zeros(len(values), H.FEATURE)
    rng = np.random.default_rng(seed)
    f["parent"] = image_id
    f["loc"] = rng.uniform(0, 1024, (len(values), 2)).astype(np.float32)
    f["sigma"] = 1.0
    f["values"] = values
    return f


def _noisy(rng, base, sigma):
    return np.clip(np.rint(base.astype(np.float64) + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def synthetic(nq, nt, seed=7):
    """(query FEATURE[nq], target FEATURE[nt]) on which every outcome of the ratio test and the mutual check occurs:
    uniform u8 descriptors; m = min(nq, nt) // 2 targets are noisy copies (sigma 8) of m queries; the next m // 10 targets
    are EXACT copies of matched targets (d1 == d2: the ratio test rejects their queries); m // 10 unmatched queries are
    noisy copies (sigma 12) of matched targets: rivals that pass the ratio test and fail the mutual check.  Cached: the
    arrays are shared between tests and must not be written to."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    m = min(nq, nt) // 2
    c = m // 10
    src, dst = rng.permutation(nq), rng.permutation(nt)
    t[dst[:m]] = _noisy(rng, q[src[:m]], 8)
    t[dst[m:m + c]] = t[dst[:c]]
    q[src[m:m + c]] = _noisy(rng, t[dst[c:2 * c]], 12)
    qf, tf = features(q, 0, seed + 1), features(t, 1, seed + 2)
    for a in (qf, tf):
        a.setflags(write=False)
    return qf, tf


def outcomes(qf, tf, ratio=0.8):
    """-> (kept by ratio, kept by mutual) bool arrays at an infinite absolute threshold"""
    r = decide(qf["values"], tf["values"], ratio, 3.0e9, False)[0]
    mu = decide(qf["values"], tf["values"], 0.0, 3.0e9, True)[0]
    return r, mu


def assert_all_outcomes(qf, tf, ratio=0.8):
    r, mu = outcomes(qf, tf, ratio)
    counts = ((r & mu).sum(), (r & ~mu).sum(), (~r & mu).sum(), (~r & ~mu).sum())
    assert all(c > 0 for c in counts), "a vacuous case: (both, ratio only, mutual only, neither) = %s" % (counts,)
    return counts
