"""The point-cloud stage on the MI355X at its edges (tests/cloud_cases.py, proved on the CPU by tests/test_cloud_cases.py):
k-NN bit for bit against cloud_ref.knn_brute at every size constant of csrc/cloud.hip and at scales where float32 products
go subnormal, vanish or overflow; the filter on hand-made dist2 against the reference's OWN threshold; normals against eigh
to a derived angle bound and, whatever the eigengap, to an eigen-residual bound.  Every output buffer carries 64 sentinel
elements of slack that must survive, and refused calls leave their outputs untouched.

Measured on the MI355X (the bounds are derived in tests/cloud_cases.py, not taken from these): the largest angle to eigh is
4.6e-8 rad, 0.19 of angle_bound; the largest eigen-residual |C n - (n'C n) n| is 0.96 * 2^-24 l_max and the largest
n'C n - l_min is 0.71 * 2^-24 l_max, against RESIDUAL_C = 2; the 2^+-60 and ECEF images give the base cloud's normals bit
for bit; the 4.2 M-point filter case takes 0.1 s, 0.4 ms of it the filter call."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import cloud_cases as C
import cloud_ref as R

pytestmark = pytest.mark.gpu

KNN = C.knn_cases()
FILTER = C.filter_cases()
INVALID_ARG, WORKSPACE = -1, -3
SLACK = 256  # bytes: 64 elements of 4
u32, f32, sz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buf(nbytes):
    """nbytes of output and the slack, every byte the sentinel 0x5A"""
    return torch.full((int(nbytes) + SLACK,), 0x5A, dtype=torch.uint8, device="cuda")


def _host(buf, dtype, count):
    return buf[: count * np.dtype(dtype).itemsize].cpu().numpy().view(dtype).copy()


def _sentinel_from(buf, used_bytes):
    return bool((buf[int(used_bytes):] == 0x5A).all().item())


def _p(t):
    return vp(0) if t is None else vp(t.data_ptr())


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _knn_ref(name):
    return R.knn_brute(KNN[name].p, KNN[name].k)


def _knn_raw(capi, p, k, cell, want_d2=True, want_far=True, n=None, ws_short=0, null=None):
    """ssrlcv_hip_knn through the C ABI into sentinel buffers -> (rc, nbr, d2, far, slack untouched, all untouched)"""
    n = len(p) if n is None else n
    pd = _dev(p)
    need = capi.LIB.ssrlcv_hip_knn_workspace_bytes(u32(len(p)), u32(max(1, min(k, 32))))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rows = len(p) * max(0, min(k, 32))
    nb, db, fb = _buf(4 * rows), (_buf(4 * rows) if want_d2 else None), (_buf(4) if want_far else None)
    args = {"points": pd, "neighbors": nb, "workspace": ws}
    if null:
        args[null] = None
    rc = capi.LIB.ssrlcv_hip_knn(_p(args["points"]), u32(n), u32(k), f32(cell), _p(args["neighbors"]), _p(db), _p(fb),
                                 _p(args["workspace"]), sz(need - ws_short), _stream())
    torch.cuda.synchronize()
    bufs = [(nb, 4 * rows)] + ([(db, 4 * rows)] if want_d2 else []) + ([(fb, 4)] if want_far else [])
    slack = all(_sentinel_from(b, used) for b, used in bufs)
    untouched = all(_sentinel_from(b, 0) for b, _ in bufs)
    nbr = _host(nb, np.uint32, rows).reshape(len(p), -1) if rows else None
    d2 = _host(db, np.float32, rows).reshape(len(p), -1) if want_d2 and rows else None
    far = int(_host(fb, np.uint32, 1)[0]) if want_far else None
    return rc, nbr, d2, far, slack, untouched


@pytest.mark.parametrize("name", list(KNN))
def test_knn_edges_bit_equal_to_brute_force(capi, name):
    """indices and d2 bits, at every cell size of the case (automatic, tiny, about right, huge for the small ones); then
    once more with dist2_out = NULL and farQueries = NULL"""
    case = KNN[name]
    rn, rd = _knn_ref(name)
    nfin = int(R.finite_mask(case.p).sum())
    fars = []
    for cell in case.cells:
        rc, nbr, d2, far, slack, _ = _knn_raw(capi, case.p, case.k, cell)
        assert rc == 0 and slack, (name, cell, rc, slack)
        bad = np.nonzero((nbr != rn).any(1) | (_bits(d2) != _bits(rd)).any(1))[0]
        assert len(bad) == 0, (name, cell, len(bad), bad[:5], nbr[bad[:2]], rn[bad[:2]], d2[bad[:2]], rd[bad[:2]])
        assert far <= nfin
        if case.all_far:
            assert far == nfin, (name, far, nfin)   # coverage: every finite query took the far scan
        if cell == case.one_cell:
            # one cell holds the cloud: ring 0 searched everything, and only a query without k finite-d2 neighbours is open
            assert far == int((np.isinf(rd[:, case.k - 1]) & R.finite_mask(case.p)).sum()), (name, far)
        fars.append(far)
    rc, nbr, _, _, slack, _ = _knn_raw(capi, case.p, case.k, case.cells[0], want_d2=False, want_far=False)
    assert rc == 0 and slack and np.array_equal(nbr, rn), name
    print("%s: n %d (%d finite) k %d, far queries per cell size %s" % (name, len(case.p), nfin, case.k, dict(zip(case.cells, fars))))


def test_knn_argument_checks_leave_outputs_untouched(capi):
    p = C.cube(100, 9)
    rn, rd = R.knn_brute(p, 16)
    refused = [dict(k=0), dict(k=33), dict(k=16, n=16), dict(k=16, cell=-1.0), dict(k=16, cell=float("nan")),
               dict(k=16, cell=float("inf")), dict(k=16, null="points"), dict(k=16, null="workspace")]
    for a in refused:
        rc, _, _, _, _, untouched = _knn_raw(capi, p, a["k"], a.get("cell", 0.0), n=a.get("n"), null=a.get("null"))
        assert rc == INVALID_ARG and untouched, (a, rc, untouched)
    rc = _knn_raw(capi, p, 16, 0.0, null="neighbors")[0]
    assert rc == INVALID_ARG
    rc, _, _, _, _, untouched = _knn_raw(capi, p, 16, 0.0, ws_short=1)
    assert rc == WORKSPACE and untouched
    rc, nbr, d2, _, slack, _ = _knn_raw(capi, p, 16, 0.0)        # exactly the queried workspace
    assert rc == 0 and slack and np.array_equal(nbr, rn) and np.array_equal(_bits(d2), _bits(rd))


# ---------------------------------------------------------------- filter
def _filter_raw(capi, case, normals="both", sigma=None):
    n, k = case.d2.shape
    pts, nrm = C.filter_points(n)
    need = capi.LIB.ssrlcv_hip_neighbor_filter_workspace_bytes(u32(n), u32(k))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    pd, dd, nd = _dev(pts), _dev(case.d2), _dev(nrm)
    out = {"mean": _buf(4 * n), "stats": _buf(24), "points": _buf(12 * n), "index": _buf(4 * n), "normals": _buf(12 * n),
           "count": _buf(4)}
    nin = nd if normals in ("both", "in") else None
    nout = out["normals"] if normals in ("both", "out") else None
    t0 = time.perf_counter()
    rc = capi.LIB.ssrlcv_hip_neighbor_distance_filter(_p(pd), u32(n), _p(dd), u32(k), f32(case.sigma if sigma is None else sigma),
                                                      _p(out["mean"]), _p(out["stats"]), _p(out["points"]), _p(out["index"]),
                                                      _p(nin), _p(nout), _p(out["count"]), _p(ws), sz(need), _stream())
    torch.cuda.synchronize()
    return rc, out, pts, nrm, time.perf_counter() - t0


def _check_filter(capi, name, case):
    n, k = case.d2.shape
    rc, out, pts, nrm, dt = _filter_raw(capi, case)
    assert rc == 0
    rm = R.mean_distance(case.d2, k)
    sig = np.float64(np.float32(case.sigma))
    rmu, rstd, rt = R.filter_stats(rm, sig)
    m = _host(out["mean"], np.float32, n)
    assert ((_bits(m) == _bits(rm)) | (np.isnan(m) & np.isnan(rm))).all(), name
    mu, std, t = _host(out["stats"], np.float64, 3)
    assert t == mu + sig * std, (name, mu, std, t)
    assert abs(mu - rmu) <= 1e-12 * abs(rmu) and abs(std - rstd) <= 1e-12 * max(rmu, rstd), (name, mu, rmu, std, rstd)
    if case.exact:
        assert std == 0.0 and t == rt
    keep = R.filter_mask(rm, rt)   # the reference's own threshold: tests/test_cloud_cases.py shows no m near it
    if case.keep is not None:
        assert np.array_equal(keep, case.keep)
    want = np.nonzero(keep)[0]
    c = int(_host(out["count"], np.uint32, 1)[0])
    assert c == len(want), (name, c, len(want))
    assert np.array_equal(_host(out["index"], np.uint32, c), want), name
    assert np.array_equal(_host(out["points"], np.float32, 3 * c).reshape(-1, 3), pts[want]), name
    assert np.array_equal(_host(out["normals"], np.float32, 3 * c).reshape(-1, 3), nrm[want]), name
    # the rows past count and the slack keep their sentinel
    assert _sentinel_from(out["index"], 4 * c) and _sentinel_from(out["points"], 12 * c) and _sentinel_from(out["normals"], 12 * c)
    assert _sentinel_from(out["mean"], 4 * n) and _sentinel_from(out["stats"], 24) and _sentinel_from(out["count"], 4)
    return c, dt


@pytest.mark.parametrize("name", list(FILTER))
def test_filter_edges_against_the_reference_threshold(capi, name):
    c, _ = _check_filter(capi, name, FILTER[name])
    print("%s: kept %d of %d" % (name, c, len(FILTER[name].d2)))


def test_filter_second_tile_of_a_block(capi):
    """n = 2048 * 2048 + 2049: 2049 compaction tiles on 2048 blocks, so one block takes a second tile"""
    case = C.filter_big()
    t0 = time.perf_counter()
    c, dt = _check_filter(capi, "big", case)
    print("big: kept %d of %d; the filter call %.1f ms, the whole test %.1f s" % (c, len(case.d2), 1e3 * dt, time.perf_counter() - t0))


def test_filter_refusals_leave_outputs_untouched(capi):
    case = FILTER["n17_sigma2"]
    for kw in (dict(normals="in"), dict(normals="out"), dict(sigma=float("nan")), dict(sigma=float("inf"))):
        rc, out, _, _, _ = _filter_raw(capi, case, **kw)
        assert rc == INVALID_ARG and all(_sentinel_from(b, 0) for b in out.values()), kw
    rc, out, _, _, _ = _filter_raw(capi, case, normals="none")
    assert rc == 0 and _sentinel_from(out["normals"], 0)


# ---------------------------------------------------------------- normals
@pytest.fixture(scope="module")
def normal_cases():
    return C.normal_cases()


_NORMALS = {}
MEASURED = {"angle": 0.0, "angle_ratio": 0.0, "residual": 0.0, "rayleigh": 0.0}


def _gpu_normals(capi, name, case):
    if name not in _NORMALS:
        n = len(case.p)
        pd, nd = _dev(case.p), _dev(np.ascontiguousarray(case.nbr, np.uint32).view(np.int32))
        out = _buf(12 * n)
        v = capi.Float3(*[float(np.float32(x)) for x in case.vp])
        rc = capi.LIB.ssrlcv_hip_point_normals(_p(pd), u32(n), _p(nd), u32(case.k), v, _p(out), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and _sentinel_from(out, 12 * n)
        _NORMALS[name] = _host(out, np.float32, 3 * n).reshape(n, 3).astype(np.float64)
    return _NORMALS[name]


def _angle(a, b, signed):
    cr, dt = np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1)
    return np.arctan2(cr, np.where(signed, dt, np.abs(dt)))


@pytest.mark.parametrize("name", C.NORMAL_NAMES)
def test_normals_edges(capi, normal_cases, name):
    case = normal_cases[name]
    k = case.k
    n = _gpu_normals(capi, name, case)
    vp32 = np.float32(case.vp).astype(np.float64)
    ref, gap = R.normals(case.p, case.nbr, k, vp32)
    zero = np.abs(ref).sum(1) == 0
    assert np.array_equal(np.abs(n).sum(1) == 0, zero), name       # the zero rows are exactly the reference's
    if case.zero_rows is not None:
        assert np.array_equal(np.nonzero(zero)[0], case.zero_rows)
    nz = ~zero
    assert nz.any() and np.abs(np.linalg.norm(n[nz], axis=1) - 1.0).max() <= 1e-6
    # orientation, wherever the sign is decided
    with np.errstate(invalid="ignore"):
        to_v = vp32 - case.p.astype(np.float64)
        dots = (n * to_v).sum(1) / np.linalg.norm(to_v, axis=1)
    sure = nz & (np.abs(dots) > 1e-6)
    assert (dots[sure] > 0).all(), name
    if name in ("plane_vp_above", "plane_vp_below"):
        assert sure.all() and np.array_equal(n[:, 2], np.full(len(n), 1.0 if "above" in name else -1.0))
    if name == "plane_vp_inside":
        assert not sure.any() and (np.abs(n[:, 2]) == 1.0).all()      # dot = 0: either sign
    # the angle to eigh where the eigengap carries it (the sign compared only where it is decided)
    good = nz & (gap > 1e-6)
    if good.any():
        ang = _angle(n[good], ref[good], sure[good])
        bound = C.angle_bound(k, gap[good])
        MEASURED["angle"] = max(MEASURED["angle"], ang.max())
        MEASURED["angle_ratio"] = max(MEASURED["angle_ratio"], (ang / bound).max())
        print("%s: %d of %d rows with a gap; largest angle %.3g rad, largest angle / bound %.3g" %
              (name, good.sum(), nz.sum(), ang.max(), (ang / bound).max()))
        assert (ang <= bound).all(), (name, ang.max(), (ang / bound).max())
    if name.startswith(("cube", "terrain", "invariance")) and k >= 2:
        assert good.sum() >= 0.99 * nz.sum()
    # eigen-residual against the float64 covariance: every non-zero row, whatever its gap
    idx, cov = R.covariances(case.p, case.nbr)
    sel = nz[idx]
    idx, cov = idx[sel], cov[sel]
    w = np.linalg.eigvalsh(cov)
    v = n[idx]
    cn = np.einsum("mab,mb->ma", cov, v)
    ray = (v * cn).sum(1)
    res = np.linalg.norm(cn - ray[:, None] * v, axis=1)
    unit = 2.0 ** -24 * w[:, 2]
    assert (unit > 0).all()
    MEASURED["residual"] = max(MEASURED["residual"], (res / unit).max())
    MEASURED["rayleigh"] = max(MEASURED["rayleigh"], ((ray - w[:, 0]) / unit).max())
    print("%s: largest |C n - (n'C n) n| / (2^-24 l_max) %.3g, largest (n'C n - l_min) / (2^-24 l_max) %.3g (bound %g)" %
          (name, (res / unit).max(), ((ray - w[:, 0]) / unit).max(), C.RESIDUAL_C))
    assert (res <= C.RESIDUAL_C * unit).all() and (ray <= w[:, 0] + C.RESIDUAL_C * unit).all(), name
    if case.line is not None:
        assert np.abs(n[nz] @ case.line).max() <= C.RESIDUAL_C * 2.0 ** -24, name
    print("so far: %s" % MEASURED)


def test_normals_scale_and_offset_invariance(capi, normal_cases):
    """2^+-60 and the ECEF offset are exact images of the base cloud (same table): within twice the angle bound of it"""
    base = normal_cases["invariance_base"]
    n0 = _gpu_normals(capi, "invariance_base", base)
    _, gap = R.normals(base.p, base.nbr, base.k, base.vp)
    good = gap > 1e-6
    for name in C.INVARIANT:
        n = _gpu_normals(capi, name, normal_cases[name])
        ang = _angle(n[good], n0[good], np.ones(good.sum(), bool))
        print("%s against the base cloud: largest angle %.3g rad (bit-equal rows %d of %d)" %
              (name, ang.max(), (n == n0).all(1).sum(), len(n)))
        assert (ang <= 2 * C.angle_bound(base.k, gap[good])).all(), (name, ang.max())
