"""CPU-only checks of the two-nearest matcher: the numpy reference (tests/match2_ref.py) against a literal restatement of
the header contract, the synthetic cases every GPU test builds on, the binders, and the kernel's compiled resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import match2_ref as R

ROOT = H.ROOT


def _literal_knn2(qv, tv):
    idx = np.full((len(qv), 2), 0xFFFFFFFF, np.uint32)
    dist = np.full((len(qv), 2), np.inf, np.float32)
    for q in range(len(qv)):
        order = []
        for f in range(len(tv)):
            d = 0
            for a, b in zip(qv[q].tolist(), tv[f].tolist()):
                d += (a - b) * (a - b)
            order.append((d, f % 32, f))
        order.sort()
        for j, (d, _, f) in enumerate(order[:2]):
            idx[q, j] = f
            dist[q, j] = d
    return idx, dist


def test_reference_equals_a_literal_double_loop():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    t[5] = t[37] = t[2]  # equal distances: the key decides
    q[7] = t[2]
    idx, dist = R.knn2(q, t)
    lidx, ldist = _literal_knn2(q, t)
    assert np.array_equal(idx, lidx) and np.array_equal(dist, ldist)
    assert tuple(idx[7]) == (2, 5) and tuple(dist[7]) == (0.0, 0.0)  # (0, 2, 2) < (0, 5, 5) < (0, 5, 37)
    # the ratio test in float32, literally; the mutual check by the literal reverse pass
    keep_r = R.decide(q, t, 0.8, 3.0e9, False)[0]
    r2 = np.float32(0.8) * np.float32(0.8)
    assert keep_r.tolist() == [bool(np.float32(ldist[i, 0]) < np.float32(r2 * np.float32(ldist[i, 1]))) for i in range(40)]
    assert not keep_r[7]  # d1 == d2
    back = _literal_knn2(t, q)[0][:, 0]
    keep_m = R.decide(q, t, 0.0, 3.0e9, True)[0]
    assert keep_m.tolist() == [int(back[lidx[i, 0]]) == i for i in range(40)]
    # one target, no target
    i1, d1 = R.knn2(q, t[:1])
    assert (i1[:, 0] == 0).all() and (i1[:, 1] == 0xFFFFFFFF).all() and np.isinf(d1[:, 1]).all()
    assert R.decide(q, t[:1], 0.8, 3.0e9, False)[0].all()  # a missing second neighbour passes
    i0, d0 = R.knn2(q, t[:0])
    assert (i0 == 0xFFFFFFFF).all() and np.isinf(d0).all() and not R.decide(q, t[:0], 0.8, 3.0e9, True)[0].any()


def test_all_equal_descriptors_are_ordered_by_the_key():
    q = np.full((40, 128), 9, np.uint8)
    idx, dist = R.knn2(q, np.full((70, 128), 9, np.uint8))
    assert (idx == [0, 32]).all() and (dist == 0).all()  # (0, f mod 32, f): 0, 32, 64, 1, ...
    idx, _ = R.knn2(q, np.full((20, 128), 9, np.uint8))
    assert (idx == [0, 1]).all()
    idx, dist = R.knn2(q, np.full((70, 128), 9, np.uint8), fast=True)
    assert (idx == [0, 32]).all() and (dist == 0).all()


@pytest.mark.parametrize("nq,nt", [(1500, 1300), (513, 1025), (33, 31)])
def test_synthetic_cases_hold_every_outcome(nq, nt):
    qf, tf = R.synthetic(nq, nt)
    both, ratio_only, mutual_only, neither = R.assert_all_outcomes(qf, tf)
    # the selection form of the reference (large inputs) against its literal form
    for a, b in zip(R.knn2(qf["values"], tf["values"], fast=True), R.knn2(qf["values"], tf["values"], fast=False)):
        assert np.array_equal(a, b)
    assert both + ratio_only + mutual_only + neither == nq
    # the records and their survivors are consistent for every struct
    for kind in (R.OUT_DMATCH, R.OUT_UINT2_PAIR, R.OUT_MATCH):
        rec = R.match_ratio(qf, tf, 0, 1, 0.8, 3.0e9, True, kind)
        assert len(R.survivors(rec, kind)) == both
        assert rec.dtype.itemsize == {0: 48, 1: 16, 2: 40}[kind]


def test_binders_and_header_declare_the_new_entry_points():
    from ssrlcv_amd import _lib, capi
    for name in ("match2_workspace", "match_knn2", "make_ratio_params", "match_ratio"):
        assert callable(getattr(capi, name)), name
    header = open(os.path.join(ROOT, "include", "ssrlcv_hip.h")).read()
    for name in ("ssrlcv_hip_match2_workspace_bytes", "ssrlcv_hip_match_knn2_u8x128", "ssrlcv_hip_match_ratio_u8x128"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name)
    assert "ssrlcv_ratio_params" in header and "#define SSRLCV_HIP_ABI_VERSION 4" in header
    import ctypes
    assert ctypes.sizeof(capi.RatioParams) == 20
    p = capi.make_ratio_params(3, 5, ratio=0.75, absolute=100.0, mutual=True)
    assert (p.queryImageID, p.targetImageID, p.ratio, p.absoluteThreshold, p.mutual) == (3, 5, 0.75, 100.0, 1)
    # the workspace begins with the one-nearest layout and holds the reverse pass's as well (host arithmetic only)
    lib = _lib.load()
    for nq, nt in ((1, 1), (33, 31), (700, 40000), (262144, 262144)):
        w2 = lib.ssrlcv_hip_match2_workspace_bytes(ctypes.c_uint32(nq), ctypes.c_uint32(nt))
        fwd = lib.ssrlcv_hip_match_workspace_bytes(ctypes.c_uint32(nq), ctypes.c_uint32(nt))
        rev = lib.ssrlcv_hip_match_workspace_bytes(ctypes.c_uint32(nt), ctypes.c_uint32(nq))
        assert w2 > fwd + rev


def test_knn2_kernel_register_budget():
    """k_match2_i8 is ONE function of its own (not a variant of k_match_i8, whose instantiations
    test_matcher_kernels_register_budget counts), spills nothing, and runs at the occupancy DESIGN.md section 4 states."""
    csrc = os.path.join(ROOT, "ssrlcv_amd", "csrc")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-fast-math", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "matcher.hip"), "-o", os.devnull],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    knn2 = {k: v for k, v in usage.items() if "k_match2_i8" in k}
    assert len(knn2) == 1, sorted(usage)
    (mangled, res), = knn2.items()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"`k_match2_i8` keeps (\w+) query tiles per wave at (\d+) waves per SIMD", design)
    assert m, "DESIGN.md section 4 must state the kernel's query tiles and occupancy"
    tiles = {"two": 2, "four": 4}[m.group(1)]
    assert "k_match2_i8ILi%dEE" % tiles in mangled, mangled
    assert res["ScratchSize [bytes/lane]"] == 0, res
    assert res["VGPRs"] + res.get("AGPRs", 0) <= 256, res
    assert res["Occupancy [waves/SIMD]"] == int(m.group(2)), res
