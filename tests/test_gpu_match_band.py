"""The band-culled matcher past one super-group of targets, against the CPU oracle: the cases of tests/band_cases.py (67 036
and 65 536 targets: 66 / 64 groups, three / two super-groups) put a target split across a super-group seam, fill the list of 64
hit groups exactly and roll it over, make a wave jump over whole super-groups, and walk every group in one wave
(tests/test_band_cases.py proves that without a GPU).  Every comparison is exact: both halves of a uint2_pair; invalid,
distance, parents and location bit patterns of a DMatch.  The oracle (H.oracle_match_pairs / H.oracle_match_dmatch) is the
reference everywhere; where it runs on a share of the queries (a query's result does not depend on the other queries) the
rows are mapped back to the full index.  Every call gets its workspace at exactly ssrlcv_hip_match_workspace_bytes between
two guards, its output between two guards, and inputs that must come back as they went in."""
import contextlib
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import band_cases as C
import helpers as H
from test_gpu_glue import Guarded

pytestmark = pytest.mark.gpu

u32, vp, sz, ci = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
QID, TID = 3, 7
KINDS = {"pair": (1, H.UINT2_PAIR), "dmatch": (0, H.DMATCH)}      # SSRLCV_OUT_UINT2_PAIR, SSRLCV_OUT_DMATCH


# ---- inputs on the device (uploaded once, guarded), the geometry of a case, the call
@functools.lru_cache(maxsize=None)
def on_device(kind, name, where=None):
    f = C.targets(name) if kind == "t" else C.queries(name, where)
    return Guarded(f.nbytes, f), f


@functools.lru_cache(maxsize=None)
def fixture_cameras():
    return H.load_view("Pipeline2View")["cameras"]


def geometry(name):
    """-> (mode, (queryCam, targetP) as the oracle takes them)"""
    if name == "orbit":
        cams = fixture_cameras()
        return 1, (cams[0:1], H.oracle_projection(H.oracle(), cams[1:2]))
    return 2, (None, np.ascontiguousarray({"horizontal": C.F_HORIZONTAL, "tilted": C.F_TILTED}[name].reshape(-1)))


def match_params(capi, name, eps, delta, mode=None):
    """the library's parameters of a geometry; the projection matrix is the library's own (ssrlcv_projection_matrix_host)"""
    if name is None:
        return capi.make_match_params(mode, QID, TID, eps, delta, C.REL, C.ABS)
    if name == "orbit":
        cams = fixture_cameras()
        return capi.make_match_params(1, QID, TID, eps, delta, C.REL, C.ABS, cams[0:1], capi.projection_matrix(cams[1:2]))
    return capi.make_match_params(2, QID, TID, eps, delta, C.REL, C.ABS, fundamental={"horizontal": C.F_HORIZONTAL, "tilted": C.F_TILTED}[name])


def gpu_match(capi, geo, q_d, nq, t_d, nt, out_kind, eps, delta=0.0, mode=None):
    """one call of ssrlcv_hip_match_u8x128 (no seed) -> the records; the guards of output and workspace are checked"""
    params = match_params(capi, geo, eps, delta, mode)
    kid, dt = KINDS[out_kind]
    need = int(capi.LIB.ssrlcv_hip_match_workspace_bytes(u32(nq), u32(nt)))
    ws, out = Guarded(need), Guarded(nq * dt.itemsize)
    rc = capi.LIB.ssrlcv_hip_match_u8x128(q_d.ptr, u32(nq), t_d.ptr, u32(nt), vp(0), ctypes.byref(params), ci(kid), out.ptr, ws.ptr,
                                          sz(need), capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    body, guards = out.host()
    assert guards, "bytes outside the output were written"
    assert ws.guards_intact(), "bytes outside the workspace were written"
    # one byte less is refused
    assert capi.LIB.ssrlcv_hip_match_u8x128(q_d.ptr, u32(nq), t_d.ptr, u32(nt), vp(0), ctypes.byref(params), ci(kid), out.ptr, ws.ptr,
                                            sz(need - 1), capi.stream_ptr()) == -3
    return body.copy().view(dt)


@functools.lru_cache(maxsize=None)
def reference(out_kind, geo, qname, where, tname, eps, delta=0.0, stride=1):
    """the oracle on every stride-th query, computed once -> (records with a.y / b.y mapped back to the full index, the rows)"""
    lib = H.oracle()
    q, rows = C.every(C.queries(qname, where), stride)
    t = C.targets(tname)
    mode, (qcam, tp) = geometry(geo)
    fn = H.oracle_match_pairs if out_kind == "pair" else H.oracle_match_dmatch
    o = fn(lib, mode, QID, q, TID, t, qcam, tp, eps, delta, None, C.REL, C.ABS)
    if out_kind == "pair":
        assert np.array_equal(o["a"][:, 1], np.arange(len(q)))
        o["a"][:, 1] = rows
        unmatched = o["b"][:, 0] == QID                       # a == b marks a query without a match
        o["b"][unmatched, 1] = rows[unmatched]
    o.setflags(write=False)
    return o, rows


@contextlib.contextmanager
def arithmetic(capi, arith):
    capi.set_match_arithmetic({"i8": capi.MATCH_ARITH_I8, "f16": capi.MATCH_ARITH_F16}[arith])
    try:
        assert capi.get_match_arithmetic() == {"i8": capi.MATCH_ARITH_I8, "f16": capi.MATCH_ARITH_F16}[arith]
        yield
    finally:
        capi.set_match_arithmetic(capi.MATCH_ARITH_I8)


def assert_pairs_equal(g, o, what):
    for half in ("a", "b"):
        ne = (g[half] != o[half]).any(1)
        assert not ne.any(), (what, half, "%d of %d rows differ, first %d: got %s want %s" % (
            int(ne.sum()), len(ne), int(np.argmax(ne)), g[half][ne][:4].tolist(), o[half][ne][:4].tolist()))


def assert_dmatch_equal(g, o, what):
    for name in ("invalid", "distance"):
        ne = g[name] != o[name]
        assert not ne.any(), (what, name, int(ne.sum()), int(np.argmax(ne)), g[name][ne][:4], o[name][ne][:4])
    ok = o["invalid"] == 0
    for name in ("kp0_parent", "kp1_parent"):
        assert np.array_equal(g[name][ok], o[name][ok]), (what, name)
    for name in ("kp0_loc", "kp1_loc"):
        assert np.array_equal(g[name][ok].view(np.uint32), o[name][ok].view(np.uint32)), (what, name)


def assert_equal(out_kind, g, o, what):
    (assert_pairs_equal if out_kind == "pair" else assert_dmatch_equal)(g, o, what)


def matched(out_kind, o):
    return (o["b"][:, 0] == TID) if out_kind == "pair" else (o["invalid"] == 0)


def check(capi, out_kind, geo, qname, where, tname, eps, delta=0.0, stride=1):
    """the kernel on all queries against the oracle on every stride-th -> (the kernel's records, the oracle's, its rows)"""
    (q_d, q), (t_d, t) = on_device("q", qname, where), on_device("t", tname)
    g = gpu_match(capi, geo, q_d, len(q), t_d, len(t), out_kind, eps, delta)
    o, rows = reference(out_kind, geo, qname, where, tname, eps, delta, stride)
    assert_equal(out_kind, g[rows], o, (out_kind, geo, qname, tname, eps, delta))
    return g, o, rows


# ---- split seams: 32 splits of 3 groups; the splits from groups 30 and 63 walk groups of two super-groups
@pytest.mark.parametrize("out_kind", ["pair", "dmatch"])
@pytest.mark.parametrize("eps", [pytest.param(C.EPS_NARROW, id="narrow"), pytest.param(40.0, id="eps40")])
@pytest.mark.parametrize("arith", C.ARITHS)
def test_q3000_split_seams_on_clusters(capi, arith, eps, out_kind):
    assert C.seam_splits(C.launch_shape(3000, C.N_CLUSTERS)) == {(0, 1): 30, (1, 2): 63}
    with arithmetic(capi, arith):
        _, o, _ = check(capi, out_kind, "horizontal", "q3000", "clusters", "clusters", eps)
    ok = matched(out_kind, o)
    qc = C.cluster_of(C.queries("q3000", "clusters")["loc"])
    assert (np.bincount(qc[ok], minlength=3) > 900).all()         # matches in all three super-groups


@pytest.mark.parametrize("eps,delta", [pytest.param(25.0, 5.0, id="eps25"), pytest.param(5.0, 0.0, id="narrow")])
def test_q3000_split_seams_uniform_orbit(capi, eps, delta):
    """mode 1 with the fixture cameras on 67 036 targets uniform in 1024^2"""
    _, o, _ = check(capi, "dmatch", "orbit", "q3000", "uniform1024", "uniform1024", eps, delta)
    assert 0 < matched("dmatch", o).sum()
    check(capi, "pair", "orbit", "q3000", "uniform1024", "uniform1024", eps, delta)


@pytest.mark.parametrize("eps", [pytest.param(C.EPS_NARROW, id="narrow"), pytest.param(40.0, id="eps40")])
def test_q3000_split_seams_uniform_tilted(capi, eps):
    """mode 2 with the tilted F of test_fundamental_constrained_matches_oracle on 67 036 targets uniform in 4096^2"""
    _, o, _ = check(capi, "pair", "tilted", "q3000", "uniform4096", "uniform4096", eps)
    assert 0 < matched("pair", o).sum()
    check(capi, "dmatch", "tilted", "q3000", "uniform4096", "uniform4096", eps)


# ---- every box hit: the band walk does brute force's work (64 splits of 2 groups, 33 of them with groups, every list full)
@pytest.mark.parametrize("arith", C.ARITHS)
def test_q700_every_box_is_hit(capi, arith):
    assert C.launch_shape(700, C.N_CLUSTERS, arith) == (66, 3, 64, 2)
    with arithmetic(capi, arith):
        for out_kind in ("pair", "dmatch"):
            _, o, _ = check(capi, out_kind, "horizontal", "q700", "clusters", "clusters", C.EPS_WIDE)
            assert matched(out_kind, o).all()


# ---- one walk over every group, narrow bands: across both seams, past clusters no band of the wave reaches
@pytest.mark.parametrize("tname", ["clusters", "clusters_64"])
def test_q65536_one_walk_narrow(capi, tname):
    assert C.launch_shape(65536, len(C.targets(tname)))[2:] == (1, {"clusters": 66, "clusters_64": 64}[tname])
    g, o, rows = check(capi, "pair", "horizontal", "q65536", "clusters", tname, C.EPS_NARROW, stride=C.QUERY_STRIDE_NARROW)
    assert len(rows) >= 8192
    qc = C.cluster_of(C.queries("q65536", "clusters")["loc"])
    assert (np.bincount(qc[rows][matched("pair", o)], minlength=3) > 2500).all()
    # the rows the oracle did not see: every query is answered in its own cluster, about as often as the oracle's share
    assert np.array_equal(g["a"], np.stack([np.full(len(g), QID), np.arange(len(g))], 1))
    ok = matched("pair", g)
    assert np.array_equal(C.cluster_of(C.targets(tname)["loc"])[g["b"][ok, 1]], qc[ok])
    assert abs(ok.mean() - matched("pair", o).mean()) < 0.01


# ---- more than 64 hit groups in one walk: 66 (a second batch of two) and exactly 64
@pytest.mark.parametrize("tname", ["clusters", "clusters_64"])
def test_q65536_more_than_a_hit_list(capi, tname):
    groups = C.launch_shape(65536, len(C.targets(tname)))[3]
    assert (groups > C.HIT_LIST) if tname == "clusters" else (groups == C.HIT_LIST)
    g, o, rows = check(capi, "pair", "horizontal", "q65536", "clusters", tname, C.EPS_WIDE, stride=C.QUERY_STRIDE_WIDE)
    assert len(rows) >= 1024 and matched("pair", o).all()
    # GPU against GPU, an extra check and not the reference: with every target a candidate the contract is brute force's
    (q_d, q), (t_d, t) = on_device("q", "q65536", "clusters"), on_device("t", tname)
    g0 = gpu_match(capi, None, q_d, len(q), t_d, len(t), "pair", 0.0, mode=0)
    assert_pairs_equal(g, g0, (tname, "mode 2 with every target a candidate against mode 0"))


# ---- the frame turned across the bands: every band crosses every strip, the lists are long although epsilon is 3
def test_frame_turned_across_the_bands():
    """The narrow q3000 and q65536 cases of this file again in a child process under the developer build with the frame's
    direction forced to 90 degrees and strips of 8 px: the targets are ordered by x, every horizontal band meets every
    group, so the narrow walks fill and roll over their hit lists as the wide ones do, and the oracle stays cheap."""
    env = H.dev_env(SSRLCV_BAND_DIR="90", SSRLCV_BAND_STRIP="8")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "narrow and not turned"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "8 passed" in r.stdout, r.stdout[-500:]      # q3000: 2 arithmetics x 2 kinds on clusters, orbit, tilted; q65536: 2


# ---- hygiene: two runs bit-equal, inputs left untouched (guards and exact workspaces: every call above and here)
def test_two_runs_are_bit_equal_and_inputs_untouched(capi):
    runs = [("dmatch", "q3000", "clusters", C.EPS_NARROW), ("pair", "q65536", "clusters", C.EPS_NARROW),
            ("pair", "q65536", "clusters_64", C.EPS_NARROW), ("pair", "q65536", "clusters", C.EPS_WIDE),
            ("pair", "q65536", "clusters_64", C.EPS_WIDE)]
    for out_kind, qname, tname, eps in runs:
        (q_d, q), (t_d, t) = on_device("q", qname, "clusters"), on_device("t", tname)
        a = gpu_match(capi, "horizontal", q_d, len(q), t_d, len(t), out_kind, eps)
        b = gpu_match(capi, "horizontal", q_d, len(q), t_d, len(t), out_kind, eps)
        if out_kind == "pair":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (qname, tname, eps)
        else:
            assert_dmatch_equal(a, b, (qname, tname, eps))
            assert np.array_equal(a["kp0_loc"].view(np.uint32), b["kp0_loc"].view(np.uint32))
        for dev, host in ((q_d, q), (t_d, t)):
            body, guards = dev.host()
            assert guards and np.array_equal(body, host.view(np.uint8).reshape(-1)), (qname, tname, "an input was written")
