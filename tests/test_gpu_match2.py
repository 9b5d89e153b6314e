"""GPU tests of the two-nearest matcher (ssrlcv_hip_match_knn2_u8x128 / ssrlcv_hip_match_ratio_u8x128) against the numpy
restatement of their header contract (tests/match2_ref.py).  Every comparison is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

import helpers as H
import match2_ref as R

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))

INF_ABS = 3.0e9
KINDS = (R.OUT_DMATCH, R.OUT_UINT2_PAIR, R.OUT_MATCH)


def _knn2(capi, qf, tf, workspace=None):
    idx, dist = capi.match_knn2(capi.to_dev(qf), len(qf), capi.to_dev(tf) if len(tf) else None, len(tf), workspace=workspace)
    return idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()


def _assert_knn2(capi, qf, tf):
    idx, dist = _knn2(capi, qf, tf)
    ridx, rdist = R.knn2(qf["values"], tf["values"])
    assert np.array_equal(idx, ridx), np.argwhere(idx != ridx)[:5]
    assert np.array_equal(H.bits(dist), H.bits(rdist))
    return idx, dist


def _tiles_per_split(nq, nt):
    """the split rule of the brute-force passes (csrc/matcher.hip make_layout2): 512 queries per block"""
    qblocks, tiles = (nq + 511) // 512, (nt + 31) // 32
    splits = 1
    while qblocks * splits < 1024 and splits * 2 <= tiles and tiles // (splits * 2) >= 16:
        splits *= 2
    return (tiles + splits - 1) // splits, splits


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (33, 31), (32, 32), (33, 33), (513, 1025), (1500, 1300), (700, 40000)])
def test_knn2_equals_reference(capi, nq, nt):
    if min(nq, nt) >= 20:
        qf, tf = R.synthetic(nq, nt)
    else:
        rng = np.random.default_rng(nq * 7 + nt)
        qf = R.features(rng.integers(0, 256, (nq, 128), dtype=np.uint8), 0, 1)
        tf = R.features(rng.integers(0, 256, (nt, 128), dtype=np.uint8), 1, 2)
    idx, _ = _assert_knn2(capi, qf, tf)
    if (nq, nt) == (513, 1025):
        assert _tiles_per_split(nq, nt) == (17, 2)  # the first target split
    if (nq, nt) == (700, 40000):
        assert _tiles_per_split(nq, nt)[1] == 64
    if (nq, nt) == (1500, 1300):
        # neighbour 1 is the winner of the existing one-nearest matcher at an infinite threshold
        params = capi.make_match_params(0, 0, 1, absolute=INF_ABS)
        old = capi.to_host(capi.match(capi.to_dev(qf), nq, capi.to_dev(tf), nt, params, capi.OUT_UINT2_PAIR), H.UINT2_PAIR, nq)
        assert (old["b"][:, 0] == 1).all() and np.array_equal(old["b"][:, 1], idx[:, 0])


def test_knn2_degenerate_ties(capi):
    """Equal distances: the key (distance, f mod 32, f) alone decides -- inside a lane, across the two lane halves of a tile
    (rows 0-3 | 4-7 of every eight), across tiles and across a target split."""
    ones = np.full((100, 128), 9, np.uint8)
    idx, dist = _assert_knn2(capi, R.features(ones[:64], 0, 1), R.features(ones, 1, 2))
    assert (idx == [0, 32]).all() and (dist == 0).all()
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, (64, 128), dtype=np.uint8)
    # lane halves: the same vector at rows 2 (half 0) and 5 (half 1) of one tile; every query is at equal distance of both
    t = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    t[2] = t[5] = np.clip(q[0].astype(int) + 1, 0, 255)
    q[1:33] = np.clip(t[2].astype(int) + rng.integers(-3, 4, (32, 128)), 0, 255)
    idx, dist = _assert_knn2(capi, R.features(q, 0, 1), R.features(t, 1, 2))
    assert (idx[:33] == [2, 5]).all() and (dist[:33, 0] == dist[:33, 1]).all()
    # ... and at rows 2, 5, 34 and the same row of the first tile of the second split
    nt = 2000
    tps, splits = _tiles_per_split(64, nt)
    assert splits >= 2
    t = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    rows = [2, 5, 34, tps * 32 + 2]
    for r in rows:
        t[r] = t[2]
    q[1:33] = np.clip(t[2].astype(int) + rng.integers(-3, 4, (32, 128)), 0, 255)
    q[0] = t[2]
    idx, dist = _assert_knn2(capi, R.features(q, 0, 1), R.features(t, 1, 2))
    assert (idx[:33] == [2, 34]).all() and (dist[:33, 0] == dist[:33, 1]).all()  # (d, 2, 0) < (d, 2, 1) < (d, 2, tps) < (d, 5, 0)
    # the other order of arrival: the copy in the second split has the smallest key of the three
    t[2] = rng.integers(0, 256, 128, dtype=np.uint8)
    t[34] = t[2]
    t[tps * 32] = t[5]
    idx, _ = _assert_knn2(capi, R.features(q, 0, 1), R.features(t, 1, 2))
    assert (idx[:33] == [tps * 32, tps * 32 + 2]).all()  # (d, 0, tps) < (d, 2, tps) < (d, 5, 0)


@pytest.mark.parametrize("nq,nt", [(33, 31), (513, 1025), (1500, 1300)])
def test_match_ratio_every_struct_byte_equals_reference(capi, nq, nt):
    import torch
    qf, tf = R.synthetic(nq, nt)
    R.assert_all_outcomes(qf, tf)
    nn = R.knn2(qf["values"], tf["values"])
    back = R.knn2(tf["values"], qf["values"])[0][:, 0]
    q_d, t_d = capi.to_dev(qf), capi.to_dev(tf)
    ws = capi.match2_workspace(nq, nt)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    median = float(np.median(nn[1][:, 0]))
    for kind in KINDS:
        size = R.OUT_DTYPE[kind].itemsize
        for mutual in (False, True):
            for ratio in (0.0, 0.8, 1.0):
                for absolute in (INF_ABS, median):
                    ref = R.match_ratio(qf, tf, 4, 9, ratio, absolute, mutual, kind, nn=nn, back=back)
                    what = (kind, mutual, ratio, absolute)
                    everything = ratio == 0.0 and not mutual and absolute == INF_ABS  # nothing rejects
                    assert 0 < len(R.survivors(ref, kind)) < nq or everything, what
                    params = capi.make_ratio_params(4, 9, ratio=ratio, absolute=absolute, mutual=mutual)
                    out = capi.match_ratio(q_d, nq, t_d, nt, params, kind, workspace=ws)
                    got = out.cpu().numpy()[: nq * size]
                    assert np.array_equal(got, ref.view(np.uint8).reshape(-1)), what
                    # validateMatches on the same workspace: the reference's survivors, in order
                    if kind == R.OUT_MATCH:  # (40 bytes: the counted copy of the asynchronous form does not take it)
                        n = capi.compact_matches(kind, out, nq, ws)
                    else:
                        capi.compact_matches_async(kind, out, nq, ws, count)
                        n = int(count.item())
                    keep = R.survivors(ref, kind)
                    assert n == len(keep), what
                    assert np.array_equal(out.cpu().numpy()[: n * size], keep.view(np.uint8).reshape(-1)), what


def test_match_ratio_on_real_descriptors(capi, everest_oracle_features):
    qf, tf = everest_oracle_features[0], everest_oracle_features[1]
    nq, nt = len(qf), len(tf)
    ref = R.match_ratio(qf, tf, 0, 1, 0.8, INF_ABS, True, R.OUT_UINT2_PAIR)
    params = capi.make_ratio_params(0, 1, ratio=0.8, absolute=INF_ABS, mutual=True)
    out = capi.to_host(capi.match_ratio(capi.to_dev(qf), nq, capi.to_dev(tf), nt, params, capi.OUT_UINT2_PAIR), H.UINT2_PAIR, nq)
    assert np.array_equal(out, ref)
    assert 0 < len(R.survivors(ref, R.OUT_UINT2_PAIR)) < nq


def test_match2_is_deterministic_and_checks_its_arguments(capi):
    import torch
    qf, tf = R.synthetic(513, 1025)
    q_d, t_d = capi.to_dev(qf), capi.to_dev(tf)
    ws = capi.match2_workspace(1500, 1300)
    assert ws.numel() >= capi.LIB.ssrlcv_hip_match2_workspace_bytes(capi.c_u32(513), capi.c_u32(1025))
    params = capi.make_ratio_params(0, 1, ratio=0.8, mutual=True)
    a = capi.match_ratio(q_d, 513, t_d, 1025, params, capi.OUT_DMATCH, workspace=ws).clone()
    ia, da = capi.match_knn2(q_d, 513, t_d, 1025, workspace=ws)
    # ... a call of other shapes on the same workspace in between
    q2, t2 = R.synthetic(1500, 1300)
    capi.match_ratio(capi.to_dev(q2), 1500, capi.to_dev(t2), 1300, params, capi.OUT_DMATCH, workspace=ws)
    b = capi.match_ratio(q_d, 513, t_d, 1025, params, capi.OUT_DMATCH, workspace=ws)
    ib, db = capi.match_knn2(q_d, 513, t_d, 1025, workspace=ws)
    assert torch.equal(a, b) and torch.equal(ia, ib) and torch.equal(da.view(torch.int32), db.view(torch.int32))

    # errors, before any launch: the outputs keep their sentinel
    lib, c = capi.LIB, capi
    out = torch.full((513 * 48,), 0xAB, dtype=torch.uint8, device="cuda")

    def call(p, kind=0, out_t=out, nbytes=None, target=t_d):
        return lib.ssrlcv_hip_match_ratio_u8x128(c.ptr(q_d), c.c_u32(513), c.ptr(target), c.c_u32(1025), ctypes.byref(p),
                                                 c.c_int(kind), c.ptr(out_t), c.ptr(ws),
                                                 c.c_sz(ws.numel() if nbytes is None else nbytes), c.stream_ptr())
    for ratio in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(c.make_ratio_params(0, 1, ratio=ratio)) == -1, ratio
    assert call(c.make_ratio_params(0, 1, absolute=float("nan"))) == -1
    assert call(params, kind=3) == -1 and call(params, kind=-1) == -1
    assert call(params, out_t=None) == -1 and call(params, target=None) == -1
    need = lib.ssrlcv_hip_match2_workspace_bytes(c.c_u32(513), c.c_u32(1025))
    assert call(params, nbytes=need - 1) == -3
    idx = torch.full((513, 2), 7, dtype=torch.int32, device="cuda")
    assert lib.ssrlcv_hip_match_knn2_u8x128(c.ptr(q_d), c.c_u32(513), c.ptr(t_d), c.c_u32(1025), c.ptr(idx), None, c.ptr(ws),
                                            c.c_sz(need - 1), c.stream_ptr()) == -3
    assert lib.ssrlcv_hip_match_knn2_u8x128(c.ptr(q_d), c.c_u32(513), c.ptr(t_d), c.c_u32(1025), None, None, c.ptr(ws),
                                            c.c_sz(need), c.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (out == 0xAB).all() and (idx == 7).all()
    assert call(params, nbytes=need) == 0  # the exact size is enough
    # numQuery 0: nothing to do
    assert lib.ssrlcv_hip_match_ratio_u8x128(c.ptr(q_d), c.c_u32(0), c.ptr(t_d), c.c_u32(1025), ctypes.byref(params), c.c_int(0),
                                             c.ptr(out), c.ptr(ws), c.c_sz(0), c.stream_ptr()) == 0
    # no targets: every neighbour missing, every entry rejected
    i0, d0 = capi.match_knn2(q_d, 513, None, 0, workspace=ws)
    assert (i0 == -1).all() and torch.isinf(d0).all()
    for kind in KINDS:
        for mutual in (False, True):
            p = capi.make_ratio_params(2, 3, ratio=0.8, absolute=1234.0, mutual=mutual)
            got = capi.match_ratio(q_d, 513, None, 0, p, kind, workspace=ws).cpu().numpy()
            ref = R.match_ratio(qf, tf[:0], 2, 3, 0.8, 1234.0, mutual, kind)
            assert np.array_equal(got[: ref.nbytes], ref.view(np.uint8).reshape(-1))
            assert len(R.survivors(ref, kind)) == 0
            if kind == R.OUT_DMATCH:
                assert (ref["distance"] == np.float32(1234.0)).all()


def test_match_ratio_replays_from_a_graph(capi):
    """The call is a single chain of kernels on the caller's stream: captured, it replays to the same bytes, every time."""
    import torch
    qf, tf = R.synthetic(513, 1025)
    q_d, t_d = capi.to_dev(qf), capi.to_dev(tf)
    ws = capi.match2_workspace(513, 1025)
    out = capi.dev_bytes(513 * 48)
    params = capi.make_ratio_params(0, 1, ratio=0.8, mutual=True)
    capi.match_ratio(q_d, 513, t_d, 1025, params, capi.OUT_DMATCH, workspace=ws, out=out)
    eager = out.clone()
    ref = R.match_ratio(qf, tf, 0, 1, 0.8, INF_ABS, True, R.OUT_DMATCH)
    assert np.array_equal(eager.cpu().numpy(), ref.view(np.uint8).reshape(-1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capi.match_ratio(q_d, 513, t_d, 1025, params, capi.OUT_DMATCH, workspace=ws, out=out)
    for _ in range(3):
        out.zero_()
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        diff = torch.nonzero(out != eager).flatten()
        assert diff.numel() == 0, "%d bytes differ, first at %s" % (diff.numel(), diff[:8].tolist())


def test_match_pairs_with_ratio_and_mutual(capi):
    from ssrlcv_amd import pipeline
    sets = [R.synthetic(300, 257)[0], R.synthetic(300, 257)[1], R.synthetic(411, 300, seed=9)[1]]
    feats = [capi.to_dev(f) for f in sets]
    got = pipeline.match_pairs(feats, None, mode=0, absolute=INF_ABS, ratio=0.8, mutual=True)
    pairs = [(0, 1), (0, 2), (1, 2)]
    assert sorted(got) == [0, 1, 2]
    kept = 0
    for p, (qi, ti) in enumerate(pairs):
        nq, nt = len(sets[qi]), len(sets[ti])
        ws = capi.match2_workspace(nq, nt)
        out = capi.match_ratio(feats[qi], nq, feats[ti], nt, capi.make_ratio_params(qi, ti, ratio=0.8, absolute=INF_ABS, mutual=True),
                               capi.OUT_UINT2_PAIR, workspace=ws)
        n = capi.compact_matches(capi.OUT_UINT2_PAIR, out, nq, ws)
        ref = R.survivors(R.match_ratio(sets[qi], sets[ti], qi, ti, 0.8, INF_ABS, True, R.OUT_UINT2_PAIR), R.OUT_UINT2_PAIR)
        assert n == len(ref) and np.array_equal(capi.to_host(got[p], H.UINT2_PAIR), ref)
        assert np.array_equal(capi.to_host(out, H.UINT2_PAIR, n), ref)
        kept += n
    assert kept > 100
    # without the new keywords: the existing path, byte for byte
    old = pipeline.match_pairs(feats, None, mode=0, absolute=INF_ABS)
    for p, (qi, ti) in enumerate(pairs):
        nq, nt = len(sets[qi]), len(sets[ti])
        ws = capi.match_workspace(nq, nt)
        out = capi.match(feats[qi], nq, feats[ti], nt, capi.make_match_params(0, qi, ti, 25.0, 5.0, 0.6, INF_ABS), capi.OUT_UINT2_PAIR,
                         workspace=ws)
        n = capi.compact_matches(capi.OUT_UINT2_PAIR, out, nq, ws)
        assert n == nq and np.array_equal(capi.to_host(old[p], H.UINT2_PAIR), capi.to_host(out, H.UINT2_PAIR, n))
    # what the new keywords refuse
    seed = sets[0][:10]
    for kw in (dict(mode=1, ratio=0.8), dict(mode=0, ratio=0.8, seed_features=seed), dict(mode=0, mutual=True, seed_features=seed)):
        with pytest.raises(ValueError):
            pipeline.match_pairs(feats, None, **kw)


def test_two_view_uncalibrated_runs_end_to_end(capi):
    """ratio + mutual matches -> F-matrix RANSAC -> F-constrained matcher on a rendered pair: runs, is deterministic, and its
    first stage is match_ratio.  (No accuracy figure: none has been measured.)"""
    import torch
    import scene
    from ssrlcv_amd import pipeline
    S = 512
    imgs, _, _, _ = scene.pinhole_views(2, S)
    feats = []
    for im in imgs:
        plan = capi.SiftPlan(S, S)
        plan.extract(im)
        feats.append(plan.features[: plan.count() * 152].clone())
    nq, nt = feats[0].numel() // 152, feats[1].numel() // 152
    assert nq > 500 and nt > 500
    a = pipeline.two_view_uncalibrated(feats[0], feats[1], ratio=0.8, samples=1024, threshold=1.0, epsilon=2.0)
    b = pipeline.two_view_uncalibrated(feats[0], feats[1], ratio=0.8, samples=1024, threshold=1.0, epsilon=2.0)
    ws = capi.match2_workspace(nq, nt)
    first = capi.match_ratio(feats[0], nq, feats[1], nt, capi.make_ratio_params(0, 1, ratio=0.8, absolute=INF_ABS, mutual=True),
                             capi.OUT_MATCH, workspace=ws)
    putative = capi.compact_matches(capi.OUT_MATCH, first, nq, ws)
    assert putative == a["num_putative"] and torch.equal(a["putative"], first[: putative * 40])
    print("two_view_uncalibrated %d^2: %d x %d features, %d putative, %d inliers, %d constrained matches" %
          (S, nq, nt, putative, a["inliers"], a["count"]))
    assert a["F"].shape == (3, 3) and np.array_equal(H.bits(a["F"]), H.bits(b["F"]))
    assert a["inliers"] == b["inliers"] and a["count"] == b["count"], (a["inliers"], b["inliers"], a["count"], b["count"])
    assert 7 <= a["inliers"] <= putative < nq
    dm, dm_b = capi.to_host(a["matches"], H.DMATCH, a["count"]), capi.to_host(b["matches"], H.DMATCH, b["count"])
    assert a["count"] > 0 and (dm["invalid"] == 0).all()
    for name in H.DMATCH.names:  # (field by field: the one-nearest matcher leaves the padding bytes of a DMatch undefined)
        assert np.array_equal(H.bits(dm[name]) if dm[name].dtype == np.float32 else dm[name], H.bits(dm_b[name]) if dm[name].dtype == np.float32 else dm_b[name]), name


def test_match_factory_ratio_through_class_api(capi, tmp_path):
    """MatchFactory::generateMatchesRatio / generateDistanceMatchesRatio / generateMatchesRatioIndexOnly
    (tests/cpp/ratio_match_test.cpp) on a dumped feature pair: the three validated arrays Python's binder gives."""
    import subprocess
    qf, tf = R.synthetic(513, 1025)
    path = str(tmp_path / "pair.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(qf), len(tf)], np.uint64).tobytes() + qf.tobytes() + tf.tobytes())
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ssrlcv_amd", "host"), "_build/ratio_match_test"])
    exe = os.path.join(ROOT, "ssrlcv_amd", "host", "_build", "ratio_match_test")
    prefix = str(tmp_path / "out")
    median = float(np.median(R.knn2(qf["values"], tf["values"])[1][:, 0]))
    out = subprocess.check_output([exe, path, "0.8", "1", repr(median), prefix]).decode()
    assert out.splitlines()[-1] == "ok", out
    q_d, t_d = capi.to_dev(qf), capi.to_dev(tf)
    ws = capi.match2_workspace(len(qf), len(tf))
    params = capi.make_ratio_params(3, 5, ratio=0.8, absolute=median, mutual=True)  # the driver's image ids
    for kind, ext in ((R.OUT_MATCH, "match"), (R.OUT_DMATCH, "dmatch"), (R.OUT_UINT2_PAIR, "pairs")):
        rec = capi.match_ratio(q_d, len(qf), t_d, len(tf), params, kind, workspace=ws)
        n = capi.compact_matches(kind, rec, len(qf), ws)
        want = rec.cpu().numpy()[: n * R.OUT_DTYPE[kind].itemsize]
        ref = R.survivors(R.match_ratio(qf, tf, 3, 5, 0.8, median, True, kind), kind)
        assert 0 < n == len(ref) and np.array_equal(want, ref.view(np.uint8).reshape(-1))
        got = np.fromfile(prefix + "." + ext, np.uint8)
        assert np.array_equal(got, want), ext
