"""GPU parity off the fixture: csrc/pose.hip (k_pose_terms, k_pose_cost) against the reference of tests/pose_cases.py --
one match at a time bit for bit, sums of many matches entry by entry within the derived bound gamma_d * sum |terms|
(pose_cases.chain_depth), with cameras of different intrinsics, n around the wave and the block, a second pass of the
grid-stride loop, key points outside the image, and a match whose rays are exactly parallel.  tests/test_pose_cases.py
proves on the oracle alone that the cases would catch a wrong kernel.

Worst |got - exact| / bound per case, MI355X: see DESIGN.md section 2."""
import numpy as np
import pytest

import helpers as H
import pose_cases as C

pytestmark = pytest.mark.gpu

INVALID_ARG = -1                                             # SSRLCV_ERR_INVALID_ARG


def _structure(jtj, jtf, what):
    """every call: JTJ exactly symmetric, the position rows, columns and JTf entries exactly +0"""
    assert np.array_equal(H.bits(jtj), H.bits(jtj.T)), (what, jtj)
    assert not H.bits(jtj[3:, :]).any() and not H.bits(jtj[:, 3:]).any() and not H.bits(jtf[3:]).any(), (what, jtj, jtf)


def _run(capi, m_d, n, c):
    jtj, jtf, cost = capi.pose_lm_terms(m_d, n, c["pose"], c["cams"][0:1], c["cams"][1:2])
    alone = capi.pose_cost(m_d, n, c["pose"], c["cams"][0:1], c["cams"][1:2])
    return jtj, jtf, cost, alone


def _check_sums(capi, oracle_lib, name):
    """one case through pose_lm_terms and pose_cost against its reference -> the worst |got - S| / bound"""
    c = C.case(name)
    ref = C.reference(oracle_lib, name)
    m_d = capi.to_dev(c["matches"])
    jtj, jtf, cost, alone = _run(capi, m_d, ref["n"], c)
    _structure(jtj, jtf, name)
    got = C.got10(jtj, jtf, cost)
    worst = 0.0
    for k, what in enumerate(C.NAMES + ("pose_cost",)):
        g, j = (got[k], k) if k < 10 else (np.float32(alone), 9)
        S, bound = ref["S"][j], ref["bound"][j]
        ratio = abs(float(g) - S) / bound if np.isfinite(S) and np.isfinite(g) and bound > 0 else float("nan")
        print("%s %s: got %r, reference %r, bound %.3g, ratio %.3f" % (name, what, float(g), float(S), bound, ratio))
        assert C.agrees(g, S, bound), (name, what, float(g), S, bound)
        if np.isfinite(S):
            worst = max(worst, ratio)
    print("%s: n %d, worst |got - exact| / bound %.3f" % (name, ref["n"], worst))
    return worst


def _single(capi, oracle_lib, matches, pose, cams, what):
    """every match alone: all 10 sums and pose_cost equal the reference bit for bit"""
    f, J = H.oracle_pose_match_terms(oracle_lib, matches, pose, cams[0:1], cams[1:2])
    assert np.isfinite(f).all() and np.isfinite(J).all()
    want = C.one_match_sums(C.products(f, J))
    m_d = capi.to_dev(matches)
    c = dict(pose=pose, cams=cams)
    bad = []
    for i in range(len(matches)):
        jtj, jtf, cost, alone = _run(capi, m_d[40 * i:40 * (i + 1)], 1, c)
        _structure(jtj, jtf, (what, i))
        got = np.append(C.got10(jtj, jtf, cost), np.float32(alone))
        w = np.append(want[i], want[i][9])
        if not np.array_equal(H.bits(got), H.bits(w)):
            bad.append((i, [(C.NAMES[min(k, 9)], float(got[k]), float(w[k])) for k in np.flatnonzero(H.bits(got) != H.bits(w))]))
    print("%s: %d of %d matches bit-equal in all 10 sums and pose_cost" % (what, len(matches) - len(bad), len(matches)))
    assert not bad, (what, len(bad), bad[:3])


def test_single_match_is_bit_equal(capi, oracle_lib):
    c = C.case("single")
    _single(capi, oracle_lib, c["matches"], c["pose"], c["cams"], "single")
    v = H.load_view("Pipeline2View")
    m = H.matches_from_matchset(v["kp0"])
    _single(capi, oracle_lib, np.ascontiguousarray(m[[0, -1]]), H.relative_pose(v["cameras"]), v["cameras"], "fixture ends")


@pytest.mark.parametrize("name", C.SUM_CASES)
def test_sums_within_the_derived_bound(capi, oracle_lib, name):
    assert _check_sums(capi, oracle_lib, name) <= 1


@pytest.mark.parametrize("name", C.NONFINITE_CASES)
def test_nonfinite_match(capi, oracle_lib, name):
    """parallel rays: NaN where the terms' sum is NaN, the bound where it is finite, +0 in the position entries"""
    ref = C.reference(oracle_lib, name)
    assert np.isnan(ref["S"]).any() and np.isfinite(ref["S"]).any()
    _check_sums(capi, oracle_lib, name)


# ---- the output contract through the raw C ABI -------------------------------------------------------------------------------
def _raw(capi, m_d, n, c, args=None):
    """both entry points with caller-owned buffers pre-filled with 0xA5 bytes, one float longer than needed
    -> (rc_terms, rc_cost, out43 bits, cost bits); no host synchronisation before the read-back"""
    import torch
    pose = np.asarray(c["pose"], np.float32).copy()
    q, t = capi._host_bytes(c["cams"][0:1], 80), capi._host_bytes(c["cams"][1:2], 80)
    out = torch.full((4 * 44,), 0xA5, dtype=torch.uint8, device="cuda")
    cost = torch.full((4 * 2,), 0xA5, dtype=torch.uint8, device="cuda")
    a = dict(matches=capi.ptr(m_d), pose=pose.ctypes.data_as(capi.c_vp), query=q.ctypes.data_as(capi.c_vp),
             target=t.ctypes.data_as(capi.c_vp), out=capi.ptr(out), cost=capi.ptr(cost))
    a.update(args or {})
    rc1 = capi.LIB.ssrlcv_hip_pose_lm_terms(a["matches"], capi.c_u32(n), a["pose"], a["query"], a["target"], a["out"],
                                            capi.stream_ptr())
    rc2 = capi.LIB.ssrlcv_hip_pose_cost(a["matches"], capi.c_u32(n), a["pose"], a["query"], a["target"], a["cost"],
                                        capi.stream_ptr())
    o, k = out.cpu().numpy().view(np.uint32), cost.cpu().numpy().view(np.uint32)
    assert o[43] == 0xA5A5A5A5 and k[1] == 0xA5A5A5A5                           # nothing past the end
    return rc1, rc2, o[:43], k[:1]


def test_outputs_are_fully_defined_whatever_they_held(capi, oracle_lib):
    c = C.case("asym_off:257")
    m_d = capi.to_dev(c["matches"])
    rc1, rc2, o, k = _raw(capi, m_d, 0, c)
    assert rc1 == 0 and rc2 == 0 and not o.any() and not k.any()                 # n = 0: all +0
    for n in (1, 257):
        rc1, rc2, o, k = _raw(capi, m_d, n, c)
        assert rc1 == 0 and rc2 == 0
        jtj, jtf, cost, alone = _run(capi, m_d, n, c)
        if n == 1:                                                              # no order enters: the same bits
            assert np.array_equal(o[:36], H.bits(jtj).reshape(-1)) and np.array_equal(o[36:42], H.bits(jtf))
            assert o[42] == np.float32(cost).view(np.uint32) and k[0] == np.float32(alone).view(np.uint32)
        of = o.view(np.float32)
        _structure(of[:36].reshape(6, 6), of[36:42], n)
        ref = C.reference(oracle_lib, "asym_off:257", n=n)
        got = C.got10(of[:36].reshape(6, 6), of[36:42], of[42])
        assert all(C.agrees(g, S, b) for g, S, b in zip(got, ref["S"], ref["bound"])), (n, got, ref["S"])
        assert C.agrees(k.view(np.float32)[0], ref["S"][9], ref["bound"][9])


def test_side_stream_without_host_sync(capi):
    import torch
    c = C.case("asym_off:257")
    m_d = capi.to_dev(c["matches"])
    _, _, o0, k0 = _raw(capi, m_d, 1, c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ms = capi.to_dev(c["matches"])                                           # upload, prefill, both calls, read-back:
        rc1, rc2, o1, k1 = _raw(capi, ms, 1, c)                                  # all ordered by the side stream alone
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(o0, o1) and np.array_equal(k0, k1)
    torch.cuda.synchronize()


def test_null_arguments_are_refused(capi):
    c = C.case("asym_off:2")
    m_d = capi.to_dev(c["matches"])
    null = capi.c_vp(0)
    for name in ("matches", "pose", "query", "target"):
        rc1, rc2, o, k = _raw(capi, m_d, 2, c, {name: null})
        assert rc1 == INVALID_ARG and rc2 == INVALID_ARG, name
        assert (o == 0xA5A5A5A5).all() and (k == 0xA5A5A5A5).all(), name        # refused before anything is written
    rc1, rc2, o, k = _raw(capi, m_d, 2, c, {"out": null, "cost": null})
    assert rc1 == INVALID_ARG and rc2 == INVALID_ARG
