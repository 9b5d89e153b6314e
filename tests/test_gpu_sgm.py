"""Semi-global matching on the GPU (ssrlcv_hip_stereo_sgm_u8; include/ssrlcv_hip.h "semi-global matching") against the numpy
restatement of the contract (tests/sgm_ref.py) on the cases of tests/sgm_cases.py (tests/test_sgm_cases.py proves without a GPU
that they test something).  Every comparison is exact: disparities as bit patterns and costs over the whole map, the border
included."""
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import sgm_cases as C
import sgm_ref as G

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)


def raw(t):
    return t.cpu().numpy().tobytes()


def args(c):
    return dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, cost_clamp=c.clamp, p1=c.P1, p2=c.P2, paths=c.paths,
                lr_tolerance=c.lr, subpixel=bool(c.subpixel))


def run(capi, name, want_cost=True, workspace=None):
    c = C.CASES[name]
    left, right = C.scene(c)
    return capi.stereo_sgm(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), want_cost=want_cost, workspace=workspace, **args(c))


def assert_maps_equal(name, disp, cost, ref=None):
    ref = C.reference(name) if ref is None else ref
    got = H.bits(disp.cpu().numpy())
    want = H.bits(ref["disparity"])
    ne = got != want
    assert not ne.any(), (name, "disparity differs at %d of %d pixels, first (y, x) %s: got %s want %s" % (
        int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4]))
    if cost is not None:
        gc = cost.cpu().numpy().view(np.uint32)
        nc = gc != ref["cost"]
        assert not nc.any(), (name, "cost differs at %d pixels, first (y, x) %s: got %s want %s" % (
            int(nc.sum()), tuple(np.argwhere(nc)[0]), gc[nc][:4], ref["cost"][nc][:4]))


@pytest.mark.parametrize("name", C.ALL)
def test_disparity_and_cost_equal_the_reference(capi, name):
    disp, cost = run(capi, name)
    assert_maps_equal(name, disp, cost)


@pytest.mark.parametrize("name", ["base_r4", "all_256", "narrower_than_window"])
def test_cost_may_be_null(capi, name):
    disp, cost = run(capi, name, want_cost=False)
    assert cost is None
    assert_maps_equal(name, disp, None)


@pytest.mark.parametrize("name", ["p0_4paths", "p0_8paths"])
def test_without_penalties_it_is_the_sad_call(capi, name):
    """P1 = P2 = 0 and a clamp no 3 x 3 cost reaches: every L_i is the SAD cost itself, so the two entry points give the same
    disparity map bit for bit and the cost map is popcount(paths) times SAD's"""
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    disp, cost = capi.stereo_sgm(left_d, right_d, want_cost=True, **args(c))
    sd, sc = capi.stereo_disparity(left_d, right_d, c.r, c.dmin, c.D, capi.STEREO_NO_LIMIT, c.lr, bool(c.subpixel))
    assert torch.equal(disp.view(torch.int32), sd.view(torch.int32))
    sc = sc.cpu().numpy().view(np.uint32).astype(np.int64)
    want = np.where(sc == 0xFFFFFFFF, sc, sc * bin(c.paths).count("1"))
    assert np.array_equal(cost.cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert (sc != 0xFFFFFFFF).sum() > 5000


def test_a_side_stream_without_host_sync_gives_the_same(capi):
    name = "all_256"
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        disp, cost = capi.stereo_sgm(left_d, right_d, want_cost=True, **args(c))
        matches, n = capi.stereo_matches(disp, 2, 0, 1)   # the next stage behind it on the same stream
    side.synchronize()
    assert_maps_equal(name, disp, cost)
    import stereo_ref as R
    assert raw(matches) == R.matches_ref(C.reference(name)["disparity"], 2, 0, 1).tobytes()


def test_two_runs_are_bit_equal(capi):
    a, ca = run(capi, "wide_range")
    b, cb = run(capi, "wide_range")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)


def test_a_second_call_on_the_same_workspace(capi):
    """the volumes of one call -- their padded entries included -- do not leak into the next: D = 256 fills every entry, the
    calls behind it on the same bytes have other widths, other paths (so another direction stores S first) and padding"""
    ws = capi.dev_bytes(64 << 20)
    ws.fill_(0xA5)
    for name in ("all_256", "nd16_r12", "dir5", "d1", "base_r1", "tall_9x37", "clamp0"):
        disp, cost = run(capi, name, workspace=ws)
        assert_maps_equal(name, disp, cost)


def test_stereo_cloud_with_sgm_equals_the_three_calls(capi):
    from ssrlcv_amd import pipeline
    name = "base_r4"
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    kw = dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, lr_tolerance=c.lr, subpixel=bool(c.subpixel))
    sgm = dict(cost_clamp=c.clamp, p1=c.P1, p2=c.P2, paths=c.paths)
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, CAMERA["foc"], CAMERA["baseline"], CAMERA["doffset"], CAMERA["cx"],
                                                  CAMERA["cy"], step=3, left_id=2, right_id=5, sgm=sgm, **kw)
    d2, cost = pipeline.stereo_sgm(left_d, right_d, want_cost=True, **sgm, **kw)
    assert_maps_equal(name, d2, cost)
    m2, n2 = capi.stereo_matches(d2, 3, 2, 5)
    p2 = capi.stereo_points(m2, n2, **CAMERA)
    assert n == n2 > 100 and torch.equal(disp.view(torch.int32), d2.view(torch.int32)) and torch.equal(matches, m2)
    assert torch.equal(pts.view(torch.int32), p2.view(torch.int32))
    # paths is optional (0xFF); a cost limit has no meaning here; sgm = None is the SAD path as before
    d3 = pipeline.stereo_cloud(left_d, right_d, 480.0, 0.12, sgm=dict(cost_clamp=c.clamp, p1=c.P1, p2=c.P2), **kw)[3]
    assert torch.equal(d3.view(torch.int32), d2.view(torch.int32))
    with pytest.raises(TypeError, match="max_cost"):
        pipeline.stereo_cloud(left_d, right_d, 480.0, 0.12, sgm=sgm, max_cost=100, **kw)
    with pytest.raises(TypeError, match="cost_clamp"):
        pipeline.stereo_cloud(left_d, right_d, 480.0, 0.12, sgm=dict(p1=1, p2=2), **kw)
    d4 = pipeline.stereo_cloud(left_d, right_d, 480.0, 0.12, sgm=None, **kw)[3]
    d5, _ = pipeline.stereo_disparity(left_d, right_d, **kw)
    assert torch.equal(d4.view(torch.int32), d5.view(torch.int32)) and not torch.equal(d4.view(torch.int32), d2.view(torch.int32))


def test_binders_refuse_what_they_would_misread(capi):
    c = C.CASES["base_r4"]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    for bad in ((left_d[:, ::2], right_d[:, ::2]), (left_d.t(), right_d.t()), (left_d.float(), right_d.float()), (left_d.cpu(), right_d.cpu()),
                (left_d, right_d[:-1])):
        with pytest.raises(AssertionError):
            capi.stereo_sgm(bad[0], bad[1], **args(c))


def test_stereo_cloud_cameras_with_sgm_equals_the_numpy_chain(capi):
    """rectify_pair -> stereo_sgm -> the mask on the rendered pair of rectify_cases.CHAIN, against rectify_ref + sgm_ref"""
    from ssrlcv_amd import pipeline
    import rectify_cases as RC
    import rectify_ref as RR
    s, t, ref = RC.scene_pair(), RC.truth(), RC.chain_reference()
    n = RC.CHAIN.size
    sgm = dict(cost_clamp=3000, p1=100, p2=1200)
    kw = dict(radius=RC.CHAIN.r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=RC.CHAIN.lr, subpixel=bool(RC.CHAIN.subpixel))
    left_d, right_d = torch.from_numpy(s["left"]).cuda(), torch.from_numpy(s["right"]).cuda()
    pts, matches, cnt, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, s["cams"][0], s["cams"][1], step=2, sgm=sgm, **kw)
    st = G.sgm_ref(ref["left_r"], ref["right_r"], RC.CHAIN.r, t["dmin"], t["D"], 3000, 100, 1200, 0xFF, RC.CHAIN.lr, RC.CHAIN.subpixel)
    want, _ = RR.mask_ref(st["disparity"], st["cost"], RC.CHAIN.r, s["rect"]["Hl"], s["rect"]["Hr"], n, n)
    ne = H.bits(disp.cpu().numpy()) != H.bits(want)
    assert not ne.any(), "disparity differs at %d pixels, first (y, x) %s" % (int(ne.sum()), tuple(np.argwhere(ne)[0]))
    assert not np.array_equal(H.bits(want), H.bits(ref["disparity"]))   # not the SAD chain's map
    assert cnt > 7000 and tuple(pts.shape) == (cnt, 3) and np.isfinite(pts.cpu().numpy()).all()
    with pytest.raises(TypeError, match="max_cost"):
        pipeline.stereo_cloud_cameras(left_d, right_d, s["cams"][0], s["cams"][1], sgm=sgm, max_cost=5, **kw)


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory::setSemiGlobal + generateDisparities (tests/cpp/sgm_test.cpp) write what the Python path gives, and
    clearSemiGlobal() returns the factory to SAD's winners"""
    name = "base_r1"
    c = C.CASES[name]
    left, right = C.scene(c)
    lraw, rraw, prefix = str(tmp_path / "left.raw"), str(tmp_path / "right.raw"), str(tmp_path / "out")
    left.tofile(lraw)
    right.tofile(rraw)
    host = os.path.join(ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/sgm_test"])
    a = [os.path.join(host, "_build", "sgm_test"), lraw, rraw, str(c.w), str(c.h), str(c.r), str(c.dmin), str(c.D), str(c.clamp), str(c.P1),
         str(c.P2), hex(c.paths), str(c.lr), str(c.subpixel), prefix]
    out = subprocess.check_output(a, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    disp, cost = run(capi, name)
    assert np.fromfile(prefix + ".disparity", np.uint8).tobytes() == raw(disp)
    assert np.fromfile(prefix + ".cost", np.uint8).tobytes() == raw(cost)
    assert_maps_equal(name, disp, cost)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    sad, _ = capi.stereo_disparity(left_d, right_d, c.r, c.dmin, c.D, capi.STEREO_NO_LIMIT, c.lr, bool(c.subpixel))
    assert np.fromfile(prefix + ".sad.disparity", np.uint8).tobytes() == raw(sad) != raw(disp)


def test_pass_events_are_recorded_in_order_and_change_nothing(capi):
    """ssrlcv_hip_stereo_sgm_set_pass_events (tools/bench_sgm.py's hook): 0x0F with the check records 1 + 1 + 4 + 1 + 1 events
    in stream order; the maps are the reference's with the hook, and after its removal"""
    name = "base_r1_4paths"
    events = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    capi.stereo_sgm_set_pass_events(events)
    try:
        disp, cost = run(capi, name)
        torch.cuda.synchronize()
        assert all(e.query() for e in events)
        assert all(events[i].elapsed_time(events[i + 1]) >= 0 for i in range(7))
    finally:
        capi.stereo_sgm_set_pass_events(None)
    assert_maps_equal(name, disp, cost)
    assert_maps_equal(name, *run(capi, name))
