"""The census cost on the GPU (ssrlcv_hip_census_u8, ssrlcv_hip_stereo_census_u8, ssrlcv_hip_stereo_sgm_census_u8;
include/ssrlcv_hip.h "census cost") against the numpy restatement of the contract (tests/census_ref.py) on the cases of
tests/census_cases.py (tests/test_census_cases.py proves without a GPU that they test something).  Every comparison is exact:
codes as 64-bit patterns, disparities as bit patterns and costs over the whole map, the border included."""
import os
import subprocess

import numpy as np
import pytest
import torch

import census_cases as C
import census_ref as CR
import helpers as H

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)


def raw(t):
    return t.cpu().numpy().tobytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bm_args(c):
    return dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, max_cost=c.max_cost, lr_tolerance=c.lr, subpixel=bool(c.subpixel),
                census=c.c)


def sgm_args(c):
    return dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, cost_clamp=c.clamp, p1=c.P1, p2=c.P2, paths=c.paths,
                lr_tolerance=c.lr, subpixel=bool(c.subpixel), census=c.c)


def run(capi, name, want_cost=True, workspace=None):
    c = C.CASES[name]
    left, right = C.scene(c)
    return capi.stereo_disparity(dev(left), dev(right), want_cost=want_cost, workspace=workspace, **bm_args(c))


def run_sgm(capi, name, want_cost=True, workspace=None):
    c = C.SGM_CASES[name]
    left, right = C.scene(c)
    return capi.stereo_sgm(dev(left), dev(right), want_cost=want_cost, workspace=workspace, **sgm_args(c))


def assert_maps_equal(name, disp, cost, ref):
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


@pytest.mark.parametrize("c", [1, 2, 3])
def test_codes_equal_the_reference(capi, c):
    """every case's left image, and images smaller than the window: every entry is written, 0 on the border"""
    images = [C.scene(case)[0] for _, case in sorted(C.CASES.items())]
    images += [np.full((2 * c, 9), 200, np.uint8), np.arange(7 * (2 * c), dtype=np.uint8).reshape(7, 2 * c), np.zeros((1, 1), np.uint8)]
    seen = 0
    for img in images:
        got = capi.census(dev(img), c).cpu().numpy().view(np.uint64)
        want = CR.census(img, c)
        ne = got != want
        assert not ne.any(), (img.shape, c, "codes differ at %d pixels, first (y, x) %s" % (int(ne.sum()), tuple(np.argwhere(ne)[0])))
        seen = max(seen, int(want.max()).bit_length())
    assert seen == CR.bits(c)      # the last bit of the code is met


@pytest.mark.parametrize("name", C.ALL)
def test_block_matching_equals_the_reference(capi, name):
    disp, cost = run(capi, name)
    assert_maps_equal(name, disp, cost, C.reference(name))


@pytest.mark.parametrize("name", C.SGM_ALL)
def test_semi_global_matching_equals_the_reference(capi, name):
    disp, cost = run_sgm(capi, name)
    assert_maps_equal(name, disp, cost, C.sgm_reference(name))


def test_cost_may_be_null(capi):
    for name in ("c3_r1", "all_256", "narrower_than_footprint"):
        disp, cost = run(capi, name, want_cost=False)
        assert cost is None
        assert_maps_equal(name, disp, None, C.reference(name))
    for name in ("c3_r1_4paths", "narrower_than_footprint"):
        disp, cost = run_sgm(capi, name, want_cost=False)
        assert cost is None
        assert_maps_equal(name, disp, None, C.sgm_reference(name))


def test_two_runs_are_bit_equal(capi):
    a, ca = run(capi, "c3_r7")
    b, cb = run(capi, "c3_r7")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
    a, ca = run_sgm(capi, "c2_r0_8paths")
    b, cb = run_sgm(capi, "c2_r0_8paths")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)


def test_a_second_call_on_the_same_workspace(capi):
    """the code maps, the winners' k and the volumes of one call do not leak into the next: other sizes, code widths, disparity
    counts and forms follow each other on the same bytes"""
    ws = capi.dev_bytes(64 << 20)
    ws.fill_(0xA5)
    for kind, name in (("sgm", "all_256"), ("bm", "all_256"), ("bm", "c3_r7"), ("sgm", "c3_r1_4paths"), ("bm", "c1_r0"), ("sgm", "d1"),
                       ("bm", "one_column"), ("sgm", "clamp0"), ("bm", "flat")):
        if kind == "bm":
            assert_maps_equal(name, *run(capi, name, workspace=ws), C.reference(name))
        else:
            assert_maps_equal(name, *run_sgm(capi, name, workspace=ws), C.sgm_reference(name))


def test_a_side_stream_without_host_sync_gives_the_same(capi):
    import stereo_ref as R
    c = C.CASES["all_256"]
    left, right = C.scene(c)
    left_d, right_d = dev(left), dev(right)
    s = C.SGM_CASES["c3_r1_4paths"]
    sl, sr = (dev(a) for a in C.scene(s))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        disp, cost = capi.stereo_disparity(left_d, right_d, want_cost=True, **bm_args(c))
        matches, n = capi.stereo_matches(disp, 2, 0, 1)   # the next stage behind it on the same stream
        sdisp, scost = capi.stereo_sgm(sl, sr, want_cost=True, **sgm_args(s))
    side.synchronize()
    assert_maps_equal("all_256", disp, cost, C.reference("all_256"))
    assert raw(matches) == R.matches_ref(C.reference("all_256")["disparity"], 2, 0, 1).tobytes()
    assert_maps_equal("c3_r1_4paths", sdisp, scost, C.sgm_reference("c3_r1_4paths"))


def test_the_maps_do_not_move_under_a_strictly_increasing_map_of_the_grey_levels(capi):
    """tests/test_census_cases.py test_radiometric_invariance, on the device: the three pairs give the same maps bit for bit,
    for block matching and for semi-global matching"""
    case, field, pairs = C.radiometric_pairs()
    kw = dict(min_disparity=case.dmin, num_disparities=case.D, lr_tolerance=1, subpixel=True, want_cost=True)
    bm = [capi.stereo_disparity(dev(l), dev(r), radius=2, census=2, **kw) for l, r in pairs]
    sg = [capi.stereo_sgm(dev(l), dev(r), radius=0, census=2, cost_clamp=24, p1=3, p2=20, **kw) for l, r in pairs]
    for maps in (bm, sg):
        for d, c in maps[1:]:
            assert torch.equal(d.view(torch.int32), maps[0][0].view(torch.int32)) and torch.equal(c, maps[0][1])
    ref = CR.census_disparity_ref(pairs[1][0], pairs[1][1], 2, 2, case.dmin, case.D, lr=1, subpixel=1)
    assert_maps_equal("gained pair", bm[1][0], bm[1][1], ref)
    valid = H.bits(bm[0][0].cpu().numpy()) != 0x7FC00000
    assert valid.sum() > 4000
    # SAD at the same footprint does move
    sad = [capi.stereo_disparity(dev(l), dev(r), radius=4, **kw)[0] for l, r in pairs[:2]]
    assert not torch.equal(sad[0].view(torch.int32), sad[1].view(torch.int32))


@pytest.mark.parametrize("name", ["p0_4paths", "p0_8paths"])
def test_without_penalties_it_is_the_block_matching_call(capi, name):
    """P1 = P2 = 0 and a clamp that cuts nothing: every L_i is the census cost itself, so the two entry points give the same
    disparity map bit for bit and the cost map is popcount(paths) times block matching's"""
    c = C.SGM_CASES[name]
    left, right = C.scene(c)
    left_d, right_d = dev(left), dev(right)
    disp, cost = capi.stereo_sgm(left_d, right_d, want_cost=True, **sgm_args(c))
    bd, bc = capi.stereo_disparity(left_d, right_d, c.r, c.dmin, c.D, capi.STEREO_NO_LIMIT, c.lr, bool(c.subpixel), census=c.c)
    assert torch.equal(disp.view(torch.int32), bd.view(torch.int32))
    bc = bc.cpu().numpy().view(np.uint32).astype(np.int64)
    want = np.where(bc == 0xFFFFFFFF, bc, bc * bin(c.paths).count("1"))
    assert np.array_equal(cost.cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert (bc != 0xFFFFFFFF).sum() > 4000


def test_census_zero_is_the_sad_call(capi):
    import sgm_cases as GC
    import stereo_cases as SC
    s = SC.CASES["base_r4"]
    left_d, right_d = (dev(a) for a in SC.scene(s))
    disp, cost = capi.stereo_disparity(left_d, right_d, s.r, s.dmin, s.D, s.max_cost, s.lr, bool(s.subpixel), True, None, 0)
    ref = SC.reference("base_r4")
    assert_maps_equal("base_r4", disp, cost, ref)
    g = GC.CASES["base_r4"]
    gl, gr = (dev(a) for a in GC.scene(g))
    disp, cost = capi.stereo_sgm(gl, gr, g.r, g.dmin, g.D, g.clamp, g.P1, g.P2, g.paths, g.lr, bool(g.subpixel), True, None, 0)
    assert_maps_equal("sgm base_r4", disp, cost, GC.reference("base_r4"))


def test_binders_refuse_what_they_would_misread(capi):
    c = C.CASES["c2_r2"]
    left, right = C.scene(c)
    left_d, right_d = dev(left), dev(right)
    for bad in ((left_d[:, ::2], right_d[:, ::2]), (left_d.t(), right_d.t()), (left_d.float(), right_d.float()), (left_d.cpu(), right_d.cpu()),
                (left_d, right_d[:-1])):
        with pytest.raises(AssertionError):
            capi.stereo_disparity(bad[0], bad[1], **bm_args(c))
        with pytest.raises(AssertionError):
            capi.stereo_sgm(bad[0], bad[1], census=2)
    for bad in (-1, 1 << 32, 2.0, True, "2", None):
        with pytest.raises(AssertionError):
            capi.stereo_disparity(left_d, right_d, census=bad)
        with pytest.raises(AssertionError):
            capi.stereo_sgm(left_d, right_d, census=bad)
        with pytest.raises(AssertionError):
            capi.census(left_d, bad)
    for bad in (left_d[:, ::2], left_d.float(), left_d.cpu(), left_d[0]):
        with pytest.raises(AssertionError):
            capi.census(bad, 2)
    with pytest.raises(capi.SsrlcvError):
        capi.census(left_d, 4)
    with pytest.raises(capi.SsrlcvError):
        capi.stereo_disparity(left_d, right_d, radius=8, census=2)


def test_stereo_cloud_with_census_equals_the_three_calls(capi):
    from ssrlcv_amd import pipeline
    name = "c2_r2"
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = dev(left), dev(right)
    kw = dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, lr_tolerance=c.lr, subpixel=bool(c.subpixel), census=2)
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, CAMERA["foc"], CAMERA["baseline"], CAMERA["doffset"], CAMERA["cx"],
                                                  CAMERA["cy"], step=3, left_id=2, right_id=5, **kw)
    d2, cost = pipeline.stereo_disparity(left_d, right_d, want_cost=True, **kw)
    assert_maps_equal(name, d2, cost, C.reference(name))
    m2, n2 = capi.stereo_matches(d2, 3, 2, 5)
    p2 = capi.stereo_points(m2, n2, **CAMERA)
    assert n == n2 > 100 and torch.equal(disp.view(torch.int32), d2.view(torch.int32)) and torch.equal(matches, m2)
    assert torch.equal(pts.view(torch.int32), p2.view(torch.int32))
    # and with semi-global matching over the census costs
    s = C.SGM_CASES["c2_r0_8paths"]
    skw = dict(radius=s.r, min_disparity=s.dmin, num_disparities=s.D, lr_tolerance=s.lr, subpixel=bool(s.subpixel), census=2)
    sgm = dict(cost_clamp=s.clamp, p1=s.P1, p2=s.P2, paths=s.paths)
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, CAMERA["foc"], CAMERA["baseline"], CAMERA["doffset"], CAMERA["cx"],
                                                  CAMERA["cy"], step=3, left_id=2, right_id=5, sgm=sgm, **skw)
    d3, cost3 = pipeline.stereo_sgm(left_d, right_d, want_cost=True, **sgm, **skw)
    assert_maps_equal("c2_r0_8paths", d3, cost3, C.sgm_reference("c2_r0_8paths"))
    m3, n3 = capi.stereo_matches(d3, 3, 2, 5)
    p3 = capi.stereo_points(m3, n3, **CAMERA)
    assert n == n3 > 100 and torch.equal(disp.view(torch.int32), d3.view(torch.int32)) and torch.equal(matches, m3)
    assert torch.equal(pts.view(torch.int32), p3.view(torch.int32)) and not torch.equal(d3.view(torch.int32), d2.view(torch.int32))


def test_stereo_cloud_cameras_with_census_masks_the_footprint(capi):
    """rectify_pair -> census block matching -> the mask on the rendered pair of rectify_cases.CHAIN, against rectify_ref +
    census_ref with the mask at rho = radius + census; the mask at the aggregation radius alone would keep pixels this one drops"""
    from ssrlcv_amd import pipeline
    import rectify_cases as RC
    import rectify_ref as RR
    s, t, ref = RC.scene_pair(), RC.truth(), RC.chain_reference()
    n = RC.CHAIN.size
    c, r = 2, 2
    kw = dict(radius=r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=RC.CHAIN.lr, subpixel=bool(RC.CHAIN.subpixel), census=c)
    left_d, right_d = dev(s["left"]), dev(s["right"])
    pts, matches, cnt, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, s["cams"][0], s["cams"][1], step=2, **kw)
    st = CR.census_disparity_ref(ref["left_r"], ref["right_r"], c, r, t["dmin"], t["D"], lr=RC.CHAIN.lr, subpixel=RC.CHAIN.subpixel)
    want, _ = RR.mask_ref(st["disparity"], st["cost"], r + c, s["rect"]["Hl"], s["rect"]["Hr"], n, n)
    narrow, _ = RR.mask_ref(st["disparity"], st["cost"], r, s["rect"]["Hl"], s["rect"]["Hr"], n, n)
    only_footprint = (H.bits(want) == 0x7FC00000) & (H.bits(narrow) != 0x7FC00000)
    assert only_footprint.sum() > 0      # the footprint, not the aggregation radius, decides some pixel
    ne = H.bits(disp.cpu().numpy()) != H.bits(want)
    assert not ne.any(), "disparity differs at %d pixels, first (y, x) %s" % (int(ne.sum()), tuple(np.argwhere(ne)[0]))
    assert cnt > 5000 and tuple(pts.shape) == (cnt, 3) and np.isfinite(pts.cpu().numpy()).all()


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory::setCensus + generateDisparities, with and without setSemiGlobal (tests/cpp/census_test.cpp), write
    what the Python path gives, and clearCensus() returns the factory to SAD's winners"""
    c, s = C.CASES["c3_r1"], C.SGM_CASES["c3_r1_4paths"]
    assert (c.w, c.h, c.c, c.r, c.dmin, c.D, c.lr, c.subpixel, c.seed) == (s.w, s.h, s.c, s.r, s.dmin, s.D, s.lr, s.subpixel, s.seed)
    left, right = C.scene(c)
    lraw, rraw, prefix = str(tmp_path / "left.raw"), str(tmp_path / "right.raw"), str(tmp_path / "out")
    left.tofile(lraw)
    right.tofile(rraw)
    host = os.path.join(ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/census_test"])
    a = [os.path.join(host, "_build", "census_test"), lraw, rraw, str(c.w), str(c.h), str(c.c), str(c.r), str(c.dmin), str(c.D), str(s.clamp),
         str(s.P1), str(s.P2), hex(s.paths), str(c.lr), str(c.subpixel), prefix]
    out = subprocess.check_output(a, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    disp, cost = run(capi, "c3_r1")
    assert np.fromfile(prefix + ".disparity", np.uint8).tobytes() == raw(disp)
    assert np.fromfile(prefix + ".cost", np.uint8).tobytes() == raw(cost)
    assert_maps_equal("c3_r1", disp, cost, C.reference("c3_r1"))
    sdisp, scost = run_sgm(capi, "c3_r1_4paths")
    assert np.fromfile(prefix + ".sgm.disparity", np.uint8).tobytes() == raw(sdisp) != raw(disp)
    assert np.fromfile(prefix + ".sgm.cost", np.uint8).tobytes() == raw(scost)
    sad, _ = capi.stereo_disparity(dev(left), dev(right), c.r + c.c, c.dmin, c.D, capi.STEREO_NO_LIMIT, c.lr, bool(c.subpixel))
    assert np.fromfile(prefix + ".sad.disparity", np.uint8).tobytes() == raw(sad) != raw(disp)


def test_pass_events_are_recorded_in_order_and_change_nothing(capi):
    """ssrlcv_hip_stereo_sgm_set_pass_events on the census call: 0x0F with the check records 1 + 1 + 4 + 1 + 1 events in stream
    order, the two census passes inside the second; the maps are the reference's with the hook, and after its removal"""
    name = "c3_r1_4paths"
    events = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    capi.stereo_sgm_set_pass_events(events)
    try:
        disp, cost = run_sgm(capi, name)
        torch.cuda.synchronize()
        assert all(e.query() for e in events)
        assert all(events[i].elapsed_time(events[i + 1]) >= 0 for i in range(7))
    finally:
        capi.stereo_sgm_set_pass_events(None)
    assert_maps_equal(name, disp, cost, C.sgm_reference(name))
    assert_maps_equal(name, *run_sgm(capi, name), C.sgm_reference(name))
