"""Dense stereo on the GPU (ssrlcv_hip_stereo_sad_u8, _stereo_matches, _stereo_points; include/ssrlcv_hip.h "dense stereo")
against the numpy restatement of the contract (tests/stereo_ref.py) on the cases of tests/stereo_cases.py
(tests/test_stereo_cases.py proves without a GPU that they test something).  Every comparison is exact: disparities as bit
patterns and costs over the whole map, the border included; the Match records byte for byte; the points bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import stereo_cases as C
import stereo_ref as R

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
u32, csz, vp, cint, f32 = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)


def raw(t):
    """the bytes of a device tensor"""
    return t.cpu().numpy().tobytes()


def run(capi, name, want_cost=True):
    c = C.CASES[name]
    left, right = C.scene(c)
    disp, cost = capi.stereo_disparity(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), c.r, c.dmin, c.D, c.max_cost, c.lr,
                                       bool(c.subpixel), want_cost=want_cost)
    return disp, cost


def assert_maps_equal(name, disp, cost):
    ref = C.reference(name)
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


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_disparity_and_cost_equal_the_reference(capi, name):
    disp, cost = run(capi, name)
    assert_maps_equal(name, disp, cost)


@pytest.mark.parametrize("name", ["base_r4", "all_256", "narrower_than_window"])
def test_cost_may_be_null(capi, name):
    disp, cost = run(capi, name, want_cost=False)
    assert cost is None
    assert_maps_equal(name, disp, None)


@pytest.mark.parametrize("name,step", [("base_r1", 1), ("base_r1", 3), ("odd_pitch_r15", 3), ("all_256", 1), ("one_column", 1),
                                       ("narrower_than_window", 1), ("wide_range", 0xFFFFFFFF)])
def test_matches_and_points_equal_the_reference(capi, name, step):
    ref = C.reference(name)
    disp = torch.from_numpy(ref["disparity"].copy()).cuda()   # the reference's map: this test is about the two later calls
    want = R.matches_ref(ref["disparity"], step, 3, 7)
    got_d, n = capi.stereo_matches(disp, step, 3, 7)
    assert n == len(want)
    assert raw(got_d) == want.tobytes()                       # the records' bytes as they lie on the device, padding (zero) included
    pts = capi.stereo_points(got_d, n, **CAMERA).cpu().numpy()
    want_pts = R.points_ref(want, **CAMERA)
    assert np.array_equal(H.bits(pts), H.bits(want_pts))
    if n:
        assert np.isfinite(pts).all()


@pytest.mark.parametrize("step,grid", [(1, (5, 7)), (3, (2, 3)), (4, (2, 2)), (6, (1, 2)), (7, (1, 1)), (0x7FFFFFFF, (1, 1)),
                                       (0xFFFFFFF9, (1, 1)), (0xFFFFFFFB, (1, 1)), (0xFFFFFFFF, (1, 1))])
def test_sampling_grid_of_any_step_on_a_hand_made_map(capi, step, grid):
    """the entry point takes any disparity map: here every pixel of a 7 x 5 map is valid, pixel (0, 0) included, so the count is
    the grid's size ceil(h / step) x ceil(w / step) whatever the step -- also where w + step - 1 or h + step - 1 passes 2^32
    (0xFFFFFFF9 + 7 and 0xFFFFFFFB + 5 are 2^32) -- and a step beyond the image leaves the one record of pixel (0, 0)"""
    h, w = 5, 7
    disp = (np.arange(h * w, dtype=np.float32).reshape(h, w) * 0.25 + 1.5)
    want = R.matches_ref(disp, step, 4, 9)
    assert len(want) == grid[0] * grid[1] == len(range(0, h, step)) * len(range(0, w, step))
    got_d, n = capi.stereo_matches(torch.from_numpy(disp).cuda(), step, 4, 9)
    assert n == len(want)
    assert raw(got_d) == want.tobytes()
    if grid == (1, 1):
        rec = np.frombuffer(raw(got_d), H.MATCH)
        assert rec["kp0_loc"].tolist() == [[0.0, 0.0]] and rec["kp1_loc"].tolist() == [[-1.5, 0.0]] and rec["invalid"][0] == 0
    # with capacity 0 and no output buffer the same count comes back
    ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_stereo_matches_workspace_bytes(u32(w), u32(h), u32(step))))
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(capi.LIB.ssrlcv_hip_stereo_matches(capi.ptr(torch.from_numpy(disp).cuda()), u32(w), u32(h), u32(step), cint(4), cint(9), vp(None),
                                                  u32(0), capi.ptr(count), capi.ptr(ws), csz(ws.numel()), capi.stream_ptr()))
    assert int(count.item()) == len(want)


def test_points_of_invalid_and_behind_the_camera_matches_are_zero(capi):
    m = np.zeros(6, H.MATCH)
    m["kp0_loc"] = [[10, 5], [10, 5], [10, 5], [10, 5], [3, 2], [40, 30]]
    m["kp1_loc"] = [[4, 5], [4, 5], [13.5, 5], [14, 5], [1, 2], [40.25, 30]]   # d = 6, 6, -3.5, -4, 2, -0.25
    m["invalid"] = [0, 1, 0, 0, 0, 0]
    want = R.points_ref(m, **CAMERA)
    assert (want[1] == 0).all() and (want[2] == 0).all() and (want[3] == 0).all() and want[0, 2] > 0 and want[5, 2] > 0
    got = capi.stereo_points(capi.to_dev(m), len(m), **CAMERA).cpu().numpy()
    assert np.array_equal(H.bits(got), H.bits(want))


def test_capacity_guards(capi):
    """the full count comes back, the first `capacity` records are written and nothing behind them is touched"""
    ref = C.reference("base_r4")
    disp = torch.from_numpy(ref["disparity"].copy()).cuda()
    want = R.matches_ref(ref["disparity"], 1, 0, 1)
    h, w = ref["disparity"].shape
    need = int(capi.LIB.ssrlcv_hip_stereo_matches_workspace_bytes(u32(w), u32(h), u32(1)))
    ws = capi.dev_bytes(need)
    assert len(want) > 4200
    for cap in (1, 100, 4097):   # inside the first run of a wave, and past the first block's 4096 elements
        buf = torch.full(((cap + 16) * 40,), 0xA5, dtype=torch.uint8, device="cuda")   # cap records + 16 guard records
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        capi.check(capi.LIB.ssrlcv_hip_stereo_matches(capi.ptr(disp), u32(w), u32(h), u32(1), cint(0), cint(1), capi.ptr(buf), u32(cap),
                                                      capi.ptr(count), capi.ptr(ws), csz(ws.numel()), capi.stream_ptr()))
        assert int(count.item()) == len(want)
        host = buf.cpu().numpy()
        assert host[: cap * 40].tobytes() == want[:cap].tobytes()
        assert (host[cap * 40:] == 0xA5).all()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")   # capacity 0 with out == NULL: the count alone
    capi.check(capi.LIB.ssrlcv_hip_stereo_matches(capi.ptr(disp), u32(w), u32(h), u32(1), cint(0), cint(1), vp(None), u32(0),
                                                  capi.ptr(count), capi.ptr(ws), csz(ws.numel()), capi.stream_ptr()))
    assert int(count.item()) == len(want)


def test_a_side_stream_without_host_sync_gives_the_same(capi):
    name = "all_256"
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        disp, cost = capi.stereo_disparity(left_d, right_d, c.r, c.dmin, c.D, c.max_cost, c.lr, bool(c.subpixel))
        cap = c.w * c.h
        need = int(capi.LIB.ssrlcv_hip_stereo_matches_workspace_bytes(u32(c.w), u32(c.h), u32(1)))
        ws, out = capi.dev_bytes(need), capi.dev_bytes(cap * 40)
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        pts = torch.zeros((cap, 3), dtype=torch.float32, device="cuda")
        # the three calls back to back on the side stream; the host learns the count only after the last one
        capi.check(capi.LIB.ssrlcv_hip_stereo_matches(capi.ptr(disp), u32(c.w), u32(c.h), u32(1), cint(0), cint(1), capi.ptr(out), u32(cap),
                                                      capi.ptr(count), capi.ptr(ws), csz(ws.numel()), capi.stream_ptr()))
        want = R.matches_ref(C.reference(name)["disparity"], 1, 0, 1)
        capi.check(capi.LIB.ssrlcv_hip_stereo_points(capi.ptr(out), u32(len(want)), f32(CAMERA["foc"]), f32(CAMERA["baseline"]),
                                                     f32(CAMERA["doffset"]), f32(CAMERA["cx"]), f32(CAMERA["cy"]), capi.ptr(pts),
                                                     capi.stream_ptr()))
    side.synchronize()
    assert_maps_equal(name, disp, cost)
    assert int(count.item()) == len(want)
    assert raw(out[: 40 * len(want)]) == want.tobytes()
    assert np.array_equal(H.bits(pts.cpu().numpy()[: len(want)]), H.bits(R.points_ref(want, **CAMERA)))


def test_two_runs_are_bit_equal(capi):
    a, ca = run(capi, "wide_range")
    b, cb = run(capi, "wide_range")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)


def test_stereo_cloud_equals_the_three_calls(capi):
    from ssrlcv_amd import pipeline
    name = "base_r4"
    c = C.CASES[name]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    kw = dict(radius=c.r, min_disparity=c.dmin, num_disparities=c.D, max_cost=c.max_cost, lr_tolerance=c.lr, subpixel=bool(c.subpixel))
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, CAMERA["foc"], CAMERA["baseline"], CAMERA["doffset"], CAMERA["cx"],
                                                  CAMERA["cy"], step=3, left_id=2, right_id=5, **kw)
    d2, cost = pipeline.stereo_disparity(left_d, right_d, **kw)
    assert_maps_equal(name, d2, cost)
    m2, n2 = capi.stereo_matches(d2, 3, 2, 5)
    p2 = capi.stereo_points(m2, n2, **CAMERA)
    assert n == n2 > 100 and torch.equal(disp.view(torch.int32), d2.view(torch.int32)) and torch.equal(matches, m2)
    assert torch.equal(pts.view(torch.int32), p2.view(torch.int32))
    # the defaults: the principal point at the image centre
    p3 = pipeline.stereo_cloud(left_d, right_d, CAMERA["foc"], CAMERA["baseline"], step=3, **kw)[0]
    p4 = capi.stereo_points(m2, n2, CAMERA["foc"], CAMERA["baseline"], 0.0, c.w / 2.0, c.h / 2.0)
    assert torch.equal(p3.view(torch.int32), p4.view(torch.int32))


def test_binders_refuse_what_they_would_misread(capi):
    """the C ABI reads maps with pitch w: a strided view, another dtype, or a host tensor is refused by the Python binders, and
    stereo_cloud, which computes no cost map, says so"""
    from ssrlcv_amd import pipeline
    c = C.CASES["base_r4"]
    left, right = C.scene(c)
    left_d, right_d = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    for bad in ((left_d[:, ::2], right_d[:, ::2]), (left_d.t(), right_d.t()), (left_d.float(), right_d.float()), (left_d.cpu(), right_d.cpu())):
        with pytest.raises(AssertionError):
            capi.stereo_disparity(bad[0], bad[1], c.r, c.dmin, c.D)
    disp = torch.from_numpy(C.reference("base_r4")["disparity"].copy()).cuda()
    for bad in (disp[:, ::2], disp.double(), disp.cpu()):
        with pytest.raises(AssertionError):
            capi.stereo_matches(bad, 1, 0, 1)
    with pytest.raises(TypeError, match="no cost map"):
        pipeline.stereo_cloud(left_d, right_d, 480.0, 0.12, want_cost=True)


def test_matches_triangulate_with_real_cameras(capi):
    """the Match records are the sparse path's: ssrlcv_hip_matchset_from_matches -> pipeline.triangulate with two synthetic
    cameras a baseline apart give a finite cloud in front of the cameras"""
    from ssrlcv_amd import pipeline
    c = C.CASES["base_r4"]
    left, right = C.scene(c)
    # disparities from 1 up: d = 0 would be a pair of parallel rays (a point at infinity)
    ref = R.disparity_ref(left, right, c.r, 1, 10, lr=1, subpixel=1)
    disp, _ = capi.stereo_disparity(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), c.r, 1, 10, lr_tolerance=1, subpixel=True)
    assert np.array_equal(H.bits(disp.cpu().numpy()), H.bits(ref["disparity"]))
    assert (ref["disparity"][ref["valid"]] >= 0.5).all()
    matches, n = capi.stereo_matches(disp, 2, 0, 1)
    assert n > 500
    kp_d, mm_d, _ = capi.matchset_from_matches(capi.OUT_MATCH, matches, n)
    kp = capi.to_host(kp_d, H.KEYPOINT, 2 * n)
    mm = capi.to_host(mm_d, H.MULTIMATCH, n)
    want = R.matches_ref(ref["disparity"], 2, 0, 1)
    assert np.array_equal(kp["loc"][0::2], want["kp0_loc"]) and np.array_equal(kp["loc"][1::2], want["kp1_loc"])
    assert (kp["parentId"][0::2] == 0).all() and (kp["parentId"][1::2] == 1).all()
    assert (mm["numKeyPoints"] == 2).all() and np.array_equal(mm["index"], 2 * np.arange(n))
    cams = np.zeros(2, H.CAMERA)
    for i, x in enumerate((0.0, 0.5)):   # two cameras looking down +z, the right one a baseline along +x
        cams[i]["cam_pos"] = (x, 0.0, 0.0)
        cams[i]["cam_rot"] = (0.0, 0.0, 0.0)
        cams[i]["foc"] = 0.05
        cams[i]["dpix"] = (0.0001, 0.0001)
        cams[i]["fov"] = (0.2, 0.2)
        cams[i]["size"] = (c.w, c.h)
    cloud = pipeline.triangulate(mm, kp, cams, nview=False).cpu().numpy()
    assert cloud.shape == (n, 3) and np.isfinite(cloud).all()
    # disparities of the scene are positive: every pair of rays meets at a finite depth on one side of the cameras
    d = want["kp0_loc"][:, 0] - want["kp1_loc"][:, 0]
    z = cloud[d > 1.0, 2]
    assert len(z) > 400 and ((z > 0).all() or (z < 0).all())


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory + PointCloudFactory::stereo_disparity (tests/cpp/stereo_test.cpp) write what the Python path gives"""
    name = "base_r1"
    c = C.CASES[name]
    left, right = C.scene(c)
    lraw, rraw, prefix = str(tmp_path / "left.raw"), str(tmp_path / "right.raw"), str(tmp_path / "out")
    left.tofile(lraw)
    right.tofile(rraw)
    host = os.path.join(ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/stereo_test"])
    args = [os.path.join(host, "_build", "stereo_test"), lraw, rraw, str(c.w), str(c.h), str(c.r), str(c.dmin), str(c.D), str(c.lr),
            str(c.subpixel), "3", repr(CAMERA["foc"]), repr(CAMERA["baseline"]), repr(CAMERA["doffset"]), repr(CAMERA["cx"]),
            repr(CAMERA["cy"]), prefix]
    out = subprocess.check_output(args, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    ref = C.reference(name)
    assert np.array_equal(np.fromfile(prefix + ".disparity", np.uint32).reshape(c.h, c.w), H.bits(ref["disparity"]))
    assert np.array_equal(np.fromfile(prefix + ".cost", np.uint32).reshape(c.h, c.w), ref["cost"])
    disp, _ = run(capi, name)
    m_d, n = capi.stereo_matches(disp, 3, 0, 1)
    assert n > 0 and ("count %d" % n) in out
    assert np.fromfile(prefix + ".matches", np.uint8).tobytes() == raw(m_d)
    pts = capi.stereo_points(m_d, n, **CAMERA).cpu().numpy()
    assert np.array_equal(np.fromfile(prefix + ".points", np.uint32).reshape(-1, 3), H.bits(pts))
