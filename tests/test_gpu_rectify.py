"""Rectification on the GPU (ssrlcv_hip_warp_homography_u8, _stereo_mask_rectified, _matches_apply_homography; include/ssrlcv_hip.h
"rectification") against the numpy restatement of the contract (tests/rectify_ref.py) on the cases of tests/rectify_cases.py
(tests/test_rectify_cases.py proves without a GPU that they test something).  Every comparison is exact: image bytes, disparities
as bit patterns, costs, the Match records byte for byte, padding included."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import rectify_cases as C
import rectify_ref as R

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
u32, vp = ctypes.c_uint32, ctypes.c_void_p
GUARD = 64


def raw(t):
    """the bytes of a device tensor"""
    return t.cpu().numpy().tobytes()


def recbytes(a):
    """the bytes of a record array as they lie in memory, padding included"""
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def h9(Hm):
    return (ctypes.c_float * 9)(*[float(v) for v in np.asarray(Hm, np.float32).reshape(9)])


def warp_guarded(capi, src, Hm, dw, dh, offset):
    """the warp into the middle of a 0xA5 buffer, `offset` bytes past a 256-byte boundary -> (output, guards intact, source intact)"""
    sh, sw = src.shape
    sbuf = torch.full((2 * GUARD + sw * sh,), 0x5A, dtype=torch.uint8, device="cuda")
    sbuf[GUARD:GUARD + sw * sh] = torch.from_numpy(src.reshape(-1)).cuda()
    before = sbuf.clone()
    dbuf = torch.full((2 * GUARD + dw * dh,), 0xA5, dtype=torch.uint8, device="cuda")
    assert dbuf.data_ptr() % 256 == 0
    capi.check(capi.LIB.ssrlcv_hip_warp_homography_u8(vp(sbuf.data_ptr() + GUARD), u32(sw), u32(sh), h9(Hm), vp(dbuf.data_ptr() + offset),
                                                      u32(dw), u32(dh), capi.stream_ptr()))
    host = dbuf.cpu().numpy()
    guards = bool((host[:offset] == 0xA5).all() and (host[offset + dw * dh:] == 0xA5).all())
    return host[offset:offset + dw * dh].reshape(dh, dw), guards, torch.equal(sbuf, before)


@pytest.mark.parametrize("name", sorted(C.WARP_CASES))
def test_warp_equals_the_reference(capi, name):
    c = C.WARP_CASES[name]
    src, Hm, want = C.warp_reference(name)
    # the rows' first bytes on every residue of a dword boundary (the one large case: an odd pitch walks through them itself)
    for offset in ((GUARD - 1,) if c.dw * c.dh > (1 << 20) else (GUARD, GUARD - 3, GUARD - 2, GUARD - 1)):
        got, guards, source_intact = warp_guarded(capi, src, Hm, c.dw, c.dh, offset)
        ne = got != want
        assert not ne.any(), (name, offset, "differs at %d of %d pixels, first (y, x) %s: got %s want %s" % (
            int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4]))
        assert guards, (name, offset, "bytes outside dst were written")
        assert source_intact, (name, offset)


def test_warp_binder_and_refusals_of_what_it_would_misread(capi):
    src, Hm, want = C.warp_reference("67x45/rig_Hl/65x3")
    src_d = torch.from_numpy(src).cuda()
    assert np.array_equal(capi.warp_homography(src_d, Hm, (3, 65)).cpu().numpy(), want)
    assert tuple(capi.warp_homography(src_d, C.IDENTITY).shape) == src.shape and torch.equal(capi.warp_homography(src_d, C.IDENTITY), src_d)
    assert capi.warp_homography(src_d, Hm, (0, 65)).numel() == 0          # a dst of 0 pixels
    for bad in (src_d[:, ::2], src_d.t(), src_d.float(), src_d.cpu()):
        with pytest.raises(AssertionError):
            capi.warp_homography(bad, Hm)
    with pytest.raises(AssertionError):
        capi.warp_homography(src_d, np.zeros(8, np.float32))


# ---- the mask
def rect_of(Hl, Hr, w, h):
    r = np.zeros(1, C_RECT())[0]
    r["Hl"], r["Hr"], r["w"], r["h"] = Hl, Hr, w, h
    return r


def C_RECT():
    from ssrlcv_amd import capi
    return capi.RECTIFICATION


@pytest.mark.parametrize("with_cost", [True, False])
def test_mask_equals_the_reference_on_the_hand_made_map(capi, with_cost):
    disp, cost = C.mask_map()
    want, want_cost = R.mask_ref(disp, cost if with_cost else None, C.MASK_R, C.MASK_HL, C.MASK_HR, *C.MASK_SRC)
    disp_d = torch.from_numpy(disp.copy()).cuda()
    cost_d = torch.from_numpy(cost.view(np.int32).copy()).cuda() if with_cost else None
    capi.stereo_mask_rectified(disp_d, cost_d, C.MASK_R, rect_of(C.MASK_HL, C.MASK_HR, *C.MASK_SRC))
    assert np.array_equal(H.bits(disp_d.cpu().numpy()), H.bits(want))
    if with_cost:
        assert np.array_equal(cost_d.cpu().numpy().view(np.uint32), want_cost)
    for bad in (disp_d[:, ::2], disp_d.double(), disp_d.cpu()):
        with pytest.raises(AssertionError):
            capi.stereo_mask_rectified(bad, None, C.MASK_R, rect_of(C.MASK_HL, C.MASK_HR, *C.MASK_SRC))


def test_mask_equals_the_reference_past_one_launch_of_lanes(capi):
    disp, Hl, Hr, src = C.big_mask_map()
    want, _ = R.mask_ref(disp, None, 3, Hl, Hr, *src)
    disp_d = torch.from_numpy(disp.copy()).cuda()
    capi.stereo_mask_rectified(disp_d, None, 3, rect_of(Hl, Hr, *src))
    assert np.array_equal(H.bits(disp_d.cpu().numpy()), H.bits(want))


def test_mask_equals_the_reference_on_the_scene_pair_s_map(capi):
    s, ref = C.scene_pair(), C.chain_reference()
    st = ref["stereo"]
    disp_d = torch.from_numpy(st["disparity"].copy()).cuda()   # the reference's map: this test is about the mask alone
    cost_d = torch.from_numpy(st["cost"].view(np.int32).copy()).cuda()
    capi.stereo_mask_rectified(disp_d, cost_d, C.CHAIN.r, s["rect"])
    assert np.array_equal(H.bits(disp_d.cpu().numpy()), H.bits(ref["disparity"]))
    assert np.array_equal(cost_d.cpu().numpy().view(np.uint32), ref["cost"])


# ---- the records
@pytest.mark.parametrize("sides", ["both", "left_null", "right_null", "none"])
def test_apply_equals_the_reference(capi, sides):
    m = C.apply_records()
    H0 = None if sides in ("left_null", "none") else C.APPLY_H0
    H1 = None if sides in ("right_null", "none") else C.APPLY_H1
    want = R.apply_ref(m, H0, H1)
    guard = np.full(80, 0xA5, np.uint8)
    buf = torch.from_numpy(np.concatenate([guard, m.view(np.uint8), guard])).cuda()
    got = capi.matches_apply_homography(buf[80:80 + 40 * len(m)], len(m), H0, H1)
    assert raw(got) == recbytes(want)            # every byte, padding included
    host = buf.cpu().numpy()
    assert (host[:80] == 0xA5).all() and (host[-80:] == 0xA5).all()
    if sides == "both":
        assert want["invalid"][5] == 1           # the record whose W is exactly 0
        # n = 0 touches nothing; fewer than all leaves the rest alone
        buf2 = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        capi.matches_apply_homography(buf2, 0, H0, H1)
        assert raw(buf2) == recbytes(m)
        capi.matches_apply_homography(buf2, 257, H0, H1)
        assert raw(buf2) == recbytes(want[:257]) + recbytes(m[257:])


# ---- the chain on the scene pair
def scene_on_device():
    s = C.scene_pair()
    return torch.from_numpy(s["left"]).cuda(), torch.from_numpy(s["right"]).cuda(), s["cams"][0], s["cams"][1]


def chain_args():
    t = C.truth()
    return dict(radius=C.CHAIN.r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=C.CHAIN.lr, subpixel=bool(C.CHAIN.subpixel))


def run_chain(capi):
    from ssrlcv_amd import pipeline
    left_d, right_d, cam_l, cam_r = scene_on_device()
    left_r, right_r, rect = pipeline.rectify_pair(left_d, right_d, cam_l, cam_r)
    disp, cost = pipeline.stereo_disparity(left_r, right_r, **chain_args())
    capi.stereo_mask_rectified(disp, cost, C.CHAIN.r, rect)
    return left_r, right_r, disp, cost, rect


def assert_chain_equals_reference(left_r, right_r, disp, cost):
    ref = C.chain_reference()
    assert np.array_equal(left_r.cpu().numpy(), ref["left_r"]) and np.array_equal(right_r.cpu().numpy(), ref["right_r"])
    ne = H.bits(disp.cpu().numpy()) != H.bits(ref["disparity"])
    assert not ne.any(), "disparity differs at %d pixels, first (y, x) %s" % (int(ne.sum()), tuple(np.argwhere(ne)[0]))
    assert np.array_equal(cost.cpu().numpy().view(np.uint32), ref["cost"])


def test_the_chain_equals_the_reference_chain(capi):
    """rectify_pair -> stereo_disparity -> the mask, bit for bit: the floors tests/test_rectify_cases.py asserts on the reference
    (valid pixels, share within half a pixel of the ground truth, largest error) hold for the GPU with no tolerance"""
    left_r, right_r, disp, cost, rect = run_chain(capi)
    assert_chain_equals_reference(left_r, right_r, disp, cost)
    assert rect.tobytes() == C.scene_pair()["rect"].tobytes()


def test_a_side_stream_without_host_sync_gives_the_same_and_two_runs_are_bit_equal(capi):
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = run_chain(capi)   # five launches back to back on the side stream; nothing reads a result in between
    side.synchronize()
    assert_chain_equals_reference(*a[:4])
    b = run_chain(capi)
    for x, y in zip(a[:4], b[:4]):
        assert raw(x) == raw(y)


def test_stereo_cloud_cameras_equals_its_steps_and_lies_on_the_ground(capi):
    from ssrlcv_amd import pipeline
    import scene as scene_mod
    s, t = C.scene_pair(), C.truth()
    left_d, right_d, cam_l, cam_r = scene_on_device()
    step = 2
    pts, matches, n, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, **chain_args())
    # the steps one by one
    left_r, right_r, disp2, _, rect2 = run_chain(capi)
    assert rect.tobytes() == rect2.tobytes() and raw(disp) == raw(disp2)
    m2, n2 = capi.stereo_matches(disp2, step, 0, 1)
    rectified = np.frombuffer(raw(m2), H.MATCH)   # the bytes as they lie on the device: a field-wise copy would drop the padding
    capi.matches_apply_homography(m2, n2, rect["Hl"], rect["Hr"])
    want = R.apply_ref(rectified, rect["Hl"], rect["Hr"])
    assert raw(m2) == recbytes(want) and not want["invalid"].any()       # every record maps back: nothing to compact
    assert n == n2 > 7000 and raw(matches) == raw(m2)
    kp_d, mm_d, _ = capi.matchset_from_matches(capi.OUT_MATCH, m2, n2)
    cams = s["cams"]
    p2 = pipeline.triangulate(capi.to_host(mm_d, H.MULTIMATCH, n2), capi.to_host(kp_d, H.KEYPOINT, 2 * n2), cams, nview=False)
    assert tuple(pts.shape) == (n, 3) and raw(pts) == raw(p2)
    with pytest.raises(TypeError, match="no cost map"):
        pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, want_cost=True)
    # the matches are in source pixels with the cameras' ids: the left point is Hl of a pixel of the sampling grid
    got = np.frombuffer(raw(matches), H.MATCH)
    assert (got["kp0_parent"] == 0).all() and (got["kp1_parent"] == 1).all()
    assert (rectified["kp0_loc"] % step == 0).all()
    # the cloud is finite and in the world frame of rig.ground_points: within the depth of 1.5 px of its left pixel's ground point
    cloud = pts.cpu().numpy().astype(np.float64)
    assert np.isfinite(cloud).all()
    rig = s["rig"]
    ground = rig.ground_points(s["scene"], C.CHAIN.views[0], torch.from_numpy(got["kp0_loc"][:, 0].astype(np.float64)),
                               torch.from_numpy(got["kp0_loc"][:, 1].astype(np.float64)))[0].numpy()
    Rn = scene_mod._euler_matrix(rect["cam_rot"])
    Z = ((ground - cam_l["cam_pos"].astype(np.float64)) @ Rn)[:, 2]
    per_pixel = Z.mean() ** 2 / (float(rect["foc"]) * float(rect["baseline"]))   # km of depth per pixel of disparity
    dist = np.linalg.norm(cloud - ground, axis=1)
    print("cloud of %d points: median %.3f km, largest %.3f km from the ground truth; %.3f km per pixel" % (
        n, np.median(dist), dist.max(), per_pixel))
    assert dist.max() <= 1.5 * per_pixel


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory::rectify, maskRectified and unrectifyMatches (tests/cpp/rectify_test.cpp) write what the Python path gives"""
    s, t = C.scene_pair(), C.truth()
    paths = {k: str(tmp_path / k) for k in ("left.raw", "right.raw", "left.cam", "right.cam", "out")}
    s["left"].tofile(paths["left.raw"])
    s["right"].tofile(paths["right.raw"])
    s["cams"][0:1].tofile(paths["left.cam"])
    s["cams"][1:2].tofile(paths["right.cam"])
    host = os.path.join(ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/rectify_test"])
    n, step = C.CHAIN.size, 3
    args = [os.path.join(host, "_build", "rectify_test"), paths["left.raw"], paths["right.raw"], str(n), str(n), paths["left.cam"],
            paths["right.cam"], str(C.CHAIN.r), str(t["dmin"]), str(t["D"]), str(C.CHAIN.lr), str(C.CHAIN.subpixel), str(step), paths["out"]]
    out = subprocess.check_output(args, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    left_r, right_r, disp, cost, rect = run_chain(capi)
    prefix = paths["out"]
    assert np.fromfile(prefix + ".left", np.uint8).tobytes() == raw(left_r) and np.fromfile(prefix + ".right", np.uint8).tobytes() == raw(right_r)
    assert np.fromfile(prefix + ".disparity", np.uint8).tobytes() == raw(disp)
    assert np.fromfile(prefix + ".cost", np.uint8).tobytes() == raw(cost)
    m_d, count = capi.stereo_matches(disp, step, 0, 1)
    capi.matches_apply_homography(m_d, count, rect["Hl"], rect["Hr"])
    assert count > 0 and ("count %d" % count) in out
    assert np.fromfile(prefix + ".matches", np.uint8).tobytes() == raw(m_d)
