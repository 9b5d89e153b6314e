"""The disparity post-filters on the GPU (ssrlcv_hip_disparity_components, ssrlcv_hip_stereo_filter_speckles,
ssrlcv_hip_stereo_filter_median; include/ssrlcv_hip.h "disparity post-filters") against the numpy restatement of the contract
(tests/speckle_ref.py) on the cases of tests/speckle_cases.py (tests/test_speckle_cases.py proves without a GPU that they test
something).  Every comparison is exact: labels and sizes as uint32, disparities as bit patterns, costs over the whole map."""
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import speckle_cases as S
import speckle_ref as R

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
CAMERA = dict(foc=480.0, baseline=0.12, doffset=3.5, cx=47.25, cy=36.5)


def raw(t):
    return t.cpu().numpy().tobytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_same(name, what, got, want):
    ne = got != want
    assert not ne.any(), (name, "%s differs at %d of %d pixels, first (y, x) %s: got %s want %s" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4]))


def cost_map(d):
    """a cost map with a value of its own at every pixel, UINT32_MAX where the map is invalid as the matching calls leave it"""
    cost = (np.arange(d.size, dtype=np.uint32).reshape(d.shape) * np.uint32(2654435761)) >> np.uint32(8)
    cost[~R.valid_mask(d)] = 0xFFFFFFFF
    return cost


@pytest.mark.parametrize("name", S.NAMES)
def test_labels_and_sizes_equal_the_reference(capi, name):
    k, ref = S.case(name), S.reference(name)
    d = dev(k.d)
    labels, sizes = capi.disparity_components(d, k.max_diff)
    assert_same(name, "labels", host_bits(labels), ref["labels"])
    assert_same(name, "sizes", host_bits(sizes), ref["sizes"])
    only, none = capi.disparity_components(d, k.max_diff, want_sizes=False)       # sizes NULL: the same labels
    assert none is None and raw(only) == raw(labels)
    assert raw(d) == k.d.tobytes()                                                  # the map is only read


@pytest.mark.parametrize("name", S.NAMES)
def test_the_speckle_filter_equals_the_reference_with_and_without_a_cost_map(capi, name):
    k, ref = S.case(name), S.reference(name)
    cost = cost_map(k.d)
    want_d, want_c = R.speckles_ref(k.d, cost, k.max_diff, k.max_size)
    assert np.array_equal(R.bits(want_d), R.bits(ref["speckles"]))
    d, c = dev(k.d), dev(cost.view(np.int32))
    capi.stereo_filter_speckles(d, c, k.max_size, k.max_diff)
    assert_same(name, "disparity", host_bits(d), R.bits(want_d))
    assert_same(name, "cost", host_bits(c), want_c)
    d2 = dev(k.d)
    capi.stereo_filter_speckles(d2, None, k.max_size, k.max_diff)                   # cost NULL
    assert raw(d2) == raw(d)
    capi.stereo_filter_speckles(d, c, k.max_size, k.max_diff)                       # twice equals once
    assert_same(name, "disparity, second pass", host_bits(d), R.bits(want_d))
    assert_same(name, "cost, second pass", host_bits(c), want_c)
    d0 = dev(k.d)
    capi.stereo_filter_speckles(d0, None, 0, k.max_diff)                            # maxSpeckleSize 0 removes nothing
    assert raw(d0) == k.d.tobytes()


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", S.NAMES)
def test_the_median_equals_the_reference(capi, name, radius):
    k, ref = S.case(name), S.reference(name)
    d = dev(k.d)
    out = capi.stereo_filter_median(d, radius)
    assert_same(name, "median %d" % radius, host_bits(out), R.bits(ref["median%d" % radius]))
    assert raw(d) == k.d.tobytes() and out.data_ptr() != d.data_ptr()               # out of place


def test_a_dirty_workspace_reused_across_shapes_changes_nothing(capi):
    """one workspace, large enough for every case and filled with 0xA5 once, then left as the calls leave it"""
    big = max(int(capi.LIB.ssrlcv_hip_stereo_filter_speckles_workspace_bytes(capi.c_u32(S.case(n).d.shape[1]), capi.c_u32(S.case(n).d.shape[0])))
              for n in S.NAMES)
    ws = torch.full((big,), 0xA5, dtype=torch.uint8, device="cuda")
    for name in ("constant", "checker_holes", "serpentine", "blobs", "one_pixel", "spirals", "noisy_real", "column", "comb_bottom", "constant"):
        k, ref = S.case(name), S.reference(name)
        labels, sizes = capi.disparity_components(dev(k.d), k.max_diff, workspace=ws)
        assert_same(name, "labels", host_bits(labels), ref["labels"])
        assert_same(name, "sizes", host_bits(sizes), ref["sizes"])
        d = dev(k.d)
        capi.stereo_filter_speckles(d, None, k.max_size, k.max_diff, workspace=ws)
        assert_same(name, "disparity", host_bits(d), R.bits(ref["speckles"]))
        ws[: ws.numel() // 2].fill_(0xA5)                                           # and dirty again, in part


@pytest.mark.parametrize("name", ["constant", "serpentine", "spirals", "noisy_real", "median_mix"])
def test_two_runs_are_bit_equal(capi, name):
    k = S.case(name)

    def once():
        d = dev(k.d)
        labels, sizes = capi.disparity_components(d, k.max_diff)
        capi.stereo_filter_speckles(d, None, k.max_size, k.max_diff)
        return raw(labels), raw(sizes), raw(d), raw(capi.stereo_filter_median(dev(k.d), 2))

    assert once() == once()


def test_a_side_stream_without_host_synchronisation(capi):
    """median, speckles, components and capi.stereo_matches queued on one side stream; nothing waits on the host in between"""
    k, ref = S.case("noisy_real"), S.reference("noisy_real")
    d = dev(k.d)
    want = R.speckles_ref(ref["median1"], None, k.max_diff, k.max_size)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        med = capi.stereo_filter_median(d, 1)
        capi.stereo_filter_speckles(med, None, k.max_size, k.max_diff)
        labels, sizes = capi.disparity_components(med, k.max_diff)
        matches, n = capi.stereo_matches(med, 1, 0, 1)                              # reads its count at the end: the only wait
    side.synchronize()
    assert_same("noisy_real", "median + speckles", host_bits(med), R.bits(want))
    want_labels, want_sizes = R.components_ref(want, k.max_diff)
    assert_same("noisy_real", "labels", host_bits(labels), want_labels)
    assert_same("noisy_real", "sizes", host_bits(sizes), want_sizes)
    import stereo_ref
    assert n == int(R.valid_mask(want).sum()) and raw(matches) == stereo_ref.matches_ref(want, 1, 0, 1).tobytes()


@pytest.mark.parametrize("args", [dict(median=1, speckle_size=30, speckle_diff=1.0), dict(median=2), dict(speckle_size=30), dict(),
                                  dict(median=0, speckle_size=0), dict(median=2, speckle_size=9, speckle_diff=0.5)])
def test_pipeline_stereo_filter_equals_the_two_calls(capi, args):
    from ssrlcv_amd import pipeline
    k = S.case("noisy_real")
    cost = cost_map(k.d).view(np.int32)
    d, c = dev(k.d), dev(cost)
    out = pipeline.stereo_filter(d, c, **args)
    d2, c2 = dev(k.d), dev(cost)
    m = args.get("median", 0)
    want = capi.stereo_filter_median(d2, m) if m else d2
    if args.get("speckle_size", 0):
        capi.stereo_filter_speckles(want, c2, args["speckle_size"], args.get("speckle_diff", 1.0))
    assert raw(out) == raw(want) and raw(c) == raw(c2)
    if m:
        assert raw(d) == k.d.tobytes() and out.data_ptr() != d.data_ptr()           # the median is out of place
    else:
        assert out.data_ptr() == d.data_ptr()                                       # speckles alone run in place
    ref = R.median_ref(k.d, m) if m else k.d
    if args.get("speckle_size", 0):
        ref = R.speckles_ref(ref, None, args.get("speckle_diff", 1.0), args["speckle_size"])[0]
    assert_same("noisy_real", "stereo_filter", host_bits(out), R.bits(ref))


def noisy_args():
    case, left, right = S.noisy_pair()
    return dev(left), dev(right), dict(radius=case.r, min_disparity=case.dmin, num_disparities=case.D, lr_tolerance=-1, subpixel=bool(case.subpixel))


def test_the_gpu_map_of_the_noisy_pair_is_the_case(capi):
    """the real case is the GPU's own block-matching map too, so the filters below see what the chain gives them"""
    left, right, args = noisy_args()
    disp, cost = capi.stereo_disparity(left, right, **args)
    assert raw(disp) == S.noisy_real()[0].tobytes() and np.array_equal(host_bits(cost), S.noisy_real()[1])


def test_stereo_cloud_with_post_equals_its_steps(capi):
    from ssrlcv_amd import pipeline
    left, right, args = noisy_args()
    post = dict(median=1, speckle_size=S.REAL_MAX_SIZE, speckle_diff=S.REAL_MAX_DIFF)
    pts, matches, n, disp = pipeline.stereo_cloud(left, right, step=1, post=post, **CAMERA, **args)
    d0 = pipeline.stereo_disparity(left, right, want_cost=False, **args)[0]
    want = pipeline.stereo_filter(d0, None, **post)
    m2, n2 = capi.stereo_matches(want, 1, 0, 1)
    p2 = capi.stereo_points(m2, n2, **CAMERA)
    assert raw(disp) == raw(want) and n == n2 > 1000 and raw(matches) == raw(m2) and raw(pts) == raw(p2)
    ref = R.speckles_ref(R.median_ref(S.noisy_real()[0], 1), None, S.REAL_MAX_DIFF, S.REAL_MAX_SIZE)[0]
    assert_same("noisy_real", "stereo_cloud's map", host_bits(disp), R.bits(ref))
    # post = None is the call without the argument, and the filter took something away
    a = pipeline.stereo_cloud(left, right, step=1, post=None, **CAMERA, **args)
    b = pipeline.stereo_cloud(left, right, step=1, **CAMERA, **args)
    assert a[2] == b[2] > n and all(raw(x) == raw(y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))
    assert raw(b[3]) == S.noisy_real()[0].tobytes()
    with pytest.raises(TypeError, match="post takes"):
        pipeline.stereo_cloud(left, right, post=dict(median=1, size=3), **CAMERA, **args)


def test_stereo_cloud_cameras_with_post_equals_its_steps(capi):
    from ssrlcv_amd import pipeline
    import rectify_cases as C
    s, t = C.scene_pair(), C.truth()
    left_d, right_d = torch.from_numpy(s["left"]).cuda(), torch.from_numpy(s["right"]).cuda()
    cam_l, cam_r = s["cams"][0], s["cams"][1]
    args = dict(radius=C.CHAIN.r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=C.CHAIN.lr, subpixel=bool(C.CHAIN.subpixel))
    post = dict(median=1, speckle_size=40, speckle_diff=1.0)
    step = 2
    pts, matches, n, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, post=post, **args)
    # the steps one by one: the filters behind the mask, before the matches
    left_r, right_r, rect2 = pipeline.rectify_pair(left_d, right_d, cam_l, cam_r)
    d2 = pipeline.stereo_disparity(left_r, right_r, want_cost=False, **args)[0]
    capi.stereo_mask_rectified(d2, None, C.CHAIN.r, rect2)
    masked = d2.clone()
    d2 = pipeline.stereo_filter(d2, None, **post)
    assert rect.tobytes() == rect2.tobytes() and raw(disp) == raw(d2) != raw(masked)
    ref = R.speckles_ref(R.median_ref(masked.cpu().numpy(), 1), None, 1.0, 40)[0]
    assert_same("scene", "stereo_cloud_cameras' map", host_bits(disp), R.bits(ref))
    m2, n2 = capi.stereo_matches(d2, step, 0, 1)
    capi.matches_apply_homography(m2, n2, rect["Hl"], rect["Hr"])
    n2 = capi.compact_matches(capi.OUT_MATCH, m2, n2, capi.match_workspace(n2, 1))
    m2 = m2[: 40 * n2]
    assert n == n2 > 1000 and raw(matches) == raw(m2)
    kp_d, mm_d, _ = capi.matchset_from_matches(capi.OUT_MATCH, m2, n2)
    p2 = pipeline.triangulate(capi.to_host(mm_d, H.MULTIMATCH, n2), capi.to_host(kp_d, H.KEYPOINT, 2 * n2), s["cams"], nview=False)
    assert tuple(pts.shape) == (n, 3) and raw(pts) == raw(p2)
    a = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, post=None, **args)
    b = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, **args)
    assert a[2] == b[2] and all(raw(x) == raw(y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and raw(b[3]) == raw(masked)


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory::medianFilter + filterSpeckles (tests/cpp/speckle_test.cpp) write what the Python path gives, from maps in
    host memory and with and without a cost map; the checksums it prints are those of the Python path's bytes"""
    case, left, right = S.noisy_pair()
    lraw, rraw, prefix = str(tmp_path / "left.raw"), str(tmp_path / "right.raw"), str(tmp_path / "out")
    left.tofile(lraw)
    right.tofile(rraw)
    host = os.path.join(ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/speckle_test"])
    a = [os.path.join(host, "_build", "speckle_test"), lraw, rraw, str(case.w), str(case.h), str(case.r), str(case.dmin), str(case.D), "1",
         str(S.REAL_MAX_SIZE), repr(S.REAL_MAX_DIFF), prefix]
    out = subprocess.check_output(a, timeout=120).decode().splitlines()
    assert out[-1] == "ok", out
    sums = dict(line.split() for line in out[:-1])

    def fnv(data):
        h = 1469598103934665603
        for byte in data:
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h

    disp, cost = capi.stereo_disparity(dev(left), dev(right), case.r, case.dmin, case.D, capi.STEREO_NO_LIMIT, -1, bool(case.subpixel))
    med = capi.stereo_filter_median(disp, 1)
    want = {"disparity": raw(disp), "median": raw(med)}
    capi.stereo_filter_speckles(med, cost, S.REAL_MAX_SIZE, S.REAL_MAX_DIFF)
    want["speckle.disparity"], want["speckle.cost"] = raw(med), raw(cost)
    capi.stereo_filter_speckles(disp, None, S.REAL_MAX_SIZE, S.REAL_MAX_DIFF)
    want["speckle.only"] = raw(disp)
    assert want["speckle.only"] != want["disparity"] and want["speckle.disparity"] != want["median"] != want["disparity"]
    for what, data in want.items():
        assert np.fromfile(prefix + "." + what, np.uint8).tobytes() == data, what
        assert sums[what] == fnv(data), what
    assert_same("noisy_real", "speckle.only", np.frombuffer(want["speckle.only"], np.uint32).reshape(case.h, case.w),
                R.bits(S.reference("noisy_real")["speckles"]))
