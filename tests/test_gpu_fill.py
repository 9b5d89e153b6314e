"""Hole filling on the GPU (ssrlcv_hip_stereo_fill_holes; include/ssrlcv_hip.h "hole filling") against the numpy restatement of
the contract (tests/fill_ref.py) on the cases of tests/fill_cases.py (tests/test_fill_cases.py proves without a GPU that they
test something).  Every comparison is exact: disparities as bit patterns, the mask byte for byte."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fill_cases as C
import fill_ref as R
import fill_scene as S
import helpers as H

pytestmark = pytest.mark.gpu

NAMES = sorted(C.CASES)
RULES = {R.MIN: "min", R.MEDIAN: "median"}


def raw(t):
    return t.cpu().numpy().tobytes()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases and references are read-only


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_same(name, what, got, want):
    ne = got != want
    assert not ne.any(), (name, "%s differs at %d of %d pixels, first (y, x) %s: got %s want %s" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4]))


def check_case(capi, name, **kw):
    k = C.CASES[name]
    want, want_mask = C.reference(name)
    d = dev(k.d)
    out, mask = capi.stereo_fill_holes(d, k.paths, k.max_gap, k.min_hits, k.rule, want_mask=True, **kw)
    assert_same(name, "out", host_bits(out), R.bits_of(want))
    assert_same(name, "filled", mask.cpu().numpy(), want_mask)
    return d, out


@pytest.mark.parametrize("name", NAMES)
def test_every_case_equals_the_reference(capi, name):
    k = C.CASES[name]
    d, out = check_case(capi, name)
    only, none = capi.stereo_fill_holes(d, k.paths, k.max_gap, k.min_hits, k.rule)            # filled NULL: the same map
    assert none is None and raw(only) == raw(out)
    assert raw(d) == k.d.tobytes() and out.data_ptr() != d.data_ptr()                          # out of place: `in` is only read
    assert raw(capi.stereo_fill_holes(d, k.paths, k.max_gap, k.min_hits, k.rule)[0]) == raw(out)   # bit-equal run to run


def test_a_dirty_workspace_reused_across_shapes_and_path_masks_changes_nothing(capi):
    """one workspace, large enough for every case and filled with the invalid pattern's neighbours once, then left as the calls
    leave it: a hit map entry the call reads it has written before"""
    big = 8 * max((4 * k.d.size + 255) // 256 * 256 for k in C.CASES.values())
    ws = torch.full((big,), 0xA5, dtype=torch.uint8, device="cuda")
    for name in ("shape_97x83", "dir_5", "paths_03", "shape_83x97", "gap_0", "paths_f0", "checkerboard", "shape_1x1", "dir_0", "frame",
                 "paths_0f", "strips_33x290", "shape_257x5", "strips_20x290", "half_hole", "shape_97x83"):
        check_case(capi, name, workspace=ws)
    ws.view(torch.int32)[: big // 8].fill_(0x40400000)                                          # 3.0f, a plausible hit, in the first maps
    for name in ("gap_7", "all_holes", "star_gap7", "dir_6"):
        check_case(capi, name, workspace=ws)


def test_a_side_stream_without_host_synchronisation(capi):
    name = "shape_97x83"
    k = C.CASES[name]
    d = dev(k.d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first, _ = capi.stereo_fill_holes(d, k.paths, k.max_gap, k.min_hits, k.rule)
        second, mask2 = capi.stereo_fill_holes(first, k.paths, k.max_gap, k.min_hits, k.rule, want_mask=True)   # not idempotent: fills on
    side.synchronize()
    assert_same(name, "out", host_bits(first), R.bits_of(C.reference(name)[0]))
    want2, want_mask2 = R.fill(C.reference(name)[0], k.paths, k.max_gap, k.min_hits, k.rule)
    assert_same(name, "second pass", host_bits(second), R.bits_of(want2))
    assert_same(name, "second mask", mask2.cpu().numpy(), want_mask2)


@pytest.mark.parametrize("name", ["paths_ff_5", "paths_0f", "gap_unlimited", "dir_4"])
def test_pipeline_stereo_fill_equals_the_c_abi_call(capi, name):
    from ssrlcv_amd import pipeline
    k = C.CASES[name]
    d = dev(k.d)
    want, want_mask = capi.stereo_fill_holes(d, k.paths, k.max_gap, k.min_hits, k.rule, want_mask=True)
    args = dict(paths=k.paths, max_gap=k.max_gap, min_hits=k.min_hits, rule=RULES[k.rule])
    out = pipeline.stereo_fill(d, **args)
    assert isinstance(out, torch.Tensor) and raw(out) == raw(want)
    out, mask = pipeline.stereo_fill(d, want_mask=True, **args)
    assert raw(out) == raw(want) and raw(mask) == raw(want_mask) and mask.dtype == torch.uint8
    assert raw(pipeline._post_filter(d, dict(fill=args))) == raw(want)
    assert_same(name, "pipeline.stereo_fill", host_bits(out), R.bits_of(C.reference(name)[0]))
    if name == "paths_ff_5":   # the defaults are paths 0xFF, max_gap 32 (no limit on a map this small), min_hits 5, "min"
        assert raw(pipeline.stereo_fill(d)) == raw(capi.stereo_fill_holes(d, 0xFF, 32, 5, capi.FILL_MIN)[0])
    with pytest.raises(ValueError):
        pipeline.stereo_fill(d, rule="mean")


def test_stereo_cloud_with_fill_equals_the_references_and_gains_the_filled_points(capi):
    from ssrlcv_amd import pipeline
    import stereo_ref
    left, right = S.pair()
    left_d, right_d = dev(left), dev(right)
    fill = dict(paths=0x03, max_gap=32, min_hits=2, rule="min")
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, step=1, post=dict(fill=fill), **S.CAMERA, **S.ARGS)
    base = pipeline.stereo_cloud(left_d, right_d, step=1, **S.CAMERA, **S.ARGS)
    assert_same("scene", "the unfilled map", host_bits(base[3]), R.bits_of(S.reference_disparity()))
    want, filled = R.fill(S.reference_disparity(), 0x03, 32, 2, R.MIN)
    assert_same("scene", "stereo_cloud's map", host_bits(disp), R.bits_of(want))
    assert filled.sum() > 100 and n == base[2] + int(filled.sum())                              # exactly the filled holes more, at step 1
    want_matches = stereo_ref.matches_ref(want, 1, 0, 1)
    assert raw(matches) == want_matches.tobytes()
    assert raw(pts) == raw(capi.stereo_points(matches, n, **S.CAMERA))
    # the same through the C-ABI call on the GPU's own map, and with the other filters in front
    by_hand, mask = capi.stereo_fill_holes(base[3], 0x03, 32, 2, capi.FILL_MIN, want_mask=True)
    assert raw(by_hand) == raw(disp) and int(mask.sum().item()) == int(filled.sum())
    post = dict(median=1, speckle_size=20, speckle_diff=1.0, fill=fill)
    chained = pipeline.stereo_cloud(left_d, right_d, step=1, post=post, **S.CAMERA, **S.ARGS)[3]
    steps = pipeline.stereo_fill(pipeline.stereo_filter(base[3].clone(), None, median=1, speckle_size=20, speckle_diff=1.0), **fill)
    assert raw(chained) == raw(steps)                                                           # the fill runs last
    with pytest.raises(TypeError, match="post takes"):
        pipeline.stereo_cloud(left_d, right_d, post=dict(fill=dict(size=3)), **S.CAMERA, **S.ARGS)


def test_stereo_cloud_cameras_with_fill_masks_once_more(capi):
    from ssrlcv_amd import pipeline
    import rectify_cases as RC
    import speckle_ref
    s, t = RC.scene_pair(), RC.truth()
    left_d, right_d = torch.from_numpy(s["left"]).cuda(), torch.from_numpy(s["right"]).cuda()
    cam_l, cam_r = s["cams"][0], s["cams"][1]
    args = dict(radius=RC.CHAIN.r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=RC.CHAIN.lr, subpixel=bool(RC.CHAIN.subpixel))
    fill = dict(paths=0xFF, max_gap=16, min_hits=3, rule="median")
    post = dict(median=1, speckle_size=40, speckle_diff=1.0, fill=fill)
    step = 2
    pts, matches, n, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, post=post, **args)
    # by hand: mask -> filters -> fill -> mask
    left_r, right_r, rect2 = pipeline.rectify_pair(left_d, right_d, cam_l, cam_r)
    d2 = pipeline.stereo_disparity(left_r, right_r, want_cost=False, **args)[0]
    capi.stereo_mask_rectified(d2, None, RC.CHAIN.r, rect2)
    masked = d2.clone()
    filtered = pipeline.stereo_filter(d2, None, median=1, speckle_size=40, speckle_diff=1.0)
    filled = pipeline.stereo_fill(filtered, **fill)
    unmasked = filled.clone()
    capi.stereo_mask_rectified(filled, None, RC.CHAIN.r, rect2)
    assert rect.tobytes() == rect2.tobytes() and raw(disp) == raw(filled)
    ref = speckle_ref.speckles_ref(speckle_ref.median_ref(masked.cpu().numpy(), 1), None, 1.0, 40)[0]
    ref_filled = R.fill(ref, 0xFF, 16, 3, R.MEDIAN)[0]
    assert_same("scene", "the map before the last mask", host_bits(unmasked), R.bits_of(ref_filled))
    # the last mask removes what the fill extrapolated, never adds, and leaves nothing it would remove
    valid, before, first = host_bits(disp) != R.INVALID, host_bits(unmasked) != R.INVALID, host_bits(masked) != R.INVALID
    assert not (valid & ~before).any() and (before & ~valid).any() and (valid & ~first).any()
    assert np.array_equal(host_bits(disp)[valid], host_bits(unmasked)[valid])
    again = disp.clone()
    capi.stereo_mask_rectified(again, None, RC.CHAIN.r, rect2)
    assert raw(again) == raw(disp)                                       # no returned pixel lies where the mask would have removed it
    m2, n2 = capi.stereo_matches(filled, step, 0, 1)
    capi.matches_apply_homography(m2, n2, rect["Hl"], rect["Hr"])
    n2 = capi.compact_matches(capi.OUT_MATCH, m2, n2, capi.match_workspace(n2, 1))
    assert n == n2 > 1000 and raw(matches) == raw(m2[: 40 * n2]) and tuple(pts.shape) == (n, 3)
    plain = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, post=dict(median=1, speckle_size=40, speckle_diff=1.0), **args)
    assert raw(plain[3]) == raw(filtered) and n > plain[2]                # without fill nothing changed, and the fill added points


def test_class_api_program_equals_the_python_path(capi, tmp_path):
    """DisparityFactory::fillHoles (tests/cpp/fill_test.cpp) writes what the Python path gives, from a map in host memory, with and
    without the mask; the checksums it prints are those of the Python path's bytes"""
    name = "shape_97x83"
    k = C.CASES[name]
    h, w = k.d.shape
    src, prefix = str(tmp_path / "map.f32"), str(tmp_path / "out")
    k.d.tofile(src)
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/fill_test"])
    a = [os.path.join(host, "_build", "fill_test"), src, str(w), str(h), hex(k.paths), str(k.max_gap), str(k.min_hits), str(k.rule), prefix]
    out = subprocess.check_output(a, timeout=120).decode().splitlines()
    assert out[-1] == "ok", out
    sums = dict(line.split() for line in out[:-1])

    def fnv(data):
        x = 1469598103934665603
        for byte in data:
            x = ((x ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % x

    want, want_mask = C.reference(name)
    for what, data in (("filled", want.tobytes()), ("mask", want_mask.tobytes())):
        assert np.fromfile(prefix + "." + what, np.uint8).tobytes() == data, what
        assert sums[what] == fnv(data), what
