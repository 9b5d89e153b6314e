"""Dense stereo, the part that needs no GPU: the header and the loader name the entry points, the parameter struct is 24
bytes, every refusal is decided on the host before a buffer is looked at (the device pointers here are bogus or null), the
workspace queries are 0 for refused parameters and grow with the image, the Window_NxN host types have their sizes and their
SAD distProtocol, and the C++ mirror program compiles."""
import ctypes
import os
import re
import subprocess

import pytest

import helpers as H

u32, i32, f32, csz, vp, cint = ctypes.c_uint32, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
NAMES = ["ssrlcv_hip_stereo_workspace_bytes", "ssrlcv_hip_stereo_sad_u8", "ssrlcv_hip_stereo_matches_workspace_bytes",
         "ssrlcv_hip_stereo_matches", "ssrlcv_hip_stereo_points"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference


class Params(ctypes.Structure):
    _fields_ = [("radius", u32), ("minDisparity", i32), ("numDisparities", u32), ("maxCost", u32), ("lrTolerance", i32),
                ("subpixel", u32)]


def params(radius=4, dmin=0, D=64, max_cost=0xFFFFFFFF, lr=1, subpixel=1):
    return Params(radius, dmin, D, max_cost, lr, subpixel)


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    lb.ssrlcv_hip_stereo_workspace_bytes.restype = csz
    lb.ssrlcv_hip_stereo_matches_workspace_bytes.restype = csz
    return lb


def need(lib, w, h, p):
    return lib.ssrlcv_hip_stereo_workspace_bytes(u32(w), u32(h), ctypes.byref(p) if p is not None else None)


def sad(lib, p, w=64, h=48, left=BOGUS, right=BOGUS, ws=BOGUS, ws_bytes=1 << 40, disp=BOGUS, cost=BOGUS):
    return lib.ssrlcv_hip_stereo_sad_u8(vp(left), vp(right), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(ws),
                                        csz(ws_bytes), vp(disp), vp(cost), vp(None))


def matches(lib, w=64, h=48, step=1, disp=BOGUS, out=BOGUS, cap=4, count=BOGUS, ws=BOGUS, ws_bytes=1 << 40):
    return lib.ssrlcv_hip_stereo_matches(vp(disp), u32(w), u32(h), u32(step), cint(0), cint(1), vp(out), u32(cap), vp(count), vp(ws),
                                         csz(ws_bytes), vp(None))


def points(lib, foc, n=4, m=BOGUS, out=BOGUS):
    return lib.ssrlcv_hip_stereo_points(vp(m), u32(n), f32(foc), f32(0.1), f32(0.0), f32(32.0), f32(24.0), vp(out), vp(None))


def test_header_and_loader_name_the_entry_points():
    from ssrlcv_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
    assert "ssrlcv_stereo_params" in header
    assert ctypes.sizeof(Params) == 24
    from ssrlcv_amd import capi
    assert ctypes.sizeof(capi.StereoParams) == 24
    assert [f[0] for f in capi.StereoParams._fields_] == [f[0] for f in Params._fields_]
    for item in ("uniqueness ratio", "unrectified", "colour", "census", "NCC", "semi-global"):
        assert item in header, item  # what the contract leaves out is stated


@pytest.mark.parametrize("kw", [dict(radius=0), dict(D=0), dict(dmin=-32769), dict(dmin=32768), dict(subpixel=2), dict(subpixel=0xFFFFFFFF)])
def test_invalid_parameters(lib, kw):
    p = params(**kw)
    assert sad(lib, p) == INVALID_ARG          # bogus device pointers: the parameters are judged first, nothing is launched
    assert need(lib, 64, 48, p) == 0


def test_null_params_and_too_many_pixels(lib):
    assert sad(lib, None) == INVALID_ARG and need(lib, 64, 48, None) == 0
    assert sad(lib, params(), w=65536, h=32768) == INVALID_ARG and need(lib, 65536, 32768, params()) == 0   # w h = 2^31
    assert need(lib, 65536, 32767, params()) > 0                                                            # just below


@pytest.mark.parametrize("kw", [dict(radius=16), dict(D=257), dict(radius=1000, D=100000)])
def test_unsupported_parameters(lib, kw):
    p = params(**kw)
    assert sad(lib, p) == UNSUPPORTED
    assert need(lib, 64, 48, p) == 0


def test_invalid_comes_before_unsupported(lib):
    assert sad(lib, params(radius=16, subpixel=2)) == INVALID_ARG
    assert sad(lib, params(radius=0, D=257)) == INVALID_ARG
    assert sad(lib, params(radius=16), w=65536, h=32768) == INVALID_ARG


def test_the_edges_of_the_parameter_ranges_are_taken(lib):
    for kw in (dict(radius=1), dict(radius=15), dict(D=1), dict(D=256), dict(dmin=-32768), dict(dmin=32767), dict(subpixel=0),
               dict(lr=-1), dict(lr=-2147483648), dict(lr=2147483647), dict(max_cost=0)):
        p = params(**kw)
        assert need(lib, 64, 48, p) > 0, kw
        assert sad(lib, p, ws_bytes=0) == WORKSPACE, kw   # past the parameter and buffer checks, stopped by the size check


def test_null_buffers_then_short_workspace(lib):
    p = params()
    for kw in (dict(left=None), dict(right=None), dict(ws=None), dict(disp=None)):
        assert sad(lib, p, **kw) == INVALID_ARG, kw
        assert sad(lib, p, ws_bytes=0, **kw) == INVALID_ARG, kw     # a NULL buffer is reported before a short workspace
    n = need(lib, 64, 48, p)
    assert sad(lib, p, ws_bytes=n - 1) == WORKSPACE
    assert sad(lib, p, ws_bytes=n - 1, cost=None) == WORKSPACE      # cost may be NULL: not an argument error
    assert sad(lib, params(radius=16), left=None) == UNSUPPORTED    # the parameters before the buffers


def test_workspace_query_grows_with_the_image(lib):
    last = 0
    for w, h in [(1, 1), (8, 30), (64, 48), (97, 83), (131, 70), (1024, 1024), (4096, 4096)]:
        n = need(lib, w, h, params())
        assert n >= last and n >= 2 * w * h, (w, h, n)
        assert n <= 2 * w * h + 4096
        last = n
    assert need(lib, 4096, 4096, params()) > need(lib, 1024, 1024, params()) > need(lib, 64, 48, params())
    assert need(lib, 0, 48, params()) >= 0  # an empty image is no error


def test_matches_refusals(lib):
    assert matches(lib, step=0) == INVALID_ARG
    assert lib.ssrlcv_hip_stereo_matches_workspace_bytes(u32(64), u32(48), u32(0)) == 0
    assert matches(lib, w=65536, h=32768) == INVALID_ARG
    assert lib.ssrlcv_hip_stereo_matches_workspace_bytes(u32(65536), u32(32768), u32(1)) == 0
    for kw in (dict(disp=None), dict(count=None), dict(ws=None), dict(out=None, cap=4)):
        assert matches(lib, **kw) == INVALID_ARG, kw
    assert matches(lib, step=0, disp=None) == INVALID_ARG
    n = lib.ssrlcv_hip_stereo_matches_workspace_bytes(u32(64), u32(48), u32(1))
    assert n > 0
    assert matches(lib, ws_bytes=n - 1) == WORKSPACE
    assert matches(lib, out=None, cap=0, ws_bytes=n - 1) == WORKSPACE   # out may be NULL with capacity 0
    sizes = [lib.ssrlcv_hip_stereo_matches_workspace_bytes(u32(w), u32(h), u32(s)) for w, h, s in
             [(64, 48, 3), (64, 48, 1), (1024, 1024, 1), (4096, 4096, 1)]]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # The query counts the samples ceil(w / step) x ceil(h / step), so it shrinks with the step and never reaches 0 for a
    # step >= 1.  (It is rounded to 256 bytes and cannot tell 0 samples from a few: that a step near 2^32 still leaves the
    # sample at pixel (0, 0) is held on the GPU, tests/test_gpu_stereo.py test_sampling_grid_of_any_step_on_a_hand_made_map.)
    q = lib.ssrlcv_hip_stereo_matches_workspace_bytes
    wide = [q(u32(1 << 24), u32(1), u32(s)) for s in (1, 16, 1 << 10, 1 << 24, 0x7FFFFFFF, 0xFF000001, 0xFFFFFFFF)]
    assert wide == sorted(wide, reverse=True) and wide[0] > wide[1] > wide[2] and wide[-1] == q(u32(1), u32(1), u32(1)) > 0


@pytest.mark.parametrize("foc", [0.0, -0.0, float("nan"), float("inf"), float("-inf")])
def test_points_refuse_a_useless_focal_length(lib, foc):
    assert points(lib, foc) == INVALID_ARG
    assert points(lib, foc, n=0, m=None, out=None) == INVALID_ARG   # the parameter first


def test_points_buffers(lib):
    assert points(lib, 500.0, m=None) == INVALID_ARG and points(lib, 500.0, out=None) == INVALID_ARG
    assert points(lib, 500.0, n=0, m=None, out=None) == OK          # nothing to do


def test_window_types_and_the_mirror_program():
    """host/Feature.hpp Window_NxN: N x N bytes, SAD distProtocol with early exit; tests/cpp/stereo_test.cpp compiles (it
    includes ssrlcv.hpp, so DisparityFactory.hpp and PointCloudFactory::stereo_disparity compile too)"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/stereo_test"])
    out = subprocess.check_output([os.path.join(host, "_build", "stereo_test"), "--windows"], timeout=60).decode().splitlines()
    assert out[-1] == "ok", out
    # a = 3x + y; b = a with the four corners raised by 10 and the centre lowered by 7 (by 4 in the 3 x 3 window, whose centre is 4)
    want = {3: 44.0, 9: 47.0, 15: 47.0, 25: 47.0, 31: 47.0}
    for line, n in zip(out, (3, 9, 15, 25, 31)):
        assert line == "window %d size %d dist %.1f %.1f self 0.0 early 20.0" % (n, n * n, want[n], want[n]), line
    feature = open(os.path.join(host, "Feature.hpp")).read()
    for n in (3, 9, 15, 25, 31):
        assert "Window_%dx%d" % (n, n) in feature
    umbrella = open(os.path.join(host, "ssrlcv.hpp")).read()
    assert '#include "DisparityFactory.hpp"' in umbrella
    pcf = open(os.path.join(host, "PointCloudFactory.hpp")).read()
    assert "stereo_disparity(ptr::value<Unity<Match>> matches, float foc, float baseline, float doffset)" in pcf
    assert "stereo disparity, plane fitting" not in pcf
    assert "disparity matchers and match-file" not in open(os.path.join(host, "MatchFactory.hpp")).read()


def test_design_no_longer_lists_stereo_as_out_of_scope():
    design = open(os.path.join(H.ROOT, "DESIGN.md")).read()
    section7 = design[design.index("## 7. Out of scope"):]
    section7 = section7[:section7.index("\n## ", 5)] if "\n## " in section7[5:] else section7
    for item in ("Window_* descriptors", "disparity matchers", "stereo disparity"):
        assert item not in section7, item
