"""Rectification, the part that needs no GPU: the header and the loader name the entry points, every refusal of the three device
entry points is decided on the host before a buffer is looked at (the device pointers here are bogus or null), and the host
builder ssrlcv_rectify_cameras_host: its refusals in their order, `out` untouched on error, a parallel pair, and the geometry
of what it builds for tools/scene.py's PinholeRig."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import rectify_cases as C

sys.path.insert(0, os.path.join(H.ROOT, "tools"))

u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
NAMES = ["ssrlcv_rectify_cameras_host", "ssrlcv_hip_warp_homography_u8", "ssrlcv_hip_stereo_mask_rectified",
         "ssrlcv_hip_matches_apply_homography"]
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference
EYE = (f32 * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    return _lib.load()


def warp(lib, Hm=EYE, src=BOGUS, sw=64, sh=48, dst=BOGUS, dw=64, dh=48):
    return lib.ssrlcv_hip_warp_homography_u8(vp(src), u32(sw), u32(sh), Hm, vp(dst), u32(dw), u32(dh), vp(None))


def mask(lib, disp=BOGUS, cost=BOGUS, w=64, h=48, r=4, Hl=EYE, Hr=EYE, sw=64, sh=48):
    return lib.ssrlcv_hip_stereo_mask_rectified(vp(disp), vp(cost), u32(w), u32(h), u32(r), Hl, Hr, u32(sw), u32(sh), vp(None))


def apply(lib, m=BOGUS, n=4, H0=EYE, H1=EYE):
    return lib.ssrlcv_hip_matches_apply_homography(vp(m), u32(n), H0, H1, vp(None))


def test_header_and_loader_name_the_entry_points():
    from ssrlcv_amd import _lib, capi
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4   # additions keep the number
    assert "ssrlcv_rectification" in header and capi.RECTIFICATION.itemsize == 184
    stereo = header[header.index("---- dense stereo"):header.index("---- rectification")]
    out_of_scope = stereo[stereo.index("Out of scope:"):]
    assert "unrectified pairs" not in out_of_scope.split(".")[0]
    block = header[header.index("---- rectification"):]
    for item in ("fundamental matrix", "ushbroom", "distortion", "other than bilinear", "colour", "convex", "never rescues"):
        assert item in block, item   # what the contract leaves out, and the two explanations it owes, are stated


# ---- the device entry points' refusals
def test_warp_refusals(lib):
    assert warp(lib, Hm=None) == INVALID_ARG
    assert warp(lib, sw=0) == INVALID_ARG and warp(lib, sh=0) == INVALID_ARG
    for kw in (dict(sw=(1 << 24) + 1, sh=1), dict(sh=(1 << 24) + 1, sw=1), dict(dw=(1 << 24) + 1, dh=1), dict(dh=(1 << 24) + 1, dw=1)):
        assert warp(lib, **kw) == INVALID_ARG, kw
    assert warp(lib, sw=65536, sh=32768) == INVALID_ARG and warp(lib, dw=65536, dh=32768) == INVALID_ARG   # w h = 2^31
    # the parameters before the buffers
    assert warp(lib, Hm=None, src=None, dst=None) == INVALID_ARG
    assert warp(lib, src=None) == INVALID_ARG and warp(lib, dst=None) == INVALID_ARG
    # a dst of 0 pixels is nothing to do -- once the parameters are sound
    assert warp(lib, dw=0) == OK and warp(lib, dh=0) == OK and warp(lib, dw=0, dst=None) == OK
    assert warp(lib, dw=0, sw=0) == INVALID_ARG and warp(lib, dw=0, Hm=None) == INVALID_ARG


def test_mask_refusals(lib):
    assert mask(lib, Hl=None) == INVALID_ARG and mask(lib, Hr=None) == INVALID_ARG
    assert mask(lib, sw=0) == INVALID_ARG and mask(lib, sh=0) == INVALID_ARG
    assert mask(lib, w=(1 << 24) + 1, h=1) == INVALID_ARG and mask(lib, sh=(1 << 24) + 1, sw=1) == INVALID_ARG
    assert mask(lib, w=65536, h=32768) == INVALID_ARG and mask(lib, sw=65536, sh=32768) == INVALID_ARG
    for r in (0, 16, 0xFFFFFFFF):
        assert mask(lib, r=r) == INVALID_ARG, r
        assert mask(lib, r=r, disp=None) == INVALID_ARG
    assert mask(lib, disp=None) == INVALID_ARG                # then the buffer
    assert mask(lib, w=0) == OK and mask(lib, h=0, disp=None) == OK
    assert mask(lib, w=0, r=0) == INVALID_ARG


def test_apply_refusals(lib):
    assert apply(lib, m=None) == INVALID_ARG
    assert apply(lib, m=None, n=0) == OK and apply(lib, n=0) == OK
    assert apply(lib, H0=None, H1=None) == OK                 # neither side moves: nothing is launched


# ---- the host builder
def camera(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0), size=(64, 48), foc=0.05, fov=0.2):
    c = np.zeros(1, H.CAMERA)
    c["cam_pos"], c["cam_rot"], c["size"], c["foc"], c["fov"] = pos, rot, size, foc, (fov, fov)
    c["dpix"] = (123.0, 456.0)   # ignored
    return c


def build(lib, left, right, out=None):
    out = np.zeros(1, _rect_dtype()) if out is None else out
    rc = lib.ssrlcv_rectify_cameras_host(H.P(left) if left is not None else None, H.P(right) if right is not None else None,
                                         H.P(out) if out is not None else None)
    return rc, out


def _rect_dtype():
    from ssrlcv_amd import capi
    return capi.RECTIFICATION


def test_a_parallel_pair_is_left_alone(lib):
    rc, out = build(lib, camera(), camera(pos=(0.5, 0.0, 0.0)))
    assert rc == OK
    r = out[0]
    eye = np.array(EYE[:], np.float32)
    for k in ("Hl", "Hr", "Gl", "Gr"):
        assert np.array_equal(r[k], eye), (k, r[k])
    assert r["doffset"] == 0.0 and r["cx"] == 32.0 and r["cy"] == 24.0 and (r["w"], r["h"]) == (64, 48)
    assert r["baseline"] == 0.5 and abs(r["foc"] - 32.0 / math.tan(0.1)) < 1e-4 and not r["cam_rot"].any()


def test_builder_refusals_in_their_order(lib):
    good_l, good_r = camera(), camera(pos=(0.5, 0.0, 0.0))
    none = lib.ssrlcv_rectify_cameras_host
    assert none(None, H.P(good_r), H.P(np.zeros(1, _rect_dtype()))) == INVALID_ARG
    assert none(H.P(good_l), None, H.P(np.zeros(1, _rect_dtype()))) == INVALID_ARG
    assert none(H.P(good_l), H.P(good_r), None) == INVALID_ARG
    bad_size = [camera(size=(64, 48)), camera(pos=(0.5, 0, 0), size=(64, 49))]
    zero_size = [camera(size=(0, 48)), camera(pos=(0.5, 0, 0), size=(0, 48))]
    steep = dict(l=(0.0, math.radians(50), 0.0), r=(0.0, -math.radians(50), 0.0))   # either axis 50 degrees off the rectified one
    cases = [
        (bad_size[0], bad_size[1], INVALID_ARG),
        (zero_size[0], zero_size[1], INVALID_ARG),
        (camera(size=(64, 0)), camera(pos=(0.5, 0, 0), size=(64, 0)), INVALID_ARG),
        (camera(foc=0.0), good_r, INVALID_ARG), (good_l, camera(pos=(0.5, 0, 0), foc=-1.0), INVALID_ARG),
        (camera(foc=float("nan")), good_r, INVALID_ARG), (camera(foc=float("inf")), good_r, INVALID_ARG),
        (camera(fov=0.0), good_r, INVALID_ARG), (good_l, camera(pos=(0.5, 0, 0), fov=float("nan")), INVALID_ARG),
        (camera(fov=float("inf")), good_r, INVALID_ARG), (camera(fov=-0.2), good_r, INVALID_ARG),
        (good_l, camera(), INVALID_ARG),                                                      # |b| = 0
        (good_r, good_l, INVALID_ARG),                                                        # the wrong way round
        (camera(), camera(pos=(0.0, 0.0, 0.5)), INVALID_ARG),                                 # the baseline along the view axis
        # in order: a size mismatch before a bad focal length, that before |b| = 0, every INVALID_ARG before an UNSUPPORTED
        (camera(size=(64, 49), foc=0.0), camera(size=(64, 48)), INVALID_ARG),
        (camera(foc=0.0), camera(), INVALID_ARG),
        (camera(pos=(0.5, 0, 0), rot=steep["l"]), camera(rot=steep["r"]), INVALID_ARG),       # swapped and too steep
        (camera(rot=steep["l"]), camera(pos=(0.5, 0, 0), rot=steep["r"]), UNSUPPORTED),       # a.z = cos 50 < cos 45
        # z_l + z_r along the baseline: z_l = (cos a, 0, sin a), z_r = (cos a, 0, -sin a), a = 0.3
        (camera(rot=(0.0, math.pi / 2 - 0.3, 0.0)), camera(pos=(0.5, 0, 0), rot=(0.0, math.pi / 2 + 0.3, 0.0)), UNSUPPORTED),
    ]
    for left, right, want in cases:
        out = np.zeros(1, _rect_dtype())
        raw = out.view(np.uint8)
        raw[:] = 0xA5
        rc, _ = build(lib, left, right, out)
        assert rc == want, (left, right, rc, want)
        assert (raw == 0xA5).all()   # `out` is untouched on any error
    # a converging pair inside the limit is taken
    rc, out = build(lib, camera(rot=(0.0, math.radians(40), 0.0)), camera(pos=(0.5, 0, 0), rot=(0.0, -math.radians(40), 0.0)))
    assert rc == OK and out[0]["doffset"] > 0


RIG_SIZE = 192


@pytest.fixture(scope="module")
def rig():
    import scene
    return scene.PinholeRig(3, RIG_SIZE)


def test_the_restatement_s_parameters_for_views_0_and_2(lib, rig):
    rc, out = build(lib, rig.cameras[0:1].copy(), rig.cameras[2:3].copy())
    assert rc == OK
    r = out[0]
    assert (r["doffset"], r["cx"], r["cy"]) == (798.0, 135.0, 96.0)
    assert abs(r["foc"] - 4582.99) < 0.01 and (r["w"], r["h"]) == (RIG_SIZE, RIG_SIZE)
    from ssrlcv_amd import capi
    assert capi.rectify_cameras(rig.cameras[0], rig.cameras[2]).tobytes() == r.tobytes()   # the binder returns the same record


@pytest.mark.parametrize("views", [(0, 2), (1, 2)])
def test_the_built_pair_is_rectified(lib, rig, views):
    """Random 3-D points in front of both cameras, projected in float64 through each camera and mapped through Gl, Gr (their
    float32 entries evaluated in float64), lie on one row, and their disparity is foc baseline / Z - doffset.

    The bound, 2^-20 (2 w + 2 h) px: the nine entries of a homography are rounded to float32, a relative error of 2^-24 each,
    which moves a mapped coordinate of size up to about w by at most about 2^-24 4 w (the numerator's three terms and the
    denominator, each one rounding on a value of size w).  Two images are compared, and each G is the rounded inverse of a
    rounded H, so four such mappings meet in one difference: 2^-24 16 w = 2^-20 w for a column and 2^-20 h for a row, pooled and
    doubled (foc, baseline and doffset are float32 too) into the one bound 2^-20 (2 w + 2 h) = 7.3e-4 px at w = h = 192.
    A float64 restatement of the contract measured 4e-5 ... 6e-5 px for the rows and 3e-5 px for the disparities, so the bound
    leaves a factor of about 30 and still catches an error of a thousandth of a pixel."""
    a, b = views
    cams = rig.cameras
    rc, out = build(lib, cams[a:a + 1].copy(), cams[b:b + 1].copy())
    assert rc == OK
    r = out[0]
    w = h = RIG_SIZE
    bound = 2.0 ** -20 * (2 * w + 2 * h)
    rng = np.random.RandomState(5)
    # points around the patch centre: +-10 km across, +-2 km of height
    pts = rig.centre + rng.uniform(-10, 10, (4000, 1)) * rig.e1 + rng.uniform(-10, 10, (4000, 1)) * rig.e2 + rng.uniform(-2, 2, (4000, 1)) * rig.down
    ul, vl, zl = C.project(cams[a], rig.M[a], pts)
    ur, vr, zr = C.project(cams[b], rig.M[b], pts)
    assert (zl > 0).all() and (zr > 0).all()
    xl, yl = C.eval64(r["Gl"], ul, vl)
    xr, yr = C.eval64(r["Gr"], ur, vr)
    import scene
    Rn = scene._euler_matrix(r["cam_rot"])
    Z = ((pts - cams[a]["cam_pos"].astype(np.float64)) @ Rn)[:, 2]
    rows = np.abs(yl - yr).max()
    cols = np.abs((xl - xr) - (float(r["foc"]) * float(r["baseline"]) / Z - float(r["doffset"]))).max()
    print("views %s: rows agree to %.2e px, disparities to %.2e px, bound %.2e" % (views, rows, cols, bound))
    assert rows < bound and cols < bound
    # the principal point: a point on the rectified axis through the left camera lands on (cx, cy)
    axis = cams[a]["cam_pos"].astype(np.float64) + 400.0 * Rn[:, 2]
    u0, v0, _ = C.project(cams[a], rig.M[a], axis[None])
    x0, y0 = C.eval64(r["Gl"], u0, v0)
    assert abs(x0[0] - r["cx"]) < bound and abs(y0[0] - r["cy"]) < bound
    # H G is the identity to the same bound, on a grid over the image and a margin around it
    gy, gx = [g.ravel() for g in np.mgrid[-32:h + 32:7.5, -32:w + 32:7.5]]
    for Hm, Gm in ((r["Hl"], r["Gl"]), (r["Hr"], r["Gr"])):
        bx, by = C.eval64(Hm, *C.eval64(Gm, gx, gy))
        assert np.abs(bx - gx).max() < bound and np.abs(by - gy).max() < bound
        assert Hm[8] == 1.0 and Gm[8] == 1.0


def test_the_mirror_program_compiles():
    """tests/cpp/rectify_test.cpp includes ssrlcv.hpp, so DisparityFactory's rectify, maskRectified and unrectifyMatches compile"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/rectify_test"])
    out = subprocess.run([os.path.join(host, "_build", "rectify_test")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    for name in ("rectify(", "maskRectified(", "unrectifyMatches("):
        assert name in factory, name
