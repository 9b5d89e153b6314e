"""What the ortho-image decides on the host (include/ssrlcv_hip.h "ortho-image"), without a GPU: the view builder
ssrlcv_dsm_ortho_view_host against a float64 numpy restatement (tests/ortho_ref.py view_of_camera) and against the geometry it
stands for, every refusal of both entry points in the stated order, and the workspace size function."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import helpers as H
import dsm_cases as DC
import dsm_ref as D
import ortho_cases as C
import ortho_ref as R

sys.path.insert(0, os.path.join(H.ROOT, "tools"))

u32, f32c, vp, csz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
NAMES = ["ssrlcv_dsm_ortho_view_host", "ssrlcv_hip_dsm_ortho_workspace_bytes", "ssrlcv_hip_dsm_ortho"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def capi():
    from ssrlcv_amd import capi
    return capi


def cframe(capi, fr):
    return capi.DsmFrame.make(fr.origin, fr.ex, fr.ey, fr.ez, fr.cell, fr.w, fr.h)


def test_header_and_loader_name_the_entry_points(capi):
    from ssrlcv_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4   # additions keep the number
    assert ctypes.sizeof(capi.OrthoView) == 80 and ctypes.sizeof(capi.OrthoParams) == 12
    surface = header[header.index("---- surface model"):header.index("---- ortho-image")]
    assert "ortho-image colours" not in surface[surface.index("Out of scope:"):] and '"ortho-image"' in surface
    block = header[header.index("---- ortho-image"):]
    block = " ".join(block[:block.index("typedef struct")].replace("*", " ").split())
    for item in ("colour images", "mean or blend", "seam smoothing", "ushbroom", "other than bilinear", "more than 8 views"):
        assert item in block[block.index("Out of scope"):], item


# ---- the view builder
def build(capi, cam, frame, out=None):
    out = capi.OrthoView() if out is None else out
    rc = capi.LIB.ssrlcv_dsm_ortho_view_host(H.P(np.ascontiguousarray(cam)) if cam is not None else None,
                                             ctypes.byref(frame) if frame is not None else None, ctypes.byref(out) if out is not None else None)
    return rc, out


def assert_view(out, cam, fr, what):
    """the builder's float32 entries against the float64 restatement: each is the restatement's value rounded to float32, or its
    float32 neighbour where the two float64 computations differ in their last bits and the value lies at a rounding boundary"""
    M, pos, eye = R.view_of_camera(cam, fr)
    for got, want in ((np.array(out.M[:], np.float32), M), (np.array(out.pos[:], np.float32), pos), (np.array(out.eye[:], np.float32), eye)):
        want32 = want.astype(np.float32)
        near = (got == want32) | (got == np.nextafter(want32, np.float32(INF))) | (got == np.nextafter(want32, np.float32(-INF)))
        assert near.all(), (what, got, want32)
        assert (np.abs(got.astype(np.float64) - want) <= np.abs(want) * 2.0 ** -23 + 1e-300).all(), what
    assert (out.w, out.h) == (int(cam["size"][0]), int(cam["size"][1]))


def test_the_builder_equals_the_restatement_on_the_rig_and_on_hand_made_cameras(capi):
    import scene
    rig = scene.PinholeRig(3, 192)
    fr = DC.scene_frame()
    for k in range(3):
        rc, out = build(capi, rig.cameras[k], cframe(capi, fr))
        assert rc == OK
        assert_view(out, rig.cameras[k], fr, "rig view %d" % k)
        bound = capi.dsm_ortho_view(rig.cameras[k], cframe(capi, fr))   # the binder returns the same record
        assert bytes(bound)[8:] == bytes(out)[8:] and bound.image is None
    for fr in (DC.axis_frame(67, 41, cell=C.CELL), D.frame(cell=0.37, w=31, h=23, **DC.SKEW)):
        for name, (cam, _) in C.cameras(DC.axis_frame(67, 41, cell=C.CELL)).items():
            rc, out = build(capi, cam, cframe(capi, fr))
            assert rc == OK, name
            assert_view(out, cam, fr, name)


def test_the_view_is_the_camera_s_geometry(capi):
    """the rig's own projection (tests/rectify_cases.py project(), the inverse of generateBundle's ray, which starts at cam_pos)
    and the view's M and pos evaluated in float64 agree on points around the patch: M is float32, a relative 2^-24 an entry, on
    pixel coordinates of size up to w = 192, three terms and a division -- 2^-24 4 w = 4.6e-5 px, doubled for pos and the rig's
    float32 camera: 1e-4 px.  And eye is the camera's position in grid coordinates."""
    import scene
    import rectify_cases as RC
    rig = scene.PinholeRig(3, 192)
    fr = DC.scene_frame()
    rng = np.random.RandomState(3)
    pts = rig.centre + rng.uniform(-8, 8, (2000, 1)) * rig.e1 + rng.uniform(-8, 8, (2000, 1)) * rig.e2 + rng.uniform(-2, 2, (2000, 1)) * rig.down
    for k in range(3):
        rc, out = build(capi, rig.cameras[k], cframe(capi, fr))
        assert rc == OK
        u, v, depth = RC.project(rig.cameras[k], rig.M[k], pts)
        d = pts - np.array(out.pos[:], np.float64)
        XYW = d @ np.array(out.M[:], np.float64).reshape(3, 3).T
        err = max(np.abs(XYW[:, 0] / XYW[:, 2] - u).max(), np.abs(XYW[:, 1] / XYW[:, 2] - v).max())
        print("view %d: the view's projection and the rig's agree to %.2e px" % (k, err))
        assert err < 1e-4 and (XYW[:, 2] > 0).all() and np.allclose(XYW[:, 2], depth, rtol=1e-5)
        q = rig.cameras[k]["cam_pos"].astype(np.float64) - fr.origin.astype(np.float64)
        want = np.array([q @ fr.ex / float(fr.cell), q @ fr.ey / float(fr.cell), q @ fr.ez], np.float64)
        assert np.allclose(np.array(out.eye[:], np.float64), want, rtol=1e-6, atol=1e-4)
    # the image pointer is left as it was
    out = capi.OrthoView()
    out.image = 0x1234
    assert build(capi, rig.cameras[0], cframe(capi, fr), out)[0] == OK and out.image == 0x1234


def test_builder_refusals_leave_out_untouched(capi):
    good = C.camera((1.0, 2.0, 30.0), (0.0, 0.0, -1.0), (64, 48), 0.5)
    frame = cframe(capi, DC.axis_frame(9, 7, cell=0.5))

    def cam(**kw):
        c = np.zeros(1, H.CAMERA)
        c[0] = good
        for k, v in kw.items():
            c[k][0] = v
        return c

    def bad_frame(**kw):
        f = cframe(capi, DC.axis_frame(9, 7, cell=0.5))
        for k, v in kw.items():
            if k == "cell":
                f.cell = v
            else:
                getattr(f, k)[1] = v
        return f

    assert build(capi, good, frame)[0] == OK
    assert build(capi, good, cframe(capi, DC.axis_frame(0, 0, cell=0.5)))[0] == OK   # an empty grid has a frame all the same
    cases = [(None, frame), (good, None),
             (good, bad_frame(cell=0.0)), (good, bad_frame(cell=-1.0)), (good, bad_frame(cell=NAN)), (good, bad_frame(cell=INF)),
             (good, bad_frame(origin=NAN)), (good, bad_frame(ex=INF)), (good, bad_frame(ey=-INF)), (good, bad_frame(ez=NAN)),
             (cam(size=(0, 48)), frame), (cam(size=(64, 0)), frame),
             (cam(foc=0.0), frame), (cam(foc=-1.0), frame), (cam(foc=NAN), frame), (cam(foc=INF), frame),
             (cam(fov=(0.0, 0.5)), frame), (cam(fov=(-0.5, 0.5)), frame), (cam(fov=(NAN, 0.5)), frame), (cam(fov=(INF, 0.5)), frame)]
    for c, f in cases:
        out = capi.OrthoView()
        ctypes.memset(ctypes.byref(out), 0xA5, ctypes.sizeof(out))
        assert build(capi, c, f, out)[0] == INVALID_ARG, (c, f)
        assert bytes(out) == b"\xA5" * 80   # `out` is untouched on any error
    assert capi.LIB.ssrlcv_dsm_ortho_view_host(H.P(np.ascontiguousarray(good)), ctypes.byref(frame), None) == INVALID_ARG
    assert build(capi, cam(fov=(0.5, NAN)), frame)[0] == OK   # fov.y is not read


# ---- the device entry point's refusals, in their order: nothing is launched, no pointer is followed
def good_view(capi, w=64, h=48, image=BOGUS):
    return capi.OrthoView(image, w, h, (f32c * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (f32c * 3)(0, 0, 0), (f32c * 3)(0, 0, 10))


def call(capi, height=BOGUS, frame="good", views="good", m=1, params="good", ortho=BOGUS, seen=BOGUS, which=BOGUS, ws=BOGUS, ws_bytes=256,
         w=9, h=7):
    fr = cframe(capi, DC.axis_frame(w, h, cell=0.5)) if frame == "good" else frame
    arr = (capi.OrthoView * 9)(*[good_view(capi) for _ in range(9)]) if views == "good" else views
    p = capi.OrthoParams(64, 0.25, 0) if params == "good" else params
    return capi.LIB.ssrlcv_hip_dsm_ortho(vp(height), ctypes.byref(fr) if fr is not None else None, arr, u32(m), ctypes.byref(p) if p is not None else None,
                                         vp(ortho), vp(seen), vp(which), vp(ws), csz(ws_bytes), vp(None))


def views_with(capi, **kw):
    arr = (capi.OrthoView * 2)(good_view(capi), good_view(capi))
    for k, v in kw.items():
        if k in ("w", "h", "image"):
            setattr(arr[1], k, v)
        else:
            getattr(arr[1], k)[2] = v
    return arr


def test_ortho_refusals_in_their_order(capi):
    bad_frame = cframe(capi, DC.axis_frame(9, 7, cell=0.5))
    bad_frame.cell = 0.0
    P = capi.OrthoParams
    huge, long_side = dict(w=65536, h=32768), dict(w=(1 << 24) + 1, h=1)
    # the parameters
    assert call(capi, frame=None) == INVALID_ARG and call(capi, frame=bad_frame) == INVALID_ARG
    assert call(capi, params=None) == INVALID_ARG and call(capi, views=None) == INVALID_ARG
    assert call(capi, m=0) == INVALID_ARG and call(capi, m=9) == INVALID_ARG
    assert call(capi, params=P(64, 0.25, 2)) == INVALID_ARG
    for bias in (-1.0, NAN, -INF, -1e-30):
        assert call(capi, params=P(64, bias, 0)) == INVALID_ARG, bias
    for kw in (dict(w=0), dict(h=0), dict(w=(1 << 24) + 1, h=1), dict(h=(1 << 24) + 1, w=1), dict(w=65536, h=32768), dict(M=NAN), dict(M=INF),
               dict(pos=NAN), dict(pos=-INF), dict(eye=NAN), dict(eye=INF)):
        assert call(capi, views=views_with(capi, **kw), m=2) == INVALID_ARG, kw
        assert call(capi, views=views_with(capi, **kw), m=1, ws_bytes=0) == WORKSPACE   # the second view is not read with m = 1
    # the parameters before the sizes: a bad parameter on a refused or an empty grid is still the parameter's refusal
    for grid in (huge, long_side, dict(w=0, h=7)):
        assert call(capi, m=0, **grid) == INVALID_ARG and call(capi, params=P(64, NAN, 0), **grid) == INVALID_ARG
        assert call(capi, views=views_with(capi, w=0), m=2, **grid) == INVALID_ARG
    # the sizes: w h >= 2^31 before a side above 2^24, both before the buffers
    assert call(capi, **huge) == INVALID_ARG and call(capi, height=None, ortho=None, ws=None, **huge) == INVALID_ARG
    assert call(capi, **long_side) == UNSUPPORTED and call(capi, height=None, ortho=None, ws=None, **long_side) == UNSUPPORTED
    assert call(capi, w=(1 << 24) + 1, h=128) == INVALID_ARG    # both: the count is refused first
    # an empty grid is nothing to do, whatever the buffers are
    for grid in (dict(w=0, h=7), dict(w=9, h=0), dict(w=0, h=0)):
        assert call(capi, **grid) == OK and call(capi, height=None, ortho=None, ws=None, ws_bytes=0, views=views_with(capi, image=None), m=2, **grid) == OK
    # the buffers, every one before the workspace's size
    for kw in (dict(height=None), dict(ortho=None), dict(ws=None), dict(views=views_with(capi, image=None), m=2)):
        assert call(capi, **kw) == INVALID_ARG and call(capi, ws_bytes=0, **kw) == INVALID_ARG, kw
    assert call(capi, ws_bytes=255) == WORKSPACE and call(capi, ws_bytes=0) == WORKSPACE
    assert call(capi, ws_bytes=255, seen=None, which=None) == WORKSPACE   # seen and which may be NULL


def test_the_workspace_size(capi):
    size = capi.LIB.ssrlcv_hip_dsm_ortho_workspace_bytes
    for w, h, m in ((1, 1, 1), (67, 41, 3), (4096, 4096, 8), (1 << 24, 127, 1), (0, 0, 1), (0, 7, 2)):
        assert size(u32(w), u32(h), u32(m)) == 256, (w, h, m)   # a256(4): the greatest height's key
    for w, h, m in ((65536, 32768, 1), ((1 << 24) + 1, 1, 1), (1, (1 << 24) + 1, 1), (9, 7, 0), (9, 7, 9)):
        assert size(u32(w), u32(h), u32(m)) == 0, (w, h, m)      # a refused size or m
