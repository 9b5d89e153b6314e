"""Dense SIFT, the part that needs no GPU: the header and the loader name the four entry points, the host-side grid and size
queries follow the contract's formulas, every refusal is decided before a device pointer is looked at, and the C++ mirror
no longer refuses dense = true."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_ref as D
import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
NAMES = ["ssrlcv_sift_dense_grid", "ssrlcv_sift_dense_max_features", "ssrlcv_hip_sift_dense_workspace_bytes",
         "ssrlcv_hip_sift_dense_u8"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


class Params(ctypes.Structure):
    _fields_ = [("stride", u32), ("sigma", f32), ("maxOrientations", u32), ("orientationThreshold", f32),
                ("orientationContribWidth", f32), ("descriptorContribWidth", f32)]


def params(stride=1, sigma=1.6, maxo=2, thr=0.8, ow=1.5, dw=6.0):
    return Params(stride, sigma, maxo, thr, ow, dw)


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    lb.ssrlcv_hip_sift_dense_workspace_bytes.restype = csz
    lb.ssrlcv_sift_dense_max_features.restype = u32
    return lb


def query(lib, w, h, p):
    m, nx, ny = u32(), u32(), u32()
    rc = lib.ssrlcv_sift_dense_grid(u32(w), u32(h), ctypes.byref(p), ctypes.byref(m), ctypes.byref(nx), ctypes.byref(ny))
    return rc, m.value, nx.value, ny.value


def test_header_and_loader_name_the_entry_points():
    from ssrlcv_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
    assert "ssrlcv_dense_params" in header
    assert ctypes.sizeof(Params) == 24


@pytest.mark.parametrize("w,h,stride,sigma,maxo", [
    (64, 48, 1, 1.6, 2), (160, 144, 1, 1.6, 1), (160, 144, 1, 1.6, 4), (97, 83, 3, 1.6, 2), (97, 83, 7, 1.6, 2),
    (128, 96, 1, 1.0, 2), (128, 96, 1, 2.3, 2), (128, 96, 4, 1.6, 2), (21, 21, 1, 1.6, 2), (22, 22, 1, 1.6, 2), (22, 21, 1, 1.6, 2),
    # one column, one row, one pixel short of either; strides from a few points per tile to the largest the ABI can name
    (22, 40, 1, 1.6, 2), (40, 22, 1, 1.6, 2), (21, 40, 1, 1.6, 2), (40, 21, 1, 1.6, 2), (128, 96, 40, 1.6, 2), (128, 96, 1000, 1.6, 2),
    (128, 96, 0x11111112, 1.6, 8), (128, 96, 0xFFFFFFFF, 1.6, 8), (100, 92, 1, 5.3, 2), (66, 66, 1, 5.3, 2), (66, 65, 0xFFFFFFFF, 5.3, 2)])
def test_grid_follows_the_formulas(lib, w, h, stride, sigma, maxo):
    p = params(stride=stride, sigma=sigma, maxo=maxo)
    m, nx, ny, _, _ = D.grid(w, h, stride, sigma)
    assert query(lib, w, h, p) == (OK, m, nx, ny)
    assert lib.ssrlcv_sift_dense_max_features(u32(w), u32(h), ctypes.byref(p)) == nx * ny * maxo
    # the formulas once more, spelled out: the last grid point is the last integer location <= size - 2 - margin
    if nx:
        assert m + (nx - 1) * stride <= w - 2 - m < m + nx * stride
        assert m + (ny - 1) * stride <= h - 2 - m < m + ny * stride
    else:
        assert w - 2 - m < m or h - 2 - m < m


def test_grid_of_a_4096_image(lib):
    """sigma 1.6: wo = ceil(7.2) = 8, wd = ceil(9.6) = 10, margin 10; x = 10 .. 4084 (<= 4096 - 2 - 10): 4075 points a side"""
    assert query(lib, 4096, 4096, params()) == (OK, 10, 4075, 4075)
    assert D.grid(4096, 4096)[:3] == (10, 4075, 4075)


def test_workspace_is_monotone_and_bounded(lib):
    last = 0
    for w, h in [(22, 22), (64, 48), (97, 83), (128, 96), (160, 144), (1024, 1024), (4096, 4096)]:
        for stride, maxo in [(4, 1), (1, 2), (1, 8)]:
            p = params(stride=stride, maxo=maxo)
            _, _, nx, ny = query(lib, w, h, p)
            need = lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(w), u32(h), ctypes.byref(p))
            assert 0 < need < 40 * w * h + 64 * nx * ny + (1 << 20), (w, h, stride, maxo, need)
        p = params()
        need = lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(w), u32(h), ctypes.byref(p))
        assert need > last
        last = need


def call(lib, p, w=64, h=48, pixels=None, ws=None, ws_bytes=0, feats=None, cap=0, count=None):
    return lib.ssrlcv_hip_sift_dense_u8(vp(pixels), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(ws), csz(ws_bytes),
                                        vp(feats), u32(cap), vp(count), vp(None))


@pytest.mark.parametrize("kw", [dict(stride=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                                dict(ow=0.0), dict(ow=float("nan")), dict(ow=float("inf")), dict(dw=-6.0), dict(dw=float("nan")),
                                dict(dw=float("inf")), dict(maxo=0), dict(maxo=9)])
def test_invalid_parameters_are_refused_before_any_launch(lib, kw):
    p = params(**kw)
    assert call(lib, p) == INVALID_ARG          # null device pointers: nothing was launched
    assert query(lib, 64, 48, p)[0] == INVALID_ARG
    assert lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(64), u32(48), ctypes.byref(p)) == 0


def test_null_pointers_and_too_many_features_are_invalid(lib):
    assert call(lib, None) == INVALID_ARG
    assert call(lib, params()) == INVALID_ARG   # valid parameters, null buffers
    assert call(lib, params(maxo=1), w=65536, h=65536) == INVALID_ARG  # 65515^2 grid points >= 2^31
    assert query(lib, 65536, 65536, params(maxo=1))[0] == INVALID_ARG
    assert query(lib, 32768, 32768, params(maxo=1))[0] == OK          # 32747^2 < 2^31
    assert query(lib, 32768, 32768, params(maxo=3))[0] == INVALID_ARG


@pytest.mark.parametrize("kw", [dict(sigma=7.2), dict(sigma=7.2, dw=1.0), dict(sigma=1.6, ow=1.0, dw=20.7)])
def test_windows_above_32_are_unsupported(lib, kw):
    p = params(**kw)
    assert call(lib, p) == UNSUPPORTED          # with null device pointers: the parameters are judged first
    assert query(lib, 64, 48, p)[0] == UNSUPPORTED


def test_the_largest_supported_windows(lib):
    # sigma 5.3: wd = ceil(31.8) = 32, wo = ceil(23.85) = 24
    assert query(lib, 200, 200, params(sigma=5.3)) == (OK, 32, 200 - 2 - 64 + 1, 200 - 2 - 64 + 1)
    # the margin is the larger of the two, whichever it is: wo = ceil(2 * 3 * 5.3) = 32, wd = ceil(2 * 3) = 6
    assert D.grid(100, 92, sigma=2.0, ori_width=5.3, desc_width=3.0) == (32, 35, 27, 32, 6)
    assert query(lib, 100, 92, params(sigma=2.0, ow=5.3, dw=3.0)) == (OK, 32, 35, 27)
    assert query(lib, 100, 92, params(sigma=5.3, ow=2.0)) == (OK, 32, 35, 27)  # both 32
    assert query(lib, 97, 83, params(ow=3.0, dw=4.0)) == (OK, 15, 66, 52)      # wo 15, wd 7


def test_workspace_of_the_longest_strides(lib):
    """one grid point however long the stride: the size queries do not wrap"""
    small = lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(128), u32(96), ctypes.byref(params(stride=1000)))
    for stride in (0x11111112, 0x80000000, 0xFFFFFFFF):
        p = params(stride=stride, maxo=8)
        assert query(lib, 128, 96, p) == (OK, 10, 1, 1)
        assert lib.ssrlcv_sift_dense_max_features(u32(128), u32(96), ctypes.byref(p)) == 8
        assert 0 < lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(128), u32(96), ctypes.byref(p)) <= small + 256


def test_short_workspace(lib):
    """buffers that are never dereferenced: the size check precedes every launch"""
    p = params()
    dummy = (ctypes.c_uint8 * 64)()
    a = ctypes.addressof(dummy)
    need = lib.ssrlcv_hip_sift_dense_workspace_bytes(u32(64), u32(48), ctypes.byref(p))
    assert call(lib, p, pixels=a, ws=a, ws_bytes=need - 1, feats=a, cap=1, count=a) == WORKSPACE
    assert call(lib, p, pixels=a, ws=a, ws_bytes=0, feats=a, cap=1, count=a) == WORKSPACE


def test_the_mirror_no_longer_refuses_dense():
    src = open(os.path.join(H.ROOT, "ssrlcv_amd", "host", "SIFT_FeatureFactory.hpp")).read()
    assert "dense SIFT is not part of" not in src
    assert "setDenseStride" in src and "setDenseSigma" in src and "ssrlcv_hip_sift_dense_u8" in src
