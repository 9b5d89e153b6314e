"""Dense SIFT (ssrlcv_hip_sift_dense_u8, include/ssrlcv_hip.h "dense SIFT") against the chain of per-kernel exports that
defines it (tests/dense_ref.py).  Every comparison is exact: descriptor bytes, loc / sigma / theta as bit patterns,
parent == -1, the count.  The shapes are the smallest that cross every seam of the tiled kernels (csrc/dense.hip): more
than one 16 x 16 tile of grid points in both directions, grid remainders, strides that change the tile shape, window widths
that change the tables and which of the two widths sets the margin."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dense_ref as D
import helpers as H

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

_IMAGES, _REFS = {}, {}


def image(w, h, seed, flat_share=0.0):
    key = (w, h, seed, flat_share)
    if key not in _IMAGES:
        img = H.synthetic_image(w, h, seed=seed)
        if flat_share:
            img = img.copy()
            img[:, : int(round(w * flat_share))] = 128
        _IMAGES[key] = img
    return _IMAGES[key]


def ref(capi, img_key, **kw):
    """the reference of one case, computed once and shared (records, level L); never modified"""
    key = (img_key, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = D.dense_ref(capi, image(*img_key), **kw)
    return _REFS[key]


def run(capi, img, **kw):
    names = {"thr": "orientation_threshold", "ori_width": "orientation_contrib_width", "desc_width": "descriptor_contrib_width"}
    feats, n = capi.sift_dense(torch.from_numpy(img).cuda(), **{names.get(k, k): v for k, v in kw.items()})
    return capi.to_host(feats, H.FEATURE, n), n


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    assert (got["parent"] == -1).all() and (want["parent"] == -1).all()
    H.assert_features_equal(got, want)


def check_case(capi, img_key, **kw):
    want, _ = ref(capi, img_key, **kw)
    got, n = run(capi, image(*img_key), **kw)
    assert n == len(want), (n, len(want))
    same(got, want)
    return want


def test_base_case(capi):
    want = check_case(capi, (64, 48, 3), stride=1, sigma=1.6, max_orientations=2)
    m, nx, ny, _, _ = D.grid(64, 48)
    assert (m, nx, ny) == (10, 43, 27) and len(want) >= nx * ny


@pytest.mark.parametrize("maxo", [1, 2, 4])
def test_many_tiles(capi, maxo):
    """160 x 144: 139 x 123 grid points, nine by eight tiles of 16 x 16 with remainders on both sides"""
    want = check_case(capi, (160, 144, 5), stride=1, sigma=1.6, max_orientations=maxo)
    _, nx, ny, _, _ = D.grid(160, 144)
    assert len(want) >= nx * ny
    if maxo >= 2:
        assert len(want) > nx * ny  # second peaks exist
    assert len(want) <= nx * ny * maxo


@pytest.mark.parametrize("stride", [3, 7])
def test_odd_sizes_and_strides(capi, stride):
    want = check_case(capi, (97, 83, 7), stride=stride, sigma=1.6, max_orientations=2)
    assert len(want) > 0


@pytest.mark.parametrize("sigma,wo,wd", [(1.0, 5, 6), (2.3, 11, 14)])
def test_window_widths(capi, sigma, wo, wd):
    assert D.grid(128, 96, sigma=sigma)[3:] == (wo, wd)
    want = check_case(capi, (128, 96, 11), stride=1, sigma=sigma, max_orientations=2)
    assert len(want) > 0


def test_holes(capi):
    """the left 40 % of the image is one value: grid points whose orientation windows lie in it have all-zero histograms and
    yield nothing; the rest is unchanged"""
    key = (160, 96, 13, 0.4)
    want = check_case(capi, key, stride=1, sigma=1.6, max_orientations=1)
    _, nx, ny, _, _ = D.grid(160, 96)
    assert 0.3 * nx * ny < len(want) < 0.9 * nx * ny, (len(want), nx * ny)
    assert want["loc"][:, 0].min() > 40  # nothing from deep inside the flat part


def test_subset_property(capi):
    """no reference involved: the stride-4 grid is the stride-1 grid restricted to every fourth point, field by field, in order"""
    img = image(128, 96, 11)
    m = D.grid(128, 96)[0]
    fine, _ = run(capi, img, stride=1, max_orientations=2)
    coarse, n4 = run(capi, img, stride=4, max_orientations=2)
    x, y = fine["loc"][:, 0].astype(np.int64), fine["loc"][:, 1].astype(np.int64)
    keep = ((x - m) % 4 == 0) & ((y - m) % 4 == 0)
    assert n4 > 0 and keep.sum() == n4
    same(coarse, fine[keep])


def test_capacity_and_empty_grid(capi):
    key = (64, 48, 3)
    want, _ = ref(capi, key, stride=1, sigma=1.6, max_orientations=2)
    assert len(want) > 116
    pix = torch.from_numpy(image(*key)).cuda()
    p = capi.DenseParams(1, 1.6, 2, 0.8, 1.5, 6.0)
    ws = capi.dense_workspace(64, 48, p)
    buf = torch.full((116 * 152,), 0xA5, dtype=torch.uint8, device="cuda")  # 100 records + 16 guard records
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(capi.LIB.ssrlcv_hip_sift_dense_u8(capi.ptr(pix), u32(64), u32(48), ctypes.byref(p), capi.ptr(ws), csz(ws.numel()),
                                                 capi.ptr(buf), u32(100), capi.ptr(count), capi.stream_ptr()))
    assert int(count.item()) == len(want)  # the full count
    host = buf.cpu().numpy()
    same(host[: 100 * 152].view(H.FEATURE), want[:100])
    assert (host[100 * 152:] == 0xA5).all()
    # an image of 2 margin + 1 pixels on a side holds no grid point: count 0, no error
    side = 2 * D.grid(64, 48)[0] + 1
    tiny = torch.from_numpy(H.synthetic_image(side, side, seed=1)).cuda()
    feats, n = capi.sift_dense(tiny, capacity=4)
    assert n == 0 and feats.numel() == 0


def test_cpu_oracle_cross_check(capi, oracle_lib):
    """up to 200 evenly spaced features of the base case: the CPU oracle's descriptor of the same key point on the host copy
    of L, all 128 bytes"""
    key = (64, 48, 3)
    _, level = ref(capi, key, stride=1, sigma=1.6, max_orientations=2)
    got, n = run(capi, image(*key), stride=1, sigma=1.6, max_orientations=2)
    pick = np.unique(np.linspace(0, n - 1, min(n, 200)).astype(np.int64))
    level = np.ascontiguousarray(level, np.float32)
    for i in pick:
        kp = np.zeros(1, H.SSKEYPOINT)
        kp["loc"], kp["sigma"], kp["theta"] = got["loc"][i], got["sigma"][i], got["theta"][i]
        ft = np.zeros(1, H.FEATURE)
        oracle_lib.oracle_fill_descriptor(H.P(level), u32(64), u32(48), f32(1.0), f32(6.0), H.P(kp), H.P(ft))
        assert np.array_equal(ft["values"][0], got["values"][i]), int(i)


def test_pipeline_binder_and_matcher(capi):
    from ssrlcv_amd import pipeline
    img = image(64, 48, 3)
    pix = torch.from_numpy(img).cuda()
    direct, n = capi.sift_dense(pix, stride=2, sigma=1.6, max_orientations=2)
    out = pipeline.extract_features_dense({0: pix, 1: pix}, stride=2, sigma=1.6, max_orientations=2)
    assert n > 100 and torch.equal(out[0], direct) and torch.equal(out[1], direct)
    # matched against itself, every feature finds itself or a byte-identical twin.  (The ratio test refuses a query whose two
    # nearest targets are equally far, include/ssrlcv_hip.h -- a query WITH a twin -- so the input must have none.)
    values = capi.to_host(direct, H.FEATURE, n)["values"]
    assert len(np.unique(values, axis=0)) == n, "the image gives byte-identical descriptors: take another seed"
    pairs = pipeline.match_pairs([out[0], out[1]], None, mode=0, ratio=0.8, mutual=True)[0]
    pairs = capi.to_host(pairs, H.UINT2_PAIR)
    assert len(pairs) == n
    assert np.array_equal(values[pairs["a"][:, 1]], values[pairs["b"][:, 1]])
    assert np.array_equal(np.sort(pairs["a"][:, 1]), np.arange(n))


def test_feature_factory_dense_through_class_api(capi, tmp_path):
    """SIFT_FeatureFactory::generateFeatures(image, true, 2) with setDenseStride(2) (tests/cpp/dense_sift_test.cpp) writes
    the records the Python binder gives"""
    img = image(64, 48, 3)
    raw = str(tmp_path / "image.raw")
    img.tofile(raw)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ssrlcv_amd", "host"), "_build/dense_sift_test"])
    exe = os.path.join(ROOT, "ssrlcv_amd", "host", "_build", "dense_sift_test")
    path = str(tmp_path / "features.bin")
    out = subprocess.check_output([exe, raw, "64", "48", "2", path]).decode()
    assert out.splitlines()[-1] == "ok", out
    feats, n = capi.sift_dense(torch.from_numpy(img).cuda(), stride=2, sigma=1.6, max_orientations=2)
    want = capi.to_host(feats, H.FEATURE, n)
    got = np.fromfile(path, np.uint8).view(H.FEATURE)
    assert n > 0
    same(got, want)
