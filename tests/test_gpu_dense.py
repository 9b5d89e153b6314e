"""Dense SIFT (ssrlcv_hip_sift_dense_u8, include/ssrlcv_hip.h "dense SIFT") three ways: the kernels of csrc/dense.hip, the
chain of per-kernel exports that defines it (tests/dense_ref.py), and the CPU oracle's restatement of the contract
(oracle_sift_dense, tests/dense_cases.py), which shares no code with either.  Every comparison is exact: the count, descriptor
bytes, loc / sigma / theta as bit patterns, parent == -1, the chain's level L.  Dense-vs-oracle and chain-vs-oracle are
reported apart: both wrong alike points at sift_sampling.h or an export, dense alone at dense.hip.  The cases
(dense_cases.CASES; tests/test_dense_oracle.py proves each a valid input without a GPU) are the smallest that cross every
seam of the tiled kernels: more than one 16 x 16 tile of grid points in both directions, grid remainders, strides that
change the tile shape up to one point per tile and past 2^32 / 15, halos up to the limit of 32 with different tile shapes
in the two kernels, which of the two widths sets the margin, every slot count, one-point and one-line grids, and images at
the edges of the arithmetic (gradient magnitude sqrt(2) everywhere, equal peaks, single-bin and mostly empty histograms)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dense_cases as C
import dense_ref as D
import helpers as H

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

_CHAIN = {}


def image(w, h, seed, flat_share=0.0):
    return C.image(C.S(w, h, seed, flat_share))


def chain(capi, name):
    """the export chain's result of one case, computed once and shared (records, level L); never modified"""
    if name not in _CHAIN:
        spec, kw = C.CASES[name]
        _CHAIN[name] = D.dense_ref(capi, C.image(spec), **kw)
    return _CHAIN[name]


def run(capi, img, **kw):
    names = {"thr": "orientation_threshold", "ori_width": "orientation_contrib_width", "desc_width": "descriptor_contrib_width"}
    feats, n = capi.sift_dense(torch.from_numpy(img).cuda(), **{names.get(k, k): v for k, v in kw.items()})
    return capi.to_host(feats, H.FEATURE, n), n


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    assert (got["parent"] == -1).all() and (want["parent"] == -1).all()
    H.assert_features_equal(got, want)


def differences(side, got, count, want, n):
    """-> what differs between one side's records and the oracle's, as a list of findings (empty: bit-equal)"""
    if count != n or len(got) != n:
        return ["%s: count %d (%d records), oracle %d" % (side, count, len(got), n)]
    found = []
    if n == 0:
        return found
    if not (got["parent"] == -1).all():
        found.append("%s: parent != -1 in %d records" % (side, int((got["parent"] != -1).sum())))
    for name in ("loc", "sigma", "theta"):
        ne = (H.bits(got[name]) != H.bits(want[name])).reshape(n, -1).any(1)
        if ne.any():
            found.append("%s: %s differs in %d of %d records, first %d" % (side, name, int(ne.sum()), n, int(np.flatnonzero(ne)[0])))
    nd = (got["values"] != want["values"]).any(1)
    if nd.any():
        found.append("%s: descriptor bytes differ in %d of %d records, first %d" % (side, int(nd.sum()), n, int(np.flatnonzero(nd)[0])))
    return found


def check_case(capi, oracle_lib, name):
    """dense, chain and oracle agree exactly; -> the oracle's records"""
    spec, kw = C.CASES[name]
    want, n, level, stats = C.oracle_case(oracle_lib, name)
    C.assert_conditions(name, want, n, stats)
    chained, chain_level = chain(capi, name)
    got, count = run(capi, C.image(spec), **kw)
    found = differences("dense", got, count, want, n) + differences("chain", chained, len(chained), want, n)
    ne = H.bits(chain_level) != H.bits(level)
    if ne.any():
        found.append("chain: level L differs in %d of %d pixels" % (int(ne.sum()), ne.size))
    assert not found, (name, found)
    same(got, chained)
    return want


def test_base_case(capi, oracle_lib):
    want = check_case(capi, oracle_lib, "base")
    m, nx, ny, _, _ = D.grid(64, 48)
    assert (m, nx, ny) == (10, 43, 27) and len(want) >= nx * ny


@pytest.mark.parametrize("maxo", [1, 2, 4])
def test_many_tiles(capi, oracle_lib, maxo):
    """160 x 144: 139 x 123 grid points, nine by eight tiles of 16 x 16 with remainders on both sides"""
    want = check_case(capi, oracle_lib, "many_tiles_%d" % maxo)
    _, nx, ny, _, _ = D.grid(160, 144)
    assert len(want) >= nx * ny
    if maxo >= 2:
        assert len(want) > nx * ny  # second peaks exist
    assert len(want) <= nx * ny * maxo


@pytest.mark.parametrize("stride", [3, 7])
def test_odd_sizes_and_strides(capi, oracle_lib, stride):
    want = check_case(capi, oracle_lib, "stride_%d" % stride)
    assert len(want) > 0


@pytest.mark.parametrize("sigma,wo,wd", [(1.0, 5, 6), (2.3, 11, 14)])
def test_window_widths(capi, oracle_lib, sigma, wo, wd):
    assert D.grid(128, 96, sigma=sigma)[3:] == (wo, wd)
    want = check_case(capi, oracle_lib, "sigma_%.1f" % sigma)
    assert len(want) > 0


def test_holes(capi, oracle_lib):
    """the left 40 % of the image is one value: grid points whose orientation windows lie in it have all-zero histograms and
    yield nothing; the rest is unchanged"""
    want = check_case(capi, oracle_lib, "holes")
    _, nx, ny, _, _ = D.grid(160, 96)
    assert 0.3 * nx * ny < len(want) < 0.9 * nx * ny, (len(want), nx * ny)
    assert want["loc"][:, 0].min() > 40  # nothing from deep inside the flat part


@pytest.mark.parametrize("name,wo,wd", [("largest_wd", 24, 32), ("both_halos_32", 32, 32), ("wo_gt_wd", 32, 6), ("small_wo_gt_wd", 15, 7)])
def test_halos_and_margins(capi, oracle_lib, name, wo, wd):
    """halos up to the limit (at 32 k_dense_orient runs 8 x 8 tiles, k_dense_desc 16 x 16, in one call) and wo > wd, where the
    margin and k_dense_desc's tile origin come from the orientation window"""
    m, nx, ny, gwo, gwd = C.grid_of(name)
    assert (gwo, gwd, m) == (wo, wd, max(wo, wd)) and nx > 16 and ny > 16
    want = check_case(capi, oracle_lib, name)
    assert len(want) >= nx * ny


@pytest.mark.parametrize("name", ["slots_8", "slots_8_thr_1", "slots_1_low_thr"])
def test_slot_logic(capi, oracle_lib, name):
    """eight slots at a low threshold (some points fill all eight), threshold 1.0 (the maximum alone), one slot for many peaks"""
    want = check_case(capi, oracle_lib, name)
    _, nx, ny, _, _ = C.grid_of(name)
    assert len(want) > 3 * nx * ny if name == "slots_8" else len(want) == nx * ny


@pytest.mark.parametrize("stride,nx,ny", [(40, 3, 2), (1000, 1, 1), (0x11111112, 1, 1), (0xFFFFFFFF, 1, 1)])
def test_long_strides(capi, oracle_lib, stride, nx, ny):
    """a few points per tile, one point per tile, and strides whose product with a tile's 15 steps passes 2^32"""
    name = "stride_%d" % stride if stride <= 1000 else "stride_0x%X" % stride
    assert C.grid_of(name)[1:3] == (nx, ny)
    want = check_case(capi, oracle_lib, name)
    assert len(want) >= nx * ny


@pytest.mark.parametrize("stride,nx,ny", [(5, 47, 41), (10, 24, 21), (13, 19, 16), (20, 12, 11), (28, 9, 8), (60, 4, 4), (100, 3, 3)])
def test_every_tile_shape(capi, oracle_lib, stride, nx, ny):
    """256 x 224 at the strides at which pick_tile steps down (dense_cases.CASES names the shapes): with the strides above,
    every tile shape of both kernels runs, in grids of several tiles with remainders"""
    name = "tiles_stride_%d" % stride
    assert C.grid_of(name)[1:3] == (nx, ny)
    want = check_case(capi, oracle_lib, name)
    assert len(want) >= nx * ny


@pytest.mark.parametrize("name,nx,ny", [("one_point", 1, 1), ("one_column", 1, 19), ("one_row", 19, 1), ("empty_grid", 0, 0)])
def test_degenerate_grids(capi, oracle_lib, name, nx, ny):
    assert C.grid_of(name)[1:3] == (nx, ny)
    want = check_case(capi, oracle_lib, name)
    assert len(want) >= nx * ny


@pytest.mark.parametrize("name,count", [("saturated", 3010), ("saturated_wd_32", 950), ("step", 630), ("ramp", 1505), ("one_pixel", 450),
                                        ("no_gradient", 0)])
def test_edge_images(capi, oracle_lib, name, count):
    """gradient magnitude sqrt(2) at every pixel with four equal peaks per histogram; single-bin histograms; four pixels with a
    gradient; none at all (count 0, no error).  The counts are the oracle's (tests/test_dense_oracle.py derives them)."""
    want = check_case(capi, oracle_lib, name)
    assert len(want) == count


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


def test_capacity_and_empty_grid(capi, oracle_lib):
    key = (64, 48, 3)
    want, n, _, _ = C.oracle_case(oracle_lib, "base")
    assert n > 116
    pix = torch.from_numpy(image(*key)).cuda()
    p = capi.DenseParams(1, 1.6, 2, 0.8, 1.5, 6.0)
    ws = capi.dense_workspace(64, 48, p)
    twin = np.flatnonzero((want["loc"][1:] == want["loc"][:-1]).all(1))
    for cap in (100, int(twin[len(twin) // 2]) + 1):  # a round number, and between the two slots of one grid point
        buf = torch.full(((cap + 16) * 152,), 0xA5, dtype=torch.uint8, device="cuda")  # cap records + 16 guard records
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        capi.check(capi.LIB.ssrlcv_hip_sift_dense_u8(capi.ptr(pix), u32(64), u32(48), ctypes.byref(p), capi.ptr(ws), csz(ws.numel()),
                                                     capi.ptr(buf), u32(cap), capi.ptr(count), capi.stream_ptr()))
        assert int(count.item()) == n  # the full count
        host = buf.cpu().numpy()
        same(host[: cap * 152].view(H.FEATURE), want[:cap])
        assert (host[cap * 152:] == 0xA5).all()
    # capacity 0 with features == NULL: the count alone
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(capi.LIB.ssrlcv_hip_sift_dense_u8(capi.ptr(pix), u32(64), u32(48), ctypes.byref(p), capi.ptr(ws), csz(ws.numel()),
                                                 vp(None), u32(0), capi.ptr(count), capi.stream_ptr()))
    assert int(count.item()) == n
    # an image of 2 margin + 1 pixels on a side holds no grid point: count 0, no error
    side = 2 * D.grid(64, 48)[0] + 1
    tiny = torch.from_numpy(H.synthetic_image(side, side, seed=1)).cuda()
    feats, n0 = capi.sift_dense(tiny, capacity=4)
    assert n0 == 0 and feats.numel() == 0


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
