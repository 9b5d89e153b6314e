"""The point-cloud stage without a GPU: the C ABI exports k-NN, the neighbour-distance filter and normals (ABI still 4:
pure additions), sizes their workspaces and refuses bad arguments before any device work; the numpy reference the GPU
tests hold csrc/cloud.hip to agrees with plain brute force; writePLY with normals round-trips through the C++ mirror."""
import ctypes
import os
import subprocess

import numpy as np

import cloud_ref as R
import helpers as H

NEW = ("ssrlcv_hip_knn_workspace_bytes", "ssrlcv_hip_knn", "ssrlcv_hip_neighbor_filter_workspace_bytes",
       "ssrlcv_hip_neighbor_distance_filter", "ssrlcv_hip_point_normals")
INVALID_ARG, WORKSPACE = -1, -3
u32, f32, sz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


def _lib():
    from ssrlcv_amd import _lib
    return _lib.load()


def test_cloud_symbols_exported_by_both_libraries():
    from ssrlcv_amd import _lib
    for path in (_lib.RELEASE_LIB_PATH, _lib.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert name in _lib.EXPORTED and hasattr(lib, name), (path, name)
        assert lib.ssrlcv_hip_abi_version() == 4


def test_workspace_grows_with_points():
    lib = _lib()
    for q in (lib.ssrlcv_hip_knn_workspace_bytes, lib.ssrlcv_hip_neighbor_filter_workspace_bytes):
        sizes = [q(u32(n), u32(16)) for n in (17, 1000, 300000, 4000000)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert all(q(u32(1000), u32(k)) >= q(u32(1000), u32(1)) for k in (8, 16, 32))
    assert lib.ssrlcv_hip_knn_workspace_bytes(u32(4000000), u32(16)) >= 4000000 * 16  # the cell-ordered copy


def _knn(lib, pts, n, k, cell, nbr, ws, wsb):
    return lib.ssrlcv_hip_knn(vp(pts), u32(n), u32(k), f32(cell), vp(nbr), vp(0), vp(0), vp(ws), sz(wsb), vp(0))


def _filt(lib, pts, n, d2, k, stats, pout, iout, cnt, ws, wsb, nin=0, nout=0, sigma=2.0):
    return lib.ssrlcv_hip_neighbor_distance_filter(vp(pts), u32(n), vp(d2), u32(k), f32(sigma), vp(0), vp(stats), vp(pout),
                                                   vp(iout), vp(nin), vp(nout), vp(cnt), vp(ws), sz(wsb), vp(0))


class _F3(ctypes.Structure):
    _fields_ = [("x", f32), ("y", f32), ("z", f32)]


def test_argument_checks_come_before_device_work():
    """Bogus (never dereferenced) pointers: every check below must return before the first HIP call."""
    lib = _lib()
    P = 1 << 20
    n = 100
    need = lib.ssrlcv_hip_knn_workspace_bytes(u32(n), u32(16))
    assert _knn(lib, P, n, 0, 0.0, P, P, need) == INVALID_ARG          # k = 0
    assert _knn(lib, P, n, 33, 0.0, P, P, need) == INVALID_ARG         # k = 33
    assert _knn(lib, P, 16, 16, 0.0, P, P, need) == INVALID_ARG        # n = k
    assert _knn(lib, 0, n, 16, 0.0, P, P, need) == INVALID_ARG         # points NULL
    assert _knn(lib, P, n, 16, 0.0, 0, P, need) == INVALID_ARG         # neighbours NULL
    assert _knn(lib, P, n, 16, 0.0, P, 0, need) == INVALID_ARG         # workspace NULL
    for cell in (-1.0, float("nan"), float("inf")):
        assert _knn(lib, P, n, 16, cell, P, P, need) == INVALID_ARG, cell
    assert _knn(lib, P, n, 16, 0.0, P, P, need - 1) == WORKSPACE
    fneed = lib.ssrlcv_hip_neighbor_filter_workspace_bytes(u32(n), u32(16))
    assert _filt(lib, P, n, P, 0, P, P, P, P, P, fneed) == INVALID_ARG
    assert _filt(lib, P, n, P, 33, P, P, P, P, P, fneed) == INVALID_ARG
    assert _filt(lib, P, 16, P, 16, P, P, P, P, P, fneed) == INVALID_ARG
    for i in range(7):  # points, dist2, stats, pointsOut, indexOut, count, workspace
        a = [P] * 7
        a[i] = 0
        assert _filt(lib, a[0], n, a[1], 16, a[2], a[3], a[4], a[6], a[5], fneed) == INVALID_ARG, i
    assert _filt(lib, P, n, P, 16, P, P, P, P, P, fneed, nin=P) == INVALID_ARG   # normals in without out
    assert _filt(lib, P, n, P, 16, P, P, P, P, P, fneed, sigma=float("nan")) == INVALID_ARG
    assert _filt(lib, P, n, P, 16, P, P, P, P, P, fneed - 1) == WORKSPACE
    v = _F3(0.0, 0.0, 0.0)
    norm = lib.ssrlcv_hip_point_normals
    assert norm(vp(P), u32(n), vp(P), u32(0), v, vp(P), vp(0)) == INVALID_ARG
    assert norm(vp(P), u32(n), vp(P), u32(33), v, vp(P), vp(0)) == INVALID_ARG
    assert norm(vp(P), u32(16), vp(P), u32(16), v, vp(P), vp(0)) == INVALID_ARG
    assert norm(vp(0), u32(n), vp(P), u32(16), v, vp(P), vp(0)) == INVALID_ARG
    assert norm(vp(P), u32(n), vp(0), u32(16), v, vp(P), vp(0)) == INVALID_ARG
    assert norm(vp(P), u32(n), vp(P), u32(16), v, vp(0), vp(0)) == INVALID_ARG
    assert norm(vp(P), u32(n), vp(P), u32(16), _F3(float("nan"), 0.0, 0.0), vp(P), vp(0)) == INVALID_ARG


def test_reference_agrees_with_brute_force():
    assert R.self_test()


def test_reference_filter_and_normals_on_terrain():
    """On terrain + 1 % outliers displaced 1-5 km (k = 16, sigma = 2), the reference removes >= 99 % of the outliers and
    <= 5 % of the terrain (measured: 100 % and 0 % at 3e5 points), and its normals of a flat patch are the vertical."""
    p, out, up = R.terrain_cloud(60000, seed=7)
    nbr, d2 = R.knn(p, 16)
    m = R.mean_distance(d2, 16)
    keep = R.filter_mask(m, R.filter_stats(m, 2.0)[2])
    assert (~keep[out]).mean() >= 0.99 and (~keep[~out]).mean() <= 0.05
    g = np.stack(np.meshgrid(np.arange(30), np.arange(30), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    flat = np.concatenate([g, np.zeros((len(g), 1), np.float32)], 1)
    fn, gap = R.normals(flat, R.knn(flat, 8)[0], 8, (0, 0, -10))
    assert np.allclose(fn, [0, 0, -1])


def test_ply_with_normals_round_trip(tmp_path):
    """writePLY(points, normals) of the C++ mirror, host only: header and nine-digit floats that read back bit for bit."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "host"), "_build/mesh_factory_test"])
    exe = os.path.join(H.ROOT, "ssrlcv_amd", "host", "_build", "mesh_factory_test")
    out = subprocess.check_output([exe, "ply", str(tmp_path)]).decode()
    assert out.strip().splitlines()[-1] == "ok"
    text = open(tmp_path / "tri.ply").read().splitlines()
    assert text[:11] == ["ply", "format ascii 1.0", "comment author: SSRLCV simple PLY writer (MI355X build)",
                         "element vertex 3", "property float x", "property float y", "property float z",
                         "property float nx", "property float ny", "property float nz", "end_header"]
    rows = np.array([[np.float32(x) for x in line.split()] for line in text[11:]], np.float32)
    want = np.array([[6371.00049, -0.1, 1e-7, 0, 0, 1], [1 / 3, 2.5, -3.25e5, 0.577350269, -0.577350269, 0.577350269],
                     [0, -0.0, 123456.789, 0, 0, 0]], np.float32)
    assert rows.shape == (3, 6) and np.array_equal(rows.view(np.uint32), want.view(np.uint32))
