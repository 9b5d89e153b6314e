"""Surface accuracy on the GPU (ssrlcv_hip_dsm_difference, ssrlcv_hip_difference_stats; include/ssrlcv_hip.h "surface accuracy")
against the numpy restatement of the contract (tests/accuracy_ref.py) on the cases of tests/accuracy_cases.py
(tests/test_accuracy_cases.py proves without a GPU that they test something).  Every comparison is exact: differences as bit
patterns, records as their 72 bytes, reports field for field."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import accuracy_cases as C
import accuracy_ref as A
import dsm_ref as D
import mesh_ref as M
from test_gpu_dsm import GUARD, PATTERN, Guarded, cframe, cloud_d

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t


def map_d(height):
    return torch.from_numpy(np.ascontiguousarray(height, np.float32)).cuda()


def difference(capi, points, height, fr, cells):
    """the call with guard words around diff -> the differences' bits; the inputs are left alone"""
    n = len(points)
    p, h_d = cloud_d(points), map_d(height)
    # a grid with a side below 2 has no cell: MESH mode is then a pointer to a byte that is never read
    c_d = torch.from_numpy(np.ascontiguousarray(cells).reshape(-1) if cells.size else np.zeros(1, np.uint8)).cuda() if cells is not None else None
    diff = Guarded(n)
    capi.check(capi.LIB.ssrlcv_hip_dsm_difference(vp(p.data_ptr()) if n else vp(0), u32(n), vp(h_d.data_ptr()), ctypes.byref(cframe(capi, fr)),
                                                  vp(c_d.data_ptr()) if c_d is not None else vp(0), diff.ptr, capi.stream_ptr()))
    assert h_d.cpu().numpy().tobytes() == np.ascontiguousarray(height, np.float32).tobytes()
    return diff.result().view(np.uint32)


@pytest.mark.parametrize("name", sorted(C.DIFFERENCE))
def test_difference_equals_the_reference_in_both_modes(capi, name):
    c = C.DIFFERENCE[name]
    for mesh in (False, True):
        cells = C.cells_of(name) if mesh else None
        if mesh and cells.size:   # the reference's cells are the GPU mesh's: one definition of the triangulation
            got_cells = capi.disparity_mesh(map_d(c.height), 1, c.max_jump)[1].cpu().numpy()
            assert np.array_equal(got_cells, cells)
        got, want = difference(capi, c.points, c.height, c.frame, cells), D.bits(C.difference_reference(name, mesh))
        ne = got != want
        assert not ne.any(), "%s %s: differs at %d points, first %d" % (name, "MESH" if mesh else "CELL", int(ne.sum()), int(np.nonzero(ne)[0][0]))


def test_difference_through_the_binders_and_on_a_plane(capi):
    from ssrlcv_amd import pipeline
    c = C.DIFFERENCE["relief_7x5"]
    fr = cframe(capi, c.frame)
    for mesh in (False, True):
        got = pipeline.surface_difference(cloud_d(c.points), map_d(c.height), fr, mesh=mesh, max_jump=c.max_jump)
        assert np.array_equal(H.bits(got.cpu().numpy()), D.bits(C.difference_reference("relief_7x5", mesh)))
    uncut = pipeline.surface_difference(cloud_d(c.points), map_d(c.height), fr)          # max_jump None: +inf
    assert np.array_equal(H.bits(uncut.cpu().numpy()), D.bits(A.difference(c.points, c.height, c.frame, M.mesh(c.height, 1, np.inf)[1])))
    for diagonal in sorted(C.PLANES):
        height, pfr, pts = C.plane(*C.PLANES[diagonal])
        d = pipeline.surface_difference(cloud_d(pts), map_d(height), cframe(capi, pfr)).cpu().numpy()
        fin = np.isfinite(d)
        assert fin.sum() > 300 and (d[fin] == 0).all(), diagonal


# ---- the statistics
def stats_call(capi, values, center, absolute, quantiles):
    """the call with guard words around the record and behind a workspace pre-filled with 0xFF -> the record's 72 bytes"""
    v = torch.from_numpy(np.ascontiguousarray(values, np.float32)).cuda()
    n = len(values)
    params = capi.DiffStatsParams(float(center), int(absolute), len(quantiles), (u32 * 8)(*(list(quantiles) + [0xFFFFFFFF] * (8 - len(quantiles)))))
    need = int(capi.LIB.ssrlcv_hip_difference_stats_workspace_bytes(u32(n), ctypes.byref(params)))
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out = Guarded(18)
    capi.check(capi.LIB.ssrlcv_hip_difference_stats(vp(v.data_ptr()) if n else vp(0), u32(n), ctypes.byref(params), out.ptr, vp(ws.data_ptr()), csz(need),
                                                    capi.stream_ptr()))
    assert (ws[need:] == 0xFF).all(), "the workspace was written behind its size"
    assert v.cpu().numpy().tobytes() == np.ascontiguousarray(values, np.float32).tobytes()
    return out.result().tobytes()


def assert_record(got, want, what):
    rec = np.frombuffer(got, A.RECORD)[0]
    assert got == want.tobytes(), "%s:\n got %s\nwant %s" % (what, rec, want)


@pytest.mark.parametrize("name", sorted(C.STATS))
def test_stats_equal_the_reference(capi, name):
    c = C.STATS[name]
    assert_record(stats_call(capi, c.values, c.center, c.absolute, c.quantiles), C.stats_reference(name), name)


def test_stats_where_the_tile_sums_need_a_second_level(capi):
    c = C.big_case()
    assert len(c.values) == 4096 * 4096 + 5
    assert_record(stats_call(capi, c.values, c.center, c.absolute, c.quantiles), C.stats_reference("big"), "big")


def test_the_same_call_twice_gives_the_same_record_and_the_binder_agrees(capi):
    from ssrlcv_amd import pipeline
    for name in ("n8193/eight", "random_bits", "all_equal"):
        c = C.STATS[name]
        a, b = (stats_call(capi, c.values, c.center, c.absolute, c.quantiles) for _ in range(2))
        assert a == b
        v = torch.from_numpy(np.ascontiguousarray(c.values)).cuda()
        rec = capi.difference_stats(v, c.center, c.absolute, c.quantiles)
        assert bytes(rec) == a
        got = pipeline.difference_stats(v, c.center, c.absolute, c.quantiles)
        want = C.stats_reference(name)
        m = int(want["finite"])
        assert got["finite"] == m and got["n"] == len(c.values) and got["sum"] == float(want["sum"]) and got["sum_sq"] == float(want["sumSq"])
        assert got["mean"] == float(np.float64(want["sum"]) / np.float64(m)) and got["rms"] == float(np.sqrt(np.float64(want["sumSq"]) / np.float64(m)))
        assert got["quantiles"] == [float(x) for x in want["quantile"][:len(c.quantiles)]]
    empty = pipeline.difference_stats(torch.empty(0, dtype=torch.float32, device="cuda"))
    assert empty["n"] == 0 and math.isnan(empty["mean"]) and math.isnan(empty["quantiles"][0])


# ---- end to end
def assert_report(got, want):
    for key, value in want.items():
        assert got[key] == value or (isinstance(value, float) and math.isnan(value) and math.isnan(got[key])), (key, got[key], value)


def test_surface_accuracy_of_the_fused_model_equals_the_reference_s_report(capi, tmp_path):
    """three pairs of the rendered rig -> surface model -> its accuracy against the scene's ground-truth height map: the report
    field for field, the error map, and MeshFactory's calls through tests/cpp/accuracy_test.cpp"""
    from ssrlcv_amd import pipeline
    from test_gpu_dsm import FUSE_ARGS, scene_clouds
    e, fr = scene_clouds(capi), C.DC.scene_frame()
    frame = cframe(capi, fr)
    model = pipeline.surface_model(e["clouds"], frame, rule="max", fuse=FUSE_ARGS)
    truth = C.truth_map()
    truth_d = map_d(truth)
    height = model["height"].cpu().numpy()
    cells = M.mesh(truth, 1, np.inf)[1]
    pts = D.points(height, fr)
    want_diff = A.difference(pts, truth, fr, cells)
    want = A.report(want_diff)
    got = pipeline.surface_accuracy(model["height"], truth_d, frame, want_map=True)
    assert np.array_equal(H.bits(got["diff"].cpu().numpy()), D.bits(want_diff))
    assert_report(got, want)
    print("fused model against the truth: n %d coverage %.3f bias %.4f nmad %.4f rms %.4f le90 %.4f km" % (
        got["n"], got["coverage"], got["bias"], got["nmad"], got["rms"], got["le90"]))
    assert got["coverage"] >= 0.5 and got["n"] > 1000
    assert abs(got["bias"]) < 0.5 and got["nmad"] < 0.5     # km: FUSE_ARGS' max_spread is 1 km and a pixel of disparity 0.25 to 0.5 km
    error_map = D.bits(got["error_map"].cpu().numpy())
    valid = D.bits(height) != D.INVALID_BITS
    assert (error_map[~valid] == D.INVALID_BITS).all() and np.array_equal(error_map[valid], D.bits(want_diff))
    # a cloud subject, CELL mode and a cut reference
    cloud = pipeline.surface_accuracy(e["clouds"][0], truth_d, frame, mesh=False)
    assert_report(cloud, A.report(A.difference(e["host"][0], truth, fr)))
    cut = pipeline.surface_accuracy(model["height"], truth_d, frame, max_jump=0.05)
    assert_report(cut, A.report(A.difference(pts, truth, fr, M.mesh(truth, 1, 0.05)[1])))
    assert cut["coverage"] < got["coverage"]
    with pytest.raises(ValueError):
        pipeline.surface_accuracy(e["clouds"][0], truth_d, frame, want_map=True)
    # the class API: MeshFactory::setReferenceSurface, calculatePerPointDifference, calculateAverageDifference, accuracyReport
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/accuracy_test"])
    frame_path, truth_path, cloud_path, prefix = (str(tmp_path / n) for n in ("frame.raw", "truth.raw", "cloud.raw", "out"))
    with open(frame_path, "wb") as f:
        f.write(bytes(frame))
    truth.tofile(truth_path), pts.tofile(cloud_path)
    out = subprocess.check_output([os.path.join(host, "_build", "accuracy_test"), frame_path, truth_path, cloud_path, "inf", prefix], timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    assert np.fromfile(prefix + ".diff", np.uint8).tobytes() == want_diff.tobytes()
    fields = np.fromfile(prefix + ".report", np.float64)
    keys = ("n", "coverage", "bias", "nmad", "mean", "rms", "le68", "le90", "le95", "min", "max", "average")
    mirror = dict(zip(keys, fields.tolist()))
    assert mirror.pop("average") == want["mean"]
    assert_report(mirror, want)


def test_raising_the_cloud_by_a_power_of_two_raises_the_bias_by_it_and_leaves_the_nmad(capi):
    from ssrlcv_amd import pipeline
    pts, height, fr = C.quantised_scene()
    frame, h_d = cframe(capi, fr), map_d(height)
    cells = M.mesh(height, 1, np.inf)[1]
    base = pipeline.surface_accuracy(cloud_d(pts), h_d, frame)
    assert_report(base, A.report(A.difference(pts, height, fr, cells)))
    assert base["coverage"] >= 0.5
    for delta in (0.5, 4.0):
        raised = C.quantised_scene(delta)[0]
        up = pipeline.surface_accuracy(cloud_d(raised), h_d, frame)
        assert_report(up, A.report(A.difference(raised, height, fr, cells)))
        assert up["bias"] == base["bias"] + delta and up["nmad"] == base["nmad"] and up["coverage"] == base["coverage"]
