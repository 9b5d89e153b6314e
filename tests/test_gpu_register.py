"""Surface registration on the GPU (ssrlcv_hip_register_terms, ssrlcv_hip_transform_points; include/ssrlcv_hip.h "surface
registration") against the numpy restatement of the contract (tests/register_ref.py) on the cases of tests/register_cases.py
(tests/test_register_cases.py proves without a GPU that they test something).  Records are compared as their 304 bytes, points as
bit patterns; the registrations of the displaced scene are held to the bounds the reference itself meets."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import accuracy_cases as AC
import dsm_ref as D
import register_cases as C
import register_ref as R
from test_gpu_dsm import GUARD, Guarded, cframe, cloud_d

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
T = lambda n: (n + 4095) // 4096  # noqa: E731


def cpose(capi, g):
    return capi.RegisterPose.from_buffer_copy(g.tobytes())


def map_d(height):
    return torch.from_numpy(np.ascontiguousarray(height, np.float32)).cuda()


def cells_d(cells):
    # a grid with a side below 2 has no cell: a pointer to a byte that is never read
    return torch.from_numpy(np.ascontiguousarray(cells).reshape(-1) if cells.size else np.zeros(1, np.uint8)).cuda()


def terms_call(capi, c, cells, p=None, fill=0xFF):
    """the call with guard words around the record and behind a workspace pre-filled with `fill` -> the record's 304 bytes; the
    inputs are left alone"""
    n = len(c.points)
    p = cloud_d(c.points) if p is None else p
    h_d, c_d = map_d(c.height), cells_d(cells)
    need = int(capi.LIB.ssrlcv_hip_register_terms_workspace_bytes(u32(n)))
    assert need == a256(288 * T(n)) + a256(288 * T(T(n)))
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    params = capi.RegisterParams(float(c.center), float(c.gate))
    out = Guarded(76)
    capi.check(capi.LIB.ssrlcv_hip_register_terms(vp(p.data_ptr()) if n else vp(0), u32(n), ctypes.byref(cpose(capi, c.pose)), vp(h_d.data_ptr()),
                                                  ctypes.byref(cframe(capi, c.frame)), vp(c_d.data_ptr()), ctypes.byref(params), out.ptr,
                                                  vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    assert h_d.cpu().numpy().tobytes() == np.ascontiguousarray(c.height, np.float32).tobytes()
    assert c_d.cpu().numpy().tobytes()[:cells.size] == np.ascontiguousarray(cells).tobytes()
    return out.result().tobytes()


def assert_record(got, want, what):
    rec = np.frombuffer(got, R.RECORD)[0]
    assert got == want.tobytes(), "%s:\n got %s\nwant %s" % (what, rec, want)


@pytest.mark.parametrize("name", sorted(C.TERMS))
def test_terms_equal_the_reference(capi, name):
    c = C.TERMS[name]
    p = cloud_d(c.points)
    first = terms_call(capi, c, C.cells_of(name), p)
    assert_record(first, C.terms_reference(name), name)
    assert terms_call(capi, c, C.cells_of(name), p, fill=0x00) == first          # twice, and whatever the workspace held
    assert p.cpu().numpy().tobytes() == np.ascontiguousarray(c.points, np.float32).tobytes()


def test_terms_where_the_tile_sums_need_a_second_level(capi):
    c = C.big_case()
    assert len(c.points) == 4096 * 4096 + 5
    assert_record(terms_call(capi, c, C.cells_of("big")), C.terms_reference("big"), "big")


def test_terms_through_the_binder(capi):
    for name in ("relief/similarity/gated", "n8193", "grid_1x5", "n0"):
        c = C.TERMS[name]
        cells = torch.from_numpy(np.ascontiguousarray(C.cells_of(name))).cuda()
        rec = capi.register_terms(cloud_d(c.points).reshape(-1, 3), cpose(capi, c.pose), map_d(c.height), cframe(capi, c.frame), cells, c.center, c.gate)
        assert_record(bytes(rec), C.terms_reference(name), name)


@pytest.mark.parametrize("name", sorted(C.TRANSFORM))
def test_transform_equals_the_reference_also_in_place(capi, name):
    from ssrlcv_amd import pipeline
    pts, g = C.TRANSFORM[name]
    n = len(pts)
    want = D.bits(R.transform(pts, g)).reshape(-1)
    p = cloud_d(pts)
    out = Guarded(3 * n)
    capi.check(capi.LIB.ssrlcv_hip_transform_points(vp(p.data_ptr()) if n else vp(0), u32(n), ctypes.byref(cpose(capi, g)), out.ptr if n else vp(0),
                                                    capi.stream_ptr()))
    assert np.array_equal(out.result().view(np.uint32), want)
    assert p.cpu().numpy().tobytes() == np.ascontiguousarray(pts, np.float32).tobytes()
    inplace = Guarded(3 * n)
    inplace.buf[GUARD:GUARD + 3 * n] = p.reshape(-1).view(torch.int32)
    capi.check(capi.LIB.ssrlcv_hip_transform_points(inplace.ptr if n else vp(0), u32(n), ctypes.byref(cpose(capi, g)), inplace.ptr if n else vp(0),
                                                    capi.stream_ptr()))
    assert np.array_equal(inplace.result().view(np.uint32), want)
    if n:   # partial overlap is refused, and the binder gives the same points
        assert capi.LIB.ssrlcv_hip_transform_points(inplace.ptr, u32(n), ctypes.byref(cpose(capi, g)), vp(inplace.ptr.value + 4), capi.stream_ptr()) == -1   # refused before any launch
        assert np.array_equal(H.bits(pipeline.transform_cloud(p.reshape(-1, 3), cpose(capi, g)).cpu().numpy()).reshape(-1), want)


# ---- the loop
def scene_inputs(capi, similarity, outliers):
    cloud, truth, keep = C.displaced(similarity, outliers)
    return cloud, truth, keep, cloud_d(cloud), map_d(AC.truth_map()), cframe(capi, C.DC.scene_frame())


@pytest.mark.parametrize("gate", [None, 3.0])
def test_the_first_record_of_surface_register_is_the_reference_s(capi, gate):
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, False, True)
    want = C.scene_reference("rigid", gate, True)[0]
    got = pipeline.surface_register(p, ref_d, frame, dof="rigid", iterations=1, gate=gate)
    assert len(got["history"]) == 1
    h, w = got["history"][0], want["history"][0]
    assert (h["center"], h["gate"]) == (w["center"], w["gate"])
    assert_record(bytes(h["terms"]), w["terms"], "gate %s" % gate)
    assert h["used"] == w["used"] and h["inside"] == w["inside"] and h["rms"] == w["rms"]
    again = pipeline.surface_register(p, ref_d, frame, dof="rigid", iterations=3, gate=gate)
    twice = pipeline.surface_register(p, ref_d, frame, dof="rigid", iterations=3, gate=gate)
    assert bytes(again["pose"]) == bytes(twice["pose"]) and [x["delta"] for x in again["history"]] == [x["delta"] for x in twice["history"]]


@pytest.mark.parametrize("dof", ["rigid", "similarity"])
def test_the_displaced_scene_is_registered_within_a_tenth_of_a_cell(capi, dof):
    """the motion is 0.8, -0.6, 0.5 cells, 0.004, -0.003, 0.006 rad and for "similarity" a scale of 1.01"""
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, dof == "similarity", False)
    got = pipeline.surface_register(p, ref_d, frame, dof=dof, iterations=6, gate=None)
    before = C.offset_cells(cloud, R.pose(), truth, keep)
    after = C.offset_cells(cloud, np.frombuffer(bytes(got["pose"]), R.POSE)[0], truth, keep)
    print("%s: %.3f -> %.4f cells in %d iterations (the reference: %.4f)" % (dof, before, after, len(got["history"]), C.scene_reference(dof, None, False)[2]))
    assert before > 1.0 and len(got["history"]) <= 6 and after < 0.1
    moved = pipeline.transform_cloud(p, got["pose"]).cpu().numpy().astype(np.float64)
    assert np.sqrt(((moved - truth) ** 2).sum(1).mean()) / float(C.DC.scene_frame().cell) < 0.1


def test_outliers_need_the_gate(capi):
    """every tenth point raised 20 cells along ez"""
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, False, True)
    pose_of = lambda r: np.frombuffer(bytes(r["pose"]), R.POSE)[0]  # noqa: E731
    free = pipeline.surface_register(p, ref_d, frame, iterations=6, gate=None)
    gated = pipeline.surface_register(p, ref_d, frame, iterations=6, gate=3.0)
    off, on = C.offset_cells(cloud, pose_of(free), truth, keep), C.offset_cells(cloud, pose_of(gated), truth, keep)
    print("outliers: without a gate %.3f cells, with %.4f" % (off, on))
    assert off > 1.0 and on < 0.1
    assert all(h["used"] < h["inside"] for h in gated["history"])


def test_surface_accuracy_registers_first_when_asked(capi):
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, False, False)
    plain = pipeline.surface_accuracy(p, ref_d, frame)
    reg = pipeline.surface_accuracy(p, ref_d, frame, register=dict(dof="rigid", iterations=6))
    print("nmad %.4f -> %.4f, rms %.4f -> %.4f" % (plain["nmad"], reg["nmad"], plain["rms"], reg["rms"]))
    assert reg["nmad"] <= plain["nmad"] and reg["rms"] < plain["rms"]
    assert set(reg) == set(plain) | {"pose", "registration"} and "pose" not in plain
    assert isinstance(reg["pose"], capi.RegisterPose) and reg["registration"]["history"]
    again = pipeline.surface_accuracy(p, ref_d, frame, register=None)
    assert {k: v for k, v in again.items() if k != "diff"} == {k: v for k, v in plain.items() if k != "diff"}


def test_the_mirror_program_gives_the_python_loop_s_pose_and_history(capi, tmp_path):
    """MeshFactory::registerToReference and PointCloudFactory::transformPointCloud through tests/cpp/register_test.cpp"""
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, False, True)
    got = pipeline.surface_register(p, ref_d, frame, dof="rigid", iterations=4, gate=3.0)
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/register_test"])
    frame_path, truth_path, cloud_path, prefix = (str(tmp_path / n) for n in ("frame.raw", "truth.raw", "cloud.raw", "out"))
    with open(frame_path, "wb") as f:
        f.write(bytes(frame))
    AC.truth_map().tofile(truth_path), cloud.tofile(cloud_path)
    out = subprocess.check_output([os.path.join(host, "_build", "register_test"), frame_path, truth_path, cloud_path, "inf", "63", "4", "3", prefix],
                                  timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    assert np.fromfile(prefix + ".pose", np.uint8).tobytes() == bytes(got["pose"])
    history = np.fromfile(prefix + ".history", np.float64).reshape(-1, 12)      # used, inside, rms, center, gate, delta[7]
    assert len(history) == len(got["history"])
    for row, h in zip(history, got["history"]):
        assert row[:5].tolist() == [h["used"], h["inside"], h["rms"], h["center"], h["gate"]] and row[5:].tolist() == h["delta"]
    moved = np.fromfile(prefix + ".points", np.float32).reshape(-1, 3)
    assert np.array_equal(H.bits(moved), H.bits(pipeline.transform_cloud(p, got["pose"]).cpu().numpy()))
