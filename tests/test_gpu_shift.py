"""The shift search on the GPU (ssrlcv_hip_shift_search; include/ssrlcv_hip.h "shift search") against the numpy restatement of the
contract (tests/shift_ref.py) on the cases of tests/shift_cases.py (tests/test_shift_cases.py holds the restatement to a plain
loop without a GPU).  Every comparison is exact on the table's bytes.  Every call runs twice, on a workspace pre-filled with 0xFF
and with 0x00, with the table between guard words and itself pre-filled; the inputs are left alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import shift_cases as C
import shift_ref as R
from test_gpu_dsm import Guarded, cframe, cloud_d

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t


def map_d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def a256(n):
    return (n + 255) // 256 * 256


def search_call(capi, m_d, r_d, w, h, scale, fill, stride=1, center=(0, 0), radius=8, center_q=0, gate_q=R.NO_GATE):
    """-> the table's bytes, written between guard words over a pattern; nothing written behind the queried workspace"""
    p = capi.ShiftParams(float(scale), stride, center[0], center[1], radius, center_q, gate_q)
    need = int(capi.LIB.ssrlcv_hip_shift_search_workspace_bytes(u32(w), u32(h), ctypes.byref(p)))
    assert need == (2 * a256(4 * (-(-w // stride)) * (-(-h // stride))) if w * h else 0)
    size = int(capi.LIB.ssrlcv_shift_table_bytes(u32(radius)))
    assert size == 16 + 24 * (2 * radius + 1) ** 2
    ws, table = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda"), Guarded(size // 4)
    capi.check(capi.LIB.ssrlcv_hip_shift_search(vp(m_d.data_ptr()) if w * h else vp(0), vp(r_d.data_ptr()) if w * h else vp(0), u32(w), u32(h), ctypes.byref(p),
                                                table.ptr, vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    return table.result().view(np.uint8)


def assert_table(got, want, what):
    if np.array_equal(got, want):
        return
    gh, wh = got[:16].view(R.HEAD)[0], want[:16].view(R.HEAD)[0]
    assert gh == wh, "%s: head %s, not %s" % (what, gh, wh)
    ge, we = got[16:].view(R.ENTRY), want[16:].view(R.ENTRY)
    bad = np.nonzero(ge != we)[0]
    raise AssertionError("%s: %d of %d entries differ, first %d: %s, not %s" % (what, len(bad), len(ge), bad[0], ge[bad[0]], we[bad[0]]))


def check(capi, name, moving, reference, scale, params):
    h, w = moving.shape
    m_d, r_d = map_d(moving), map_d(reference)
    for p in params:
        want = R.table_bytes(*R.search(moving, reference, scale, **p))
        what = "%s %d x %d %s" % (name, w, h, p)
        first = search_call(capi, m_d, r_d, w, h, scale, 0xFF, **p)
        assert_table(first, want, what)
        assert np.array_equal(first, search_call(capi, m_d, r_d, w, h, scale, 0x00, **p)), what      # the workspace's content, and run to run
    assert np.array_equal(m_d.cpu().numpy().view(np.uint32), np.ascontiguousarray(moving, np.float32).view(np.uint32))   # the inputs are left alone
    assert np.array_equal(r_d.cpu().numpy().view(np.uint32), np.ascontiguousarray(reference, np.float32).view(np.uint32))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_table_equals_the_restatement(capi, size):
    """radii 0, 1, 3, 5, 7, 8 and 32, strides 1, 2, 3 and 5, centres (0, 0), (5, -3), far out and +-2^24, gates 0, 1, wide and none
    about centres up to +-2^18, on maps with 30 % and 10 % holes"""
    w, h = size
    moving, reference = C.pair(w, h)
    check(capi, "pair", moving, reference, C.SCALE, C.PARAMS)


def test_invalid_maps_clipping_and_the_64_bit_sums(capi):
    for name, (moving, reference, scale, params) in C.contents().items():
        check(capi, name, moving, reference, scale, params)
    clip = C.clip_map()
    h, w = clip.shape
    head = search_call(capi, map_d(clip), map_d(clip[::-1].copy()), w, h, C.SCALE, 0xFF, radius=1)[:16].view(R.HEAD)[0]
    assert head["clippedMoving"] == head["clippedReference"] == C.CLIPPED_IN_CLIP_MAP
    assert head["validMoving"] == head["validReference"] == w * h - C.INVALID_IN_CLIP_MAP
    moving, reference, scale, params = C.contents()["wide_plus"]
    e = search_call(capi, map_d(moving), map_d(reference), 512, 512, scale, 0xFF, **params[0])[16:].view(R.ENTRY)[4]
    assert (int(e["n"]), int(e["sum"]), int(e["sumSq"])) == (1 << 18, 1 << 35, 1 << 52)


def test_more_tiles_than_the_search_grid_and_more_cells_than_a_quantise_trip(capi):
    moving, reference = C.beyond_caps()
    check(capi, "beyond_caps", moving, reference, C.SCALE, (dict(radius=1), dict(radius=1, center=(-1, 1), center_q=0, gate_q=0)))


def test_the_binders_an_empty_grid_and_the_pick(capi):
    moving, reference = C.pair(130, 35)
    m_d, r_d = map_d(moving), map_d(reference)
    ws = capi.dev_bytes(2 * a256(4 * 130 * 35))
    for p in (dict(radius=7), dict(stride=2, center=(1, 0), radius=3, center_q=20, gate_q=200)):
        got = capi.shift_search(m_d, r_d, C.SCALE, ws=ws, **p)
        head, entries = R.search(moving, reference, C.SCALE, **p)
        assert np.array_equal(got["bytes"], R.table_bytes(head, entries)) and got["head"] == head and np.array_equal(got["entries"], entries)
        assert got["entries"].shape == (2 * p["radius"] + 1,) * 2
        for min_overlap in (0, 300, 10 ** 6):
            res, want = capi.shift_pick(got, got["params"], min_overlap), R.pick(entries, C.SCALE, p.get("stride", 1), p.get("center", (0, 0)), min_overlap)
            assert (want is None) == (min_overlap == 10 ** 6)
            if want is None:
                assert res is None
                continue
            assert (res.shiftX, res.shiftY, res.n, res.candidates) == (*want["shift"], want["n"], want["candidates"])
            assert (res.subX, res.subY, res.bias, res.variance, res.second) == (*want["sub"], want["bias"], want["variance"], want["second"])
        assert capi.shift_pick(got["bytes"], got["params"], 0).n == capi.shift_pick(got, got["params"], 0).n   # the bytes alone do
    for w, h in ((0, 5), (5, 0), (0, 0)):                                # an empty grid: the table of zeros, no buffer looked at
        table = search_call(capi, None, None, w, h, C.SCALE, 0xFF, radius=2)
        assert table.size == 16 + 24 * 25 and not table.any()
        assert capi.shift_pick(table, capi.ShiftParams(C.SCALE, 1, 0, 0, 2, 0, R.NO_GATE), 0) is None


def scene_inputs(capi, outliers):
    import accuracy_cases as AC
    import dsm_cases as DC
    cloud, truth, keep = C.displaced(outliers)
    return cloud, truth, keep, cloud_d(cloud), map_d(AC.truth_map()), cframe(capi, DC.scene_frame())


def offset_cells(capi_pose, cloud, truth, keep):
    import register_cases as RC
    import register_ref as RR
    return RC.offset_cells(cloud, np.frombuffer(bytes(capi_pose), RR.POSE)[0], truth, keep)


@pytest.mark.parametrize("outliers", [False, True], ids=["clean", "raised"])
def test_the_displaced_scene_is_found_and_registered_within_a_tenth_of_a_cell(capi, outliers):
    """the cloud of the truth map, 7.3, -4.6, 0.5 cells and register_cases.MOTION_ROTATION about its centroid off; with `raised`
    every tenth point lies 20 cells higher and the gate is 3 NMAD"""
    import accuracy_cases as AC
    import dsm_cases as DC
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, outliers)
    gate = 3.0 if outliers else None
    cell = float(DC.scene_frame().cell)
    plain = pipeline.surface_register(p, ref_d, frame, iterations=6, gate=gate)
    print("plain surface_register from %.3f cells off: %.4f cells after %d iterations" % (
        offset_cells(capi.RegisterPose.make(), cloud, truth, keep), offset_cells(plain["pose"], cloud, truth, keep), len(plain["history"])))
    found = pipeline.surface_shift_search(p, ref_d, frame, gate=gate)
    last = found["levels"][-1]["result"]
    assert (last.shiftX, last.shiftY) == (7, -5)                          # before the sub-cell step
    assert abs(found["shift"][0] - 7) <= 0.5 and abs(found["shift"][1] + 5) <= 0.5 and abs(found["bias"] / cell + C.MOTION_CELLS[2]) < 0.1
    after_search = offset_cells(found["pose"], cloud, truth, keep)
    assert after_search < 0.8                                            # the start test_gpu_register's scene converges from
    # the restatement's levels on the restatement's rasterisation: the same tables and the same record
    want = R.levels(C.displaced_map(outliers), AC.truth_map(), cell, gate=gate)
    for lv, wl in zip(found["levels"], want["levels"]):
        assert np.array_equal(lv["table"]["bytes"], R.table_bytes(wl["head"], wl["entries"]))
        assert (lv["params"].centerQ, lv["params"].gateQ) == (wl["params"]["center_q"], wl["params"]["gate_q"])
    assert found["shift"] == want["shift"] and (found["bias"], found["variance"], found["second"]) == (want["bias"], want["variance"], want["second"])
    got = pipeline.surface_register_coarse(p, ref_d, frame, dict(gate=gate), iterations=6, gate=gate)
    after = offset_cells(got["pose"], cloud, truth, keep)
    print("search: %.3f cells off, registered from there: %.5f cells in %d iterations; variance %.5f, second %.5f" % (
        after_search, after, len(got["history"]), found["variance"], found["second"]))
    assert after < 0.1 and got["search"]["shift"] == found["shift"]
    moved = pipeline.transform_cloud(p, got["pose"]).cpu().numpy().astype(np.float64)[keep]
    assert np.sqrt(((moved - truth[keep]) ** 2).sum(1).mean()) / cell < 0.1
    # a height-map subject gives the same search, and surface_accuracy passes the search through
    as_map = pipeline.surface_shift_search(capi.dsm_rasterize(p, frame, capi.DSM_MAX, False, False)[0], ref_d, frame, gate=gate)
    assert as_map["shift"] == found["shift"] and bytes(as_map["pose"]) == bytes(found["pose"])
    report = pipeline.surface_accuracy(p, ref_d, frame, register=dict(search=dict(gate=gate), iterations=6, gate=gate))
    assert bytes(report["pose"]) == bytes(got["pose"]) and report["registration"]["search"]["shift"] == found["shift"]


def test_a_level_without_a_candidate_raises(capi):
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, False)
    with pytest.raises(capi.SsrlcvError):
        pipeline.surface_shift_search(p, ref_d, frame, min_overlap=2.0)


def test_the_mirror_program_gives_the_python_search(capi, tmp_path):
    """MeshFactory::searchShift and registerToReference from its pose through tests/cpp/shift_test.cpp"""
    import accuracy_cases as AC
    from ssrlcv_amd import pipeline
    cloud, truth, keep, p, ref_d, frame = scene_inputs(capi, True)
    moving = capi.dsm_rasterize(p, frame, capi.DSM_MAX, False, False)[0]
    found = pipeline.surface_shift_search(moving, ref_d, frame, radius=8, strides=(4, 1), gate=3.0)
    got = pipeline.surface_register(p, ref_d, frame, iterations=4, gate=3.0, initial=found["pose"])
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/shift_test"])
    paths = {k: str(tmp_path / k) for k in ("frame.raw", "moving.raw", "reference.raw", "cloud.raw", "out")}
    open(paths["frame.raw"], "wb").write(bytes(frame))
    moving.cpu().numpy().tofile(paths["moving.raw"])
    AC.truth_map().tofile(paths["reference.raw"])
    cloud.tofile(paths["cloud.raw"])
    out = subprocess.check_output([os.path.join(host, "_build", "shift_test"), paths["frame.raw"], paths["moving.raw"], paths["reference.raw"], "8", "4,1", "3.0",
                                   "0.25", paths["out"], paths["cloud.raw"], "4"], timeout=120).decode()
    lines = out.splitlines()
    assert lines[-1] == "ok", out

    def fnv1a(raw):
        hash_ = 0xcbf29ce484222325
        for b in raw.tobytes():
            hash_ = ((hash_ ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return hash_
    bits = lambda v: "%016x" % np.float64(v).view(np.uint64)  # noqa: E731
    for k, lv in enumerate(found["levels"]):
        q, r = lv["params"], lv["result"]
        assert "level %d stride %d center %d %d radius %d centerQ %d gateQ %d checksum %016x" % (
            k, q.stride, q.centerX, q.centerY, q.radius, q.centerQ, q.gateQ, fnv1a(lv["table"]["bytes"])) in lines, out
        assert "result %d %d %d %d %s %s %s %s %s" % (r.shiftX, r.shiftY, r.n, r.candidates, bits(r.subX), bits(r.subY), bits(r.bias), bits(r.variance),
                                                      bits(r.second)) in lines, out
    assert "shift %.17g %.17g" % found["shift"] in lines, out
    assert open(paths["out"] + ".pose", "rb").read() == bytes(found["pose"])
    assert np.array_equal(np.fromfile(paths["out"] + ".table", np.uint8), found["levels"][-1]["table"]["bytes"])
    assert "registered %d converged %d" % (len(got["history"]), int(got["converged"])) in lines, out
    assert open(paths["out"] + ".registered", "rb").read() == bytes(got["pose"])
