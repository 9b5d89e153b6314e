"""Surface objects on the GPU (ssrlcv_hip_dsm_objects; include/ssrlcv_hip.h "surface objects") against the numpy restatement of the
contract (tests/objects_ref.py) on the cases of tests/objects_cases.py (tests/test_objects_cases.py holds the restatement to a plain
loop without a GPU).  count, every entry of ids and every byte of every record are compared, exact.  Every output lies between
guard words, the workspace is pre-filled and checked behind its queried size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import objects_cases as C
import objects_ref as R
from test_gpu_dsm import Guarded, cframe

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
WORDS = R.RECORD.itemsize // 4


def map_d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(capi, c, capacity, fill=0xFF, want_ids=True, in_d=None):
    """one call -> (count, ids uint32 (h, w) or None, the bytes of records[0, capacity) as the device left them: uint8).  The ids,
    the records and the count lie between guard words; nothing is written behind the queried workspace; the map is left alone"""
    h, w = c.d.shape
    in_d = map_d(c.d) if in_d is None else in_d
    need = int(capi.LIB.ssrlcv_hip_dsm_objects_workspace_bytes(u32(w), u32(h)))
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    ids, records, count = Guarded(w * h) if want_ids else None, Guarded(capacity * WORDS), Guarded(1)
    p = capi.ObjectParams(c.min_height, c.max_diff, c.scale, c.min_cells)
    capi.check(capi.LIB.ssrlcv_hip_dsm_objects(vp(in_d.data_ptr()), u32(w), u32(h), ctypes.byref(p), ids.ptr if ids else vp(0),
                                               records.ptr if capacity else vp(0), u32(capacity), count.ptr, vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    assert np.array_equal(in_d.cpu().numpy().view(np.uint32), c.d.view(np.uint32)), "the map was written"
    return (int(count.result().view(np.uint32)[0]), ids.result().view(np.uint32).reshape(h, w) if ids else None,
            records.result().view(np.uint8).copy())


def assert_records(got_bytes, want, what):
    got = got_bytes[:len(want) * R.RECORD.itemsize].view(R.RECORD)
    for field in R.RECORD.names:
        a, b = (x[field].view(np.uint32) if field in ("peak", "low") else x[field] for x in (got, want))
        ne = a != b
        assert not ne.any(), "%s: %s differs at %d records, first %d: %r, not %r" % (what, field, int(ne.sum()), int(np.nonzero(ne)[0][0]), a[ne][0], b[ne][0])
    assert got.tobytes() == want.tobytes(), what


def check(capi, c, want=None):
    """capacity 0 counts, capacity count writes: both against the restatement; a second run on a zeroed workspace gives equal bytes"""
    want = C.reference(c) if want is None else want
    in_d = map_d(c.d)
    count, ids, nothing = run(capi, c, 0, in_d=in_d)
    assert count == want["count"] and len(nothing) == 0, c.name
    ne = ids != want["ids"]
    assert not ne.any(), "%s: ids differ at %d cells, first (y, x) %s: %d, not %d" % (c.name, int(ne.sum()), tuple(np.argwhere(ne)[0]), ids[ne][0], want["ids"][ne][0])
    first = run(capi, c, count, in_d=in_d)
    assert first[0] == count and np.array_equal(first[1], want["ids"]), c.name
    assert_records(first[2], want["records"], c.name)
    again = run(capi, c, count, fill=0x00, in_d=in_d)
    assert again[0] == count and np.array_equal(again[1], first[1]) and again[2].tobytes() == first[2].tobytes(), c.name   # bit-equal run to run
    without = run(capi, c, count, want_ids=False, in_d=in_d)
    assert without[0] == count and without[1] is None and without[2].tobytes() == first[2].tobytes(), c.name


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_case_of_a_size_equals_the_restatement(capi, size):
    tail = " %dx%d" % size
    cases = [c for c in C.CASES if c.name.endswith(tail)]
    assert len(cases) >= 13
    for c in cases:
        check(capi, c)


@pytest.mark.parametrize("name", ["blobs 130x35", "checkerboard 65x17", "blobs minCells 4 130x35", "hard -inf 130x35", "seams 130x35"])
def test_truncation_leaves_the_words_behind_the_capacity_alone(capi, name):
    c = C.BY_NAME[name]
    want = C.reference(c)
    count = want["count"]
    assert count >= 3
    in_d = map_d(c.d)
    for capacity in (0, 1, count - 1, count, count + 5):
        h, w = c.d.shape
        need = int(capi.LIB.ssrlcv_hip_dsm_objects_workspace_bytes(u32(w), u32(h)))
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        records, ids, got = Guarded((count + 5) * WORDS), Guarded(w * h), Guarded(1)        # room for every record: what lies behind the capacity is looked at
        p = capi.ObjectParams(c.min_height, c.max_diff, c.scale, c.min_cells)
        capi.check(capi.LIB.ssrlcv_hip_dsm_objects(vp(in_d.data_ptr()), u32(w), u32(h), ctypes.byref(p), ids.ptr, records.ptr, u32(capacity), got.ptr,
                                                   vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
        words = records.result().view(np.uint32)
        written = min(count, capacity)
        assert int(got.result().view(np.uint32)[0]) == count, capacity                  # the full number kept
        assert np.array_equal(ids.result().view(np.uint32).reshape(h, w), want["ids"]), capacity   # the numbers do not depend on the capacity
        assert_records(words[:written * WORDS].view(np.uint8), R.truncated(want, capacity)["records"], "%s capacity %d" % (name, capacity))
        assert (words[written * WORDS:] == records.pattern).all(), capacity               # pre-filled and unchanged


def test_a_map_past_the_caps_of_every_launch_grid(capi):
    c = C.large()
    want = R.objects(c.d, c.min_height, c.max_diff, c.scale, c.min_cells)
    h, w = c.d.shape
    k = C.caps()
    assert want["count"] > k["finish"] * 256 and w * h > k["mask"] * 256
    big = want["records"][-1]
    assert big["cells"] == (h - h // 2 - 1) * w and big["peakIndex"] >= (h - 1) * w and big["maxY"] == h - 1   # one object over every tile of the lower half
    in_d = map_d(c.d)
    count, ids, _ = run(capi, c, 0, in_d=in_d)
    assert count == want["count"] and np.array_equal(ids, want["ids"])
    count, ids, records = run(capi, c, count, in_d=in_d)
    assert np.array_equal(ids, want["ids"])
    assert_records(records, want["records"], c.name)


def test_an_empty_map_and_the_binder(capi):
    for w, h in ((0, 5), (5, 0), (0, 0)):                                            # nothing is looked at but the count
        count = Guarded(1)
        p = capi.ObjectParams(1.0, float("inf"), 256.0, 1)
        capi.check(capi.LIB.ssrlcv_hip_dsm_objects(vp(0), u32(w), u32(h), ctypes.byref(p), vp(0), vp(0), u32(0), count.ptr, vp(0), csz(0), capi.stream_ptr()))
        assert int(count.result().view(np.uint32)[0]) == 0
    c = C.BY_NAME["blobs minCells 4 130x35"]
    want = C.reference(c)
    count, ids, records = capi.dsm_objects(map_d(c.d), c.min_height, c.max_diff, c.min_cells, c.scale)
    assert count == want["count"] and np.array_equal(ids.cpu().numpy().view(np.uint32), want["ids"]) and records.tobytes() == want["records"].tobytes()
    count, ids, records = capi.dsm_objects(map_d(c.d), c.min_height, c.max_diff, c.min_cells, c.scale, capacity=2, want_ids=False)
    assert count == want["count"] and ids is None and records.tobytes() == want["records"][:2].tobytes()
    ws = capi.dev_bytes(1 << 22)
    assert capi.dsm_objects(map_d(c.d), c.min_height, c.max_diff, c.min_cells, c.scale, workspace=ws)[2].tobytes() == want["records"].tobytes()


def test_the_boxed_scene_through_the_pipeline_and_the_class_api(capi, tmp_path):
    """pipeline.surface_objects behind pipeline.surface_terrain on the boxed scene of tests/terrain_cases.py: the five boxes, not the
    plateau, as tests/test_objects_cases.py fixes them from the references; the measures are the host call's; and
    MeshFactory::extractObjects + objectMeasures on the same object map give the same bytes"""
    import dsm_cases as DC
    import terrain_cases as TC
    from ssrlcv_amd import pipeline
    s = C.scene_objects()
    want = s["want"]
    height = TC.scene()["height"]
    h, w = height.shape
    fr = cframe(capi, DC.axis_frame(w, h, cell=1.0))
    terrain = pipeline.surface_terrain(map_d(height), fr, **{k: v for k, v in TC.SCHEDULE.items() if k != "cell"})
    assert np.array_equal(terrain["objects"].cpu().numpy().view(np.uint32), s["objects"].view(np.uint32))
    got = pipeline.surface_objects(terrain, fr, C.SCENE_MIN_HEIGHT)
    assert got["count"] == 5 and tuple(got["records"]["cells"].tolist()) == C.SCENE_CELLS
    assert np.array_equal(got["ids"].cpu().numpy().view(np.uint32), want["ids"]) and got["records"].tobytes() == want["records"].tobytes()
    boxes = sorted(TC.BOXES, key=lambda b: b[1] * w + b[0])
    assert [(int(r["minX"]), int(r["minY"]), int(r["maxX"] - r["minX"] + 1)) for r in got["records"]] == [b[:3] for b in boxes]
    frame = R.Frame(cell=1.0, w=w, h=h)
    assert len(got["measures"]) == 5
    for rec, m in zip(want["records"], got["measures"]):
        ref = R.measures(rec, frame, 256.0)
        assert [m["world"][k] for k in range(3)] == [ref["world%d" % k] for k in range(3)]
        assert all(np.float64(m[n]).view(np.uint64) == ref[n].view(np.uint64) for n in R.MEASURES if not n.startswith("world")), m
    assert pipeline.surface_objects(terrain["objects"], fr, C.SCENE_MIN_HEIGHT, min_cells=10)["count"] == 3   # the map alone; the 1 and the 3 dropped
    # the class API
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/objects_test"])
    path = str(tmp_path / "objects.raw")
    s["objects"].tofile(path)
    out = subprocess.check_output([os.path.join(host, "_build", "objects_test"), str(w), str(h), path, "1.0", "inf", "1", "256", "1.0", str(tmp_path) + os.sep],
                                  timeout=120).decode()
    lines = out.splitlines()
    assert lines[-1] == "ok" and lines[0] == "objects 5", out
    assert np.array_equal(np.fromfile(str(tmp_path / "ids.raw"), np.uint32).reshape(h, w), want["ids"])
    assert np.fromfile(str(tmp_path / "records.raw"), np.uint8).tobytes() == want["records"].tobytes()
    measures = np.fromfile(str(tmp_path / "measures.raw"), np.float64).reshape(5, len(R.MEASURES))
    for rec, row in zip(want["records"], measures):
        ref = R.measures(rec, frame, 256.0)
        assert row.view(np.uint64).tolist() == [ref[n].view(np.uint64) for n in R.MEASURES]
