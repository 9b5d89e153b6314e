"""The terrain filter on the GPU (ssrlcv_hip_dsm_morphology, _dsm_terrain, _dsm_subtract; include/ssrlcv_hip.h "terrain filter")
against the numpy restatement of the contract (tests/terrain_ref.py) on the cases of tests/terrain_cases.py
(tests/test_terrain_cases.py holds the restatement to a plain loop without a GPU).  Every comparison is exact on bit patterns.
Every call runs twice, on a workspace pre-filled with 0xFF and with 0x00, between guard words."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import terrain_cases as C
import terrain_ref as R
from test_gpu_dsm import Guarded, cframe

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
OPS = (R.ERODE, R.DILATE, R.OPEN, R.CLOSE)


def map_d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def a256(n):
    return (n + 255) // 256 * 256


def workspace(need, fill):
    return torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")


def morphology_call(capi, in_d, w, h, radius, op, fill):
    """-> the output's bits (h, w), written between guard words, nothing written behind the queried workspace"""
    need = int(capi.LIB.ssrlcv_hip_dsm_morphology_workspace_bytes(u32(w), u32(h)))
    assert need == 2 * a256(4 * w * h)
    ws, out = workspace(need, fill), Guarded(w * h)
    capi.check(capi.LIB.ssrlcv_hip_dsm_morphology(vp(in_d.data_ptr()), out.ptr, u32(w), u32(h), u32(radius), u32(op), vp(ws.data_ptr()), csz(need),
                                                  capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    return out.result().view(np.uint32).reshape(h, w)


def terrain_call(capi, in_d, w, h, radii, thresholds, fill, want_level=True, want_opened=True):
    """-> (terrain bits, level or None, opened bits or None)"""
    need = int(capi.LIB.ssrlcv_hip_dsm_terrain_workspace_bytes(u32(w), u32(h)))
    assert need == 4 * a256(4 * w * h)
    p = capi.TerrainParams(len(radii), (u32 * 8)(*radii), (ctypes.c_float * 8)(*thresholds))
    ws, terrain = workspace(need, fill), Guarded(w * h)
    level = Guarded(w * h, dtype=torch.uint8) if want_level else None
    opened = Guarded(w * h) if want_opened else None
    capi.check(capi.LIB.ssrlcv_hip_dsm_terrain(vp(in_d.data_ptr()), u32(w), u32(h), ctypes.byref(p), terrain.ptr, level.ptr if level else vp(0),
                                               opened.ptr if opened else vp(0), vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    return (terrain.result().view(np.uint32).reshape(h, w), level.result().reshape(h, w) if level else None,
            opened.result().view(np.uint32).reshape(h, w) if opened else None)


def assert_bits(got, want, what):
    ne = got != want
    assert not ne.any(), "%s: differs at %d cells, first (y, x) %s: %08x, not %08x" % (
        what, int(ne.sum()), tuple(np.argwhere(ne)[0]), int(got[ne][0]), int(want[ne][0]))


def check_morphology(capi, name, a, radii):
    h, w = a.shape
    bits, in_d = R.bits_of(a), map_d(a)
    for radius in radii:
        for op in OPS:
            want = R.morphology_bits(bits, radius, op)
            first = morphology_call(capi, in_d, w, h, radius, op, 0xFF)
            assert_bits(first, want, "%s %d x %d radius %d op %d" % (name, w, h, radius, op))
            assert np.array_equal(first, morphology_call(capi, in_d, w, h, radius, op, 0x00)), (name, w, h, radius, op)
    assert np.array_equal(in_d.cpu().numpy().view(np.uint32), bits)            # the input is left alone


def check_terrain(capi, name, a, params=C.TERRAIN_PARAMS):
    h, w = a.shape
    in_d = map_d(a)
    for radii, thresholds in params:
        want = R.terrain(a, radii, thresholds)
        what = "%s %d x %d radii %s" % (name, w, h, radii)
        first = terrain_call(capi, in_d, w, h, radii, thresholds, 0xFF)
        assert_bits(first[0], R.bits_of(want["terrain"]), what + " terrain")
        assert_bits(first[1], want["level"], what + " level")
        assert_bits(first[2], R.bits_of(want["opened"]), what + " opened")
        again = terrain_call(capi, in_d, w, h, radii, thresholds, 0x00)
        assert all(np.array_equal(x, y) for x, y in zip(first, again)), what
        for want_level, want_opened in ((False, False), (True, False), (False, True)):
            part = terrain_call(capi, in_d, w, h, radii, thresholds, 0xFF, want_level, want_opened)
            assert np.array_equal(part[0], first[0]), what
            assert part[1] is None if not want_level else np.array_equal(part[1], first[1]), what
            assert part[2] is None if not want_opened else np.array_equal(part[2], first[2]), what


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_morphology_equals_the_restatement(capi, size):
    w, h = size
    for name, a in C.maps(w, h):
        check_morphology(capi, name, a, C.radii_of(size))


@pytest.mark.parametrize("size", C.BOUNDARY_SIZES, ids=lambda s: "%dx%d" % s)
def test_morphology_at_the_kernels_own_boundaries(capi, size):
    """255, 256 and 257 (above) columns: one block of columns and the next; 65535 and 65536 segments of 3 rows a column and 200 000
    rows: the grid of segments is 65535 high and walks the rest in strides"""
    w, h = size
    for name in ("noise", "holes5", "hard"):
        check_morphology(capi, name, C.CONTENTS[name](w, h), C.BOUNDARY_RADII)


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_terrain_equals_the_restatement(capi, size):
    w, h = size
    for name, a in C.maps(w, h):
        check_terrain(capi, name, a)


def test_subtract_equals_the_restatement_also_in_place(capi):
    for w, h in C.SIZES:
        a, b = C.subtract_pair(w, h)
        want = R.bits_of(R.subtract(a, b))
        a_d, b_d, out = map_d(a), map_d(b), Guarded(w * h)
        capi.check(capi.LIB.ssrlcv_hip_dsm_subtract(vp(a_d.data_ptr()), vp(b_d.data_ptr()), u32(w), u32(h), out.ptr, capi.stream_ptr()))
        assert_bits(out.result().view(np.uint32).reshape(h, w), want, "subtract %d x %d" % (w, h))
        if w >= 4:
            assert want[0, 0] == want[0, 1] == want[0, 3] == R.INVALID and want[0, 2] == 0x7F800000   # inf - inf does not reach the map
        for alias in (0, 1):                                                    # out == a, then out == b
            x_d, y_d = map_d(a), map_d(b)
            res = capi.dsm_subtract(x_d, y_d, out=(x_d, y_d)[alias])
            assert res is (x_d, y_d)[alias]
            assert_bits(res.cpu().numpy().view(np.uint32), want, "subtract %d x %d onto input %d" % (w, h, alias))
            assert np.array_equal((y_d, x_d)[alias].cpu().numpy().view(np.uint32), R.bits_of((b, a)[alias]))
        assert np.array_equal(capi.dsm_subtract(a_d, b_d).cpu().numpy().view(np.uint32), want)


def test_the_binders_and_an_empty_map(capi):
    a = C.holes5(65, 33)
    a_d = map_d(a)
    assert np.array_equal(capi.dsm_morphology(a_d, 3, capi.MORPH_OPEN).cpu().numpy().view(np.uint32), R.morphology_bits(R.bits_of(a), 3, R.OPEN))
    ws = capi.dev_bytes(4 * a256(4 * 65 * 33))
    out = torch.empty_like(a_d)
    assert capi.dsm_morphology(a_d, capi.MORPH_WHOLE_MAP, capi.MORPH_DILATE, out=out, workspace=ws) is out
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.morphology_bits(R.bits_of(a), C.UINT32_MAX, R.DILATE))
    radii, thresholds = C.TERRAIN_PARAMS[1]
    want = R.terrain(a, radii, thresholds)
    terrain, level, opened = capi.dsm_terrain(a_d, radii, thresholds, want_opened=True, workspace=ws)
    assert np.array_equal(terrain.cpu().numpy().view(np.uint32), R.bits_of(want["terrain"]))
    assert np.array_equal(level.cpu().numpy(), want["level"]) and np.array_equal(opened.cpu().numpy().view(np.uint32), R.bits_of(want["opened"]))
    assert capi.dsm_terrain(a_d, radii, thresholds, want_level=False)[1:] == (None, None)
    for w, h in ((0, 5), (5, 0), (0, 0)):                                          # nothing is looked at
        capi.check(capi.LIB.ssrlcv_hip_dsm_morphology(vp(0), vp(0), u32(w), u32(h), u32(2), u32(0), vp(0), csz(0), capi.stream_ptr()))
        p = capi.TerrainParams(1, (u32 * 8)(1), (ctypes.c_float * 8)(0.5))
        capi.check(capi.LIB.ssrlcv_hip_dsm_terrain(vp(0), u32(w), u32(h), ctypes.byref(p), vp(0), vp(0), vp(0), vp(0), csz(0), capi.stream_ptr()))
        capi.check(capi.LIB.ssrlcv_hip_dsm_subtract(vp(0), vp(0), u32(w), u32(h), vp(0), capi.stream_ptr()))


def test_the_boxed_scene_through_the_pipeline_and_the_class_api(capi, tmp_path):
    """pipeline.surface_terrain on the boxed scene map of tests/test_terrain_cases.py: level, bare and objects equal the
    restatement, terrain is bare through the fill's restatement, the object heights are what was built, and
    MeshFactory::extractTerrain + objectHeights on the same raw files give the same counts and maps"""
    import dsm_cases as DC
    import fill_ref as F
    from ssrlcv_amd import pipeline
    s = C.scene()
    height = s["height"]
    h, w = height.shape
    fr = DC.axis_frame(w, h, cell=1.0)
    got = pipeline.surface_terrain(map_d(height), cframe(capi, fr), **{k: v for k, v in C.SCHEDULE.items() if k != "cell"})
    radii, thresholds = R.schedule(**C.SCHEDULE)
    assert got["radii"] == list(radii) and got["thresholds"] == [float(t) for t in thresholds]
    want = R.terrain(height, radii, thresholds)
    assert np.array_equal(got["level"].cpu().numpy(), want["level"])
    assert np.array_equal(got["bare"].cpu().numpy().view(np.uint32), R.bits_of(want["terrain"]))
    assert np.array_equal(got["ground"].cpu().numpy(), want["level"] == 0)
    filled = F.fill(want["terrain"], 0xFF, F.NO_LIMIT, 1, F.MEDIAN)[0]
    assert np.array_equal(got["terrain"].cpu().numpy().view(np.uint32), R.bits_of(filled))
    objects = got["objects"].cpu().numpy()
    assert np.array_equal(objects.view(np.uint32), R.bits_of(R.subtract(height, filled)))
    relief = np.float32(0.3)
    assert (np.abs(objects[s["ground"]]) <= relief).all()
    assert (objects[s["box"]] >= s["top"][s["box"]] - relief).all()
    flagged = want["level"] != 0
    counts = (int(flagged.sum()), int((~flagged).sum()), int((flagged & s["box"]).sum()))
    print("boxed scene %d x %d: %d cells flagged (%d of %d box cells), %d ground; object heights on the ground within %.3f, on the boxes at least top - %.3f"
          % (w, h, counts[0], counts[2], int(s["box"].sum()), counts[1], float(np.abs(objects[s["ground"]]).max()),
             float((s["top"][s["box"]] - objects[s["box"]]).max())))
    stats = pipeline.difference_stats(got["objects"])                              # the form the statistics take as it is
    assert stats["finite"] == w * h
    # the class API
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/terrain_test"])
    height_path = str(tmp_path / "height.raw")
    height.tofile(height_path)
    out = subprocess.check_output([os.path.join(host, "_build", "terrain_test"), str(w), str(h), height_path, "1", "8", "0.3", "0.5", "1.5",
                                   str(tmp_path) + os.sep], timeout=120).decode()
    lines = out.splitlines()
    assert lines[-1] == "ok", out
    assert "flagged %d ground %d invalid 0" % counts[:2] in lines, out
    assert np.array_equal(np.fromfile(str(tmp_path / "level.raw"), np.uint8).reshape(h, w), want["level"])
    assert np.array_equal(np.fromfile(str(tmp_path / "bare.raw"), np.uint32).reshape(h, w), R.bits_of(want["terrain"]))
    assert np.array_equal(np.fromfile(str(tmp_path / "terrain.raw"), np.uint32).reshape(h, w), R.bits_of(filled))
    assert np.array_equal(np.fromfile(str(tmp_path / "objects.raw"), np.uint32).reshape(h, w), objects.view(np.uint32))
