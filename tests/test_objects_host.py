"""Surface objects, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "surface objects" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace query follows the header's formula, the structures have
the header's sizes, ssrlcv_object_measures_host equals the numpy float64 restatement bit for bit, and the C++ mirror program
compiles."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import objects_ref as R

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERY = "ssrlcv_hip_dsm_objects_workspace_bytes"
NAMES = [QUERY, "ssrlcv_hip_dsm_objects", "ssrlcv_object_measures_host"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x1000  # a "device pointer" nothing may dereference
INF, NAN = float("inf"), float("nan")


class Params(ctypes.Structure):
    _fields_ = [("minHeight", f32), ("maxDiff", f32), ("scale", f32), ("minCells", u32)]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, QUERY).restype = csz
    return lb


def a256(n):
    return (n + 255) // 256 * 256


def formula(w, h):
    """3 a256(4 w h) + c(w h), c(N) = a256(4 (4 ceil(N / 4096) + 3))"""
    n = w * h
    return 3 * a256(4 * n) + a256(4 * (4 * ((n + 4095) // 4096) + 3))


def call(lib, w=64, h=48, p="default", objects=BOGUS, ids=BOGUS + 0x1000, records=BOGUS + 0x2000, capacity=4, count=BOGUS + 0x3000, ws=BOGUS + 0x4000,
         ws_bytes=1 << 50):
    p = Params(1.0, INF, 256.0, 1) if p == "default" else p
    return lib.ssrlcv_hip_dsm_objects(vp(objects), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(ids), vp(records), u32(capacity),
                                      vp(count), vp(ws), csz(ws_bytes), vp(None))


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    assert QUERY in inspect.getsource(_lib.load)                                     # among the c_size_t queries
    subtract_at, at, end = header.index("int ssrlcv_hip_dsm_subtract("), header.index("---- surface objects"), header.index("int ssrlcv_sift_plan_overflow")
    assert header.index("---- terrain filter") < subtract_at < at < end             # directly behind "terrain filter", before the overflow section
    assert "/* ----" not in header[header.index(";", subtract_at):at] and "/* ----" not in header[at + 10:end]
    assert "surface objects: dsm_objects (+ its workspace query), object_measures_host" in header[:at]   # the list of additions
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header     # additions keep the number
    section = re.sub(r"\n \*\s+", " ", header[at:end])
    for text in ("0x7FC00000", "v >= minHeight in float32", "+inf is a member", "never a member", "4-connectivity", "smallest raster index",
                 "Two +inf cells do not link", "minCells = 0 behaves as 1", "ascending label", "the full number kept", "min(count, capacity)",
                 "nothing behind records[capacity) is touched", "ssrlcv_hip_stereo_matches", "every entry is written", "UINT32_MAX",
                 "do not depend on capacity", "-0 < +0", "fabsf(t) <= 65536.0f", "(int32)rintf(t)", "in nothing below", "w, h <= 65536 and w h <= 2^30",
                 "< 2^46", "< 2^62", "2^31 + 2", "12.566370614359172", "no libm call", "a NaN (0 / 0)", "is not refused",
                 "3 a256(4 w h) + c(w h)", "It may hold anything on entry", "no host synchronisation", "no block waits for another",
                 "integer atomics only", "bit-equal run to run", "is never touched", "16 bytes", "104 bytes", "152 bytes"):
        assert text in section, text
    scope = section[section.index("Out of scope:"):]
    for text in ("8-connectivity", "polygons", "medians", "building or vegetation", "objects of a cloud", "mosaic"):
        assert text in scope, text
    assert ctypes.sizeof(Params) == 16 == ctypes.sizeof(capi.ObjectParams) and ctypes.sizeof(capi.ObjectRecord) == 104 == R.RECORD.itemsize
    assert capi.OBJECT_RECORD == R.RECORD and [n for n, _ in capi.ObjectRecord._fields_] == list(R.RECORD.names)
    assert [(n, capi.OBJECT_RECORD.fields[n][1]) for n in R.RECORD.names] == [(n, getattr(capi.ObjectRecord, n).offset) for n in R.RECORD.names]
    assert ctypes.sizeof(capi.ObjectMeasures) == 152 == 8 * len(R.MEASURES)
    sig = inspect.signature
    assert list(sig(pipeline.surface_objects).parameters) == ["terrain_or_objects", "frame", "min_height", "max_diff", "min_cells", "scale"]
    defaults = {k: v.default for k, v in sig(pipeline.surface_objects).parameters.items()}
    assert (defaults["max_diff"], defaults["min_cells"], defaults["scale"]) == (INF, 1, 256.0)
    assert list(sig(capi.dsm_objects).parameters)[:5] == ["objects_d", "min_height", "max_diff", "min_cells", "scale"]
    assert list(sig(capi.object_measures).parameters) == ["record", "frame", "scale"]
    assert list(sig(pipeline.surface_terrain).parameters)[:2] == ["model_or_height", "frame"]   # unchanged


def test_refusals_in_the_contract_s_order(lib):
    bad = [None, Params(NAN, INF, 256.0, 1), Params(1.0, NAN, 256.0, 1), Params(1.0, -0.5, 256.0, 1), Params(1.0, -INF, 256.0, 1), Params(1.0, 1.0, 0.0, 1),
           Params(1.0, 1.0, -1.0, 1), Params(1.0, 1.0, INF, 1), Params(1.0, 1.0, NAN, 1)]
    for p in bad:                                                                    # the parameters before everything
        assert call(lib, p=p) == INVALID_ARG
        assert call(lib, p=p, w=65537, h=1) == INVALID_ARG and call(lib, p=p, count=None) == INVALID_ARG
        assert call(lib, p=p, w=0, objects=None, ws=None) == INVALID_ARG
    for w, h in ((65537, 1), (1, 65537), (65536, 16385), (32769, 32768), (0xFFFFFFFF, 0xFFFFFFFF), (65537, 0)):   # then the limits
        assert call(lib, w=w, h=h) == UNSUPPORTED, (w, h)
        assert call(lib, w=w, h=h, count=None, objects=None, ws=None) == UNSUPPORTED, (w, h)
    assert call(lib, count=None) == INVALID_ARG and call(lib, w=0, count=None) == INVALID_ARG   # then the count, also of an empty map
    for null in ("objects", "ws"):                                                   # then the buffers
        assert call(lib, **{null: None}) == INVALID_ARG, null
        assert call(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null            # a NULL buffer before a short workspace
    assert call(lib, records=None, capacity=1) == INVALID_ARG and call(lib, records=None, capacity=1, ws_bytes=0) == INVALID_ARG
    assert call(lib, records=BOGUS + 4) == INVALID_ARG                               # the 64-bit sums are added in place
    want = lib.ssrlcv_hip_dsm_objects_workspace_bytes(u32(64), u32(48))
    assert want == formula(64, 48)
    assert call(lib, ws_bytes=want - 1) == WORKSPACE and call(lib, ws_bytes=0) == WORKSPACE
    legal = [dict(ids=None), dict(records=None, capacity=0), dict(ids=None, records=None, capacity=0), dict(p=Params(-INF, 0.0, 1e-30, 0)),
             dict(p=Params(INF, INF, 3.4e38, 0xFFFFFFFF)), dict(p=Params(-0.0, 0.0, 1.0, 7)), dict(w=1, h=1), dict(w=65536, h=16384), dict(w=16384, h=65536),
             dict(capacity=0xFFFFFFFF)]
    for kw in legal:
        assert call(lib, ws_bytes=0, **kw) == WORKSPACE, kw                           # accepted up to the size check


def test_the_workspace_query_follows_the_header(lib):
    for (w, h) in ((1, 1), (2, 2), (63, 5), (64, 16), (257, 131), (4096, 4096), (65536, 16384), (1 << 14, 1 << 16), (1, 65536), (32768, 32768)):
        assert lib.ssrlcv_hip_dsm_objects_workspace_bytes(u32(w), u32(h)) == formula(w, h), (w, h)
    for (w, h) in ((65537, 1), (1, 65537), (32769, 32768), (0, 9), (9, 0), (0, 0), (1 << 31, 2)):
        assert lib.ssrlcv_hip_dsm_objects_workspace_bytes(u32(w), u32(h)) == 0, (w, h)


# ---- the measures
def record(**fields):
    r = np.zeros(1, R.RECORD)
    for k, v in fields.items():
        if k in ("peak", "low"):
            r[k] = np.float32(v)
        else:
            r[k] = v
    return r[0]


def from_cells(cells, q=None, clipped=0):
    """the record of a hand-written list of (x, y) cells, perimeter counted, q the quantised heights of the cells that take part"""
    own = set(cells)
    xs, ys = [x for x, _ in cells], [y for _, y in cells]
    q = [0] * (len(cells) - clipped) if q is None else q
    perimeter = sum((x + dx, y + dy) not in own for x, y in cells for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))
    return record(label=0, cells=len(cells), minX=min(xs), minY=min(ys), maxX=max(xs), maxY=max(ys), perimeter=perimeter, clipped=clipped,
                  sumX=sum(xs), sumY=sum(ys), sumXX=sum(x * x for x in xs), sumXY=sum(x * y for x, y in cells), sumYY=sum(y * y for y in ys),
                  sumQ=sum(q), sumQQ=sum(v * v for v in q))


HAND = {
    "one cell": from_cells([(5, 7)], q=[640]),
    "one cell at the origin": from_cells([(0, 0)], q=[-3]),
    "a row of cells": from_cells([(x, 9) for x in range(3, 40)], q=list(range(100, 137))),
    "a column of cells": from_cells([(11, y) for y in range(2, 9)], q=[512] * 7),
    "a diagonal staircase": from_cells([(k + d, k) for k in range(12) for d in (0, 1)], q=[7 * k for k in range(24)]),
    "a descending staircase": from_cells([(20 - k + d, k) for k in range(12) for d in (0, 1)], q=[-5 * k for k in range(24)]),
    "a square": from_cells([(x, y) for y in range(30, 46) for x in range(60, 76)], q=[1536] * 256),
    "a plus": from_cells([(10, 10), (9, 10), (11, 10), (10, 9), (10, 11)], q=[256, 257, 255, 1000, -1000]),
    "every cell clipped": from_cells([(3, 3), (4, 3)], clipped=2),
    "one cell left": from_cells([(3, 3), (4, 3), (4, 4)], q=[65536], clipped=2),
    "far corner, large sums": record(label=7, cells=1 << 30, minX=0, minY=0, maxX=65535, maxY=16383, perimeter=2 * (65536 + 16384), clipped=12345,
                                     sumX=(1 << 30) * 65535 // 2, sumY=(1 << 30) * 16383 // 2, sumXX=(1 << 61) + 12345, sumXY=(1 << 60) + 7,
                                     sumYY=(1 << 59) + 1, sumQ=-(1 << 45) - 3, sumQQ=(1 << 62) - 1),
}
FRAMES = {"unit": R.Frame(), "skew": R.Frame(origin=(-3.3, 2.1, 0.7), ex=(1, 0.25, 0), ey=(0.1, 1, 0.05), ez=(0.2, -0.1, 1), cell=0.37, w=9, h=9)}


def measures_c(capi, rec, frame, scale):
    fr = capi.DsmFrame.make(frame.origin, frame.ex, frame.ey, frame.ez, frame.cell, frame.w, frame.h)
    m = capi.object_measures(rec, fr, scale)
    values = [getattr(m, n) for n in R.MEASURES[:5]] + list(m.world) + [getattr(m, n) for n in R.MEASURES[8:]]
    return np.array(values, np.float64)


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_measures_equal_the_float64_restatement_bit_for_bit(name):
    from ssrlcv_amd import capi
    for frame_name, frame in FRAMES.items():
        for scale in (256.0, 1.0, 0.3):
            want = R.measures(HAND[name], frame, scale)
            got = measures_c(capi, HAND[name], frame, scale)
            want_bits = np.array([want[n] for n in R.MEASURES], np.float64).view(np.uint64)
            ne = got.view(np.uint64) != want_bits
            assert not ne.any(), (name, frame_name, scale, [(R.MEASURES[i], got[i], want[R.MEASURES[i]]) for i in np.nonzero(ne)[0]])


def test_the_measures_of_hand_records():
    unit = FRAMES["unit"]
    m = R.measures(HAND["one cell"], unit, 256.0)
    assert (m["area"], m["perimeterLength"], m["centroidX"], m["centroidY"], m["meanHeight"], m["volume"], m["rmsHeight"]) == (1, 4, 5, 7, 2.5, 2.5, 0)
    assert (m["mxx"], m["mxy"], m["myy"], m["lambdaMajor"], m["lambdaMinor"], m["axisX"], m["axisY"], m["elongation"]) == (0, 0, 0, 0, 0, 1, 0, 1)
    assert (m["world0"], m["world1"], m["world2"]) == (5.5, 7.5, 0) and abs(m["compactness"] - np.pi / 4) < 1e-15
    m = R.measures(HAND["a row of cells"], unit, 256.0)
    assert m["myy"] == 0 and m["mxx"] == (37 * 37 - 1) / 12 and m["axisX"] == 1 and m["axisY"] == 0 and m["elongation"] > 1e6
    m = R.measures(HAND["a column of cells"], unit, 256.0)
    assert m["mxx"] == 0 and m["myy"] == 4 and (m["axisX"], m["axisY"]) == (0, 1) and m["elongation"] == np.inf and m["rmsHeight"] == 0
    m = R.measures(HAND["a square"], unit, 256.0)
    assert m["mxx"] == m["myy"] == (256 - 1) / 12 and m["mxy"] == 0 and (m["axisX"], m["axisY"], m["elongation"]) == (1, 0, 1) and m["volume"] == 6 * 256
    up, down = R.measures(HAND["a diagonal staircase"], unit, 256.0), R.measures(HAND["a descending staircase"], unit, 256.0)
    assert up["axisX"] > 0 and up["axisY"] > 0 and down["axisX"] > 0 and down["axisY"] < 0
    assert abs(np.hypot(up["axisX"], up["axisY"]) - 1) < 1e-15 and up["lambdaMajor"] > up["lambdaMinor"] > 0
    m = R.measures(HAND["every cell clipped"], unit, 256.0)
    assert np.isnan(m["meanHeight"]) and np.isnan(m["rmsHeight"]) and m["volume"] == 0 and m["area"] == 2   # not refused
    m = R.measures(HAND["one cell left"], unit, 256.0)
    assert (m["meanHeight"], m["rmsHeight"], m["volume"]) == (256, 0, 256)
    m = R.measures(HAND["a plus"], FRAMES["skew"], 256.0)
    assert m["area"] == 5 * (np.float64(np.float32(0.37)) ** 2) and m["mxy"] == 0 and m["rmsHeight"] > 0


def test_the_measures_refusals(lib):
    from ssrlcv_amd import capi
    rec = capi.ObjectRecord.from_buffer_copy(np.asarray(HAND["a plus"], R.RECORD).reshape(1).tobytes())
    fr = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 4, 4)
    out = capi.ObjectMeasures()
    fn = lib.ssrlcv_object_measures_host
    assert fn(ctypes.byref(rec), ctypes.byref(fr), f32(256.0), ctypes.byref(out)) == OK and out.area == 5.0
    assert fn(None, ctypes.byref(fr), f32(256.0), ctypes.byref(out)) == INVALID_ARG
    assert fn(ctypes.byref(rec), None, f32(256.0), ctypes.byref(out)) == INVALID_ARG
    assert fn(ctypes.byref(rec), ctypes.byref(fr), f32(256.0), None) == INVALID_ARG
    for scale in (0.0, -1.0, INF, NAN):
        assert fn(ctypes.byref(rec), ctypes.byref(fr), f32(scale), ctypes.byref(out)) == INVALID_ARG
    for cell in (0.0, -1.0, INF, NAN):
        bad = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 4, 4)
        bad.cell = cell
        assert fn(ctypes.byref(rec), ctypes.byref(bad), f32(256.0), ctypes.byref(out)) == INVALID_ARG
    empty = capi.ObjectRecord()
    assert fn(ctypes.byref(empty), ctypes.byref(fr), f32(256.0), ctypes.byref(out)) == INVALID_ARG
    rec.clipped = rec.cells + 1
    assert fn(ctypes.byref(rec), ctypes.byref(fr), f32(256.0), ctypes.byref(out)) == INVALID_ARG
    assert out.area == 5.0                                                          # untouched on error


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/objects_test"])
    r = subprocess.run([os.path.join(host, "_build", "objects_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("static bool extractObjects(", "static bool objectMeasures(", "ssrlcv_hip_dsm_objects(", "ssrlcv_hip_dsm_objects_workspace_bytes(",
                   "ssrlcv_object_measures_host("):
        assert member in factory, member
    assert "objects_test" in open(os.path.join(host, "Makefile")).read()


def test_the_library_has_one_path_and_the_documents_exist():
    root = H.ROOT
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "objects.hip")).read()
    assert "getenv" not in source and "svdev::" not in source                      # no developer switch
    assert "svcc::label_components(" in source and "k_cc_tile<<<" not in source and "void k_cc_tile(" not in source   # the labelling is called, not copied
    assert not re.search(r"atomic(Add|Max|Min)\s*\(\s*\(?float", source) and "atomicAdd_f" not in source and "unsafeAtomicAdd" not in source
    assert "objects.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_dsm_objects" in open(os.path.join(root, doc)).read(), doc
    assert "objects_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    for tool in ("bench_objects.py", "objects_lab.hip"):
        assert os.path.exists(os.path.join(root, "tools", tool)) and tool in open(os.path.join(root, "tools", "README.md")).read()
