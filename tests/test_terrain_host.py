"""The terrain filter, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "terrain filter" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace queries follow the header's formula, the schedule gives
the hand values, and the C++ mirror program compiles."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERIES = ["ssrlcv_hip_dsm_morphology_workspace_bytes", "ssrlcv_hip_dsm_terrain_workspace_bytes"]
NAMES = QUERIES + ["ssrlcv_hip_dsm_morphology", "ssrlcv_hip_dsm_terrain", "ssrlcv_hip_dsm_subtract"]
OK, INVALID_ARG, WORKSPACE = 0, -1, -3
BOGUS = 0x10  # a "device pointer" nothing may dereference
INF, NAN = float("inf"), float("nan")


class Params(ctypes.Structure):
    _fields_ = [("levels", u32), ("radius", u32 * 8), ("threshold", f32 * 8)]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    for q in QUERIES:
        getattr(lb, q).restype = csz
    return lb


def a256(n):
    return (n + 255) // 256 * 256


def params(radii=(1, 2, 4), thresholds=(0.5, 1.0, 1.5), levels=None):
    return Params(len(radii) if levels is None else levels, (u32 * 8)(*radii), (f32 * 8)(*thresholds))


def morphology(lib, w=64, h=48, radius=3, op=2, src=BOGUS, out=BOGUS + 0x1000, ws=BOGUS + 0x2000, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_dsm_morphology(vp(src), vp(out), u32(w), u32(h), u32(radius), u32(op), vp(ws), csz(ws_bytes), vp(None))


def terrain(lib, w=64, h=48, p="default", height=BOGUS, out=BOGUS + 0x1000, level=BOGUS + 0x2000, opened=BOGUS + 0x3000, ws=BOGUS + 0x4000,
            ws_bytes=1 << 50):
    p = params() if p == "default" else p
    return lib.ssrlcv_hip_dsm_terrain(vp(height), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(out), vp(level), vp(opened), vp(ws),
                                      csz(ws_bytes), vp(None))


def subtract(lib, w=64, h=48, a=BOGUS, b=BOGUS + 0x1000, out=BOGUS + 0x2000):
    return lib.ssrlcv_hip_dsm_subtract(vp(a), vp(b), u32(w), u32(h), vp(out), vp(None))


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    simplify_at, at = header.index("int ssrlcv_hip_dsm_simplify_mesh("), header.index("---- terrain filter")
    end = header.index("int ssrlcv_sift_plan_overflow")
    assert simplify_at < at < end                                                  # directly behind "surface simplification"
    assert "/* ----" not in header[header.index(";", simplify_at):at]
    section = re.sub(r"\n \*\s+", " ", header[at:end])
    for text in ("0x7FC00000", "k(f) = b >= 0 ? b : b ^ 0x7FFFFFFF", "-0 < +0", "equal keys are equal bits", "clipped at the image, never padded",
                 "min(radius, max(w, h) - 1)", "UINT32_MAX is legal", "radius == 0 is refused", "whether or not p itself is valid",
                 "O = DILATE(ERODE(in))", "holes stay holes", "k(O(p)) <= k(in(p))", "ERODE(DILATE(in))", "k(C(p)) >= k(in(p))", "in == out is refused",
                 "input bits or the invalid pattern", "Z_0 = height", "d > threshold[k-1]", "inf - inf flags nothing", "NaN bit patterns cannot leak",
                 "255 for an invalid input cell", "plateau of side >= 2 r_max + 1 is never flagged", "the method and not a defect",
                 "2 (r_1 + ... + r_K) cells from every border", "flags 1136 cells", "within 7 cells of a border", "stored as the invalid pattern",
                 "`out` may alias `a` or `b`", "ssrlcv_hip_difference_stats", "2 a256(4 w h)", "4 a256(4 w h)", "It may hold anything on entry",
                 "no atomics", "bit-equal run to run", "O(1) whatever the radius", "no loop has a trip count per cell that grows with the radius"):
        assert text in section, text
    scope = section[section.index("Out of scope:"):]
    for text in ("per-cell thresholds", "discs", "cloth-simulation", "TIN-densification", "interpolating the terrain", "pit removal", "points of a cloud",
                 "surface registration"):
        assert text in scope, text
    assert ctypes.sizeof(Params) == 68 == ctypes.sizeof(capi.TerrainParams) and "68 bytes" in header[at:end]
    assert _lib.ABI_VERSION == 4                                                   # additions keep the number
    assert (capi.MORPH_ERODE, capi.MORPH_DILATE, capi.MORPH_OPEN, capi.MORPH_CLOSE) == (0, 1, 2, 3)
    for k, name in enumerate(("ERODE", "DILATE", "OPEN", "CLOSE")):
        assert re.search(r"#define SSRLCV_MORPH_%s %d\b" % (name, k), header)
    sig = inspect.signature
    assert list(sig(capi.dsm_morphology).parameters) == ["height_d", "radius", "op", "out", "workspace"]
    assert list(sig(capi.dsm_terrain).parameters) == ["height_d", "radii", "thresholds", "want_level", "want_opened", "workspace"]
    assert list(sig(capi.dsm_subtract).parameters) == ["a_d", "b_d", "out"]
    assert list(sig(pipeline.terrain_schedule).parameters) == ["cell", "max_radius", "slope", "initial", "maximum", "radii"]
    assert list(sig(pipeline.surface_terrain).parameters) == ["model_or_height", "frame", "max_radius", "slope", "initial", "maximum", "radii", "fill",
                                                              "want_level"]
    assert sig(pipeline.surface_terrain).parameters["fill"].default == dict(paths=0xFF, max_gap=None, min_hits=1, rule="median")


def test_morphology_refusals_in_the_contract_s_order(lib):
    for bad in (dict(op=4), dict(op=0xFFFFFFFF), dict(radius=0)):
        assert morphology(lib, **bad) == INVALID_ARG
        assert morphology(lib, w=65536, h=32768, **bad) == INVALID_ARG and morphology(lib, w=0, src=None, **bad) == INVALID_ARG   # before everything
    assert morphology(lib, w=65536, h=32768) == INVALID_ARG and morphology(lib, w=65536, h=32768, src=None, ws=None) == INVALID_ARG
    assert morphology(lib, w=(1 << 31), h=0) == OK                                 # w h is 0: a size the limit takes
    for empty in (dict(w=0), dict(h=0)):
        assert morphology(lib, src=None, out=None, ws=None, ws_bytes=0, **empty) == OK
    for null in ("src", "out", "ws"):
        assert morphology(lib, **{null: None}) == INVALID_ARG, null
        assert morphology(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null    # a NULL buffer before a short workspace
    assert morphology(lib, out=BOGUS) == INVALID_ARG and morphology(lib, out=BOGUS, ws_bytes=0) == INVALID_ARG   # in == out
    want = lib.ssrlcv_hip_dsm_morphology_workspace_bytes(u32(64), u32(48))
    assert want == 2 * a256(4 * 64 * 48)
    assert morphology(lib, ws_bytes=want - 1) == WORKSPACE and morphology(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(radius=1), dict(radius=0xFFFFFFFF), dict(radius=1 << 31), dict(op=0), dict(op=1), dict(op=3), dict(w=1, h=1),
                  dict(w=32768, h=65535)):
        assert morphology(lib, ws_bytes=0, **legal) == WORKSPACE, legal             # accepted up to the size check


def test_terrain_refusals_in_the_contract_s_order(lib):
    bad = [None, params(levels=0), params(levels=9), params((0, 2, 4)), params((1, 1, 4)), params((1, 4, 2)), params((2, 3, 0)),
           params(thresholds=(0.5, -0.0001, 1.0)), params(thresholds=(NAN, 1.0, 1.0)), params(thresholds=(0.5, 1.0, INF)),
           params(thresholds=(0.5, 1.0, -INF))]
    for p in bad:
        assert terrain(lib, p=p) == INVALID_ARG
        assert terrain(lib, p=p, w=65536, h=32768) == INVALID_ARG and terrain(lib, p=p, w=0, height=None) == INVALID_ARG   # before everything
    assert terrain(lib, w=65536, h=32768) == INVALID_ARG and terrain(lib, w=65536, h=32768, height=None, ws=None) == INVALID_ARG
    for empty in (dict(w=0), dict(h=0)):
        assert terrain(lib, height=None, out=None, level=None, opened=None, ws=None, ws_bytes=0, **empty) == OK
    for null in ("height", "out", "ws"):
        assert terrain(lib, **{null: None}) == INVALID_ARG, null
        assert terrain(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null
    want = lib.ssrlcv_hip_dsm_terrain_workspace_bytes(u32(64), u32(48))
    assert want == 4 * a256(4 * 64 * 48)
    assert terrain(lib, ws_bytes=want - 1) == WORKSPACE and terrain(lib, ws_bytes=0) == WORKSPACE
    legal = [dict(level=None), dict(opened=None), dict(level=None, opened=None), dict(p=params((7,), (0.0,))), dict(p=params((1, 0xFFFFFFFF), (0.0, 3.4e38))),
             dict(p=params((1, 2, 3, 4, 5, 6, 7, 8), (0.0,) * 8)), dict(p=params((3, 2, 1), (1.0, -1.0, NAN), levels=1)),   # the rest is ignored
             dict(p=params(thresholds=(-0.0, 0.0, 0.0))), dict(w=1, h=1)]
    for kw in legal:
        assert terrain(lib, ws_bytes=0, **kw) == WORKSPACE, kw


def test_subtract_refusals(lib):
    assert subtract(lib, w=65536, h=32768) == INVALID_ARG and subtract(lib, w=65536, h=32768, a=None) == INVALID_ARG
    for empty in (dict(w=0), dict(h=0)):
        assert subtract(lib, a=None, b=None, out=None, **empty) == OK
    for null in ("a", "b", "out"):
        assert subtract(lib, **{null: None}) == INVALID_ARG, null


def test_the_workspace_queries_follow_the_header(lib):
    for (w, h) in ((1, 1), (2, 2), (63, 5), (257, 131), (4096, 4096), (1 << 30, 1), (1, (1 << 31) - 1), (32768, 65535)):
        assert lib.ssrlcv_hip_dsm_morphology_workspace_bytes(u32(w), u32(h)) == 2 * a256(4 * w * h), (w, h)
        assert lib.ssrlcv_hip_dsm_terrain_workspace_bytes(u32(w), u32(h)) == 4 * a256(4 * w * h), (w, h)
    for (w, h) in ((65536, 32768), (1 << 31, 1), (0, 9), (9, 0)):
        assert lib.ssrlcv_hip_dsm_morphology_workspace_bytes(u32(w), u32(h)) == 0, (w, h)
        assert lib.ssrlcv_hip_dsm_terrain_workspace_bytes(u32(w), u32(h)) == 0, (w, h)


def test_the_schedule_against_hand_values():
    from ssrlcv_amd import pipeline
    import terrain_ref as R
    f = lambda *v: [float(np.float32(x)) for x in v]  # noqa: E731
    assert pipeline.terrain_schedule(1, 8, 0.3, 0.5, 1.5) == ([1, 2, 4, 8], f(0.5, 1.1, 1.5, 1.5))     # 0.5 + 0.6, then 1.7 and 2.9 capped
    assert pipeline.terrain_schedule(0.5, 8, 0.3, 0.5, 10.0) == ([1, 2, 4, 8], f(0.5, 0.8, 1.1, 1.7))
    assert pipeline.terrain_schedule(2.0, 5, 0.1, 0.25, 9.0) == ([1, 2, 4, 5], f(0.25, 0.65, 1.05, 0.65))   # max_radius as the last entry
    assert pipeline.terrain_schedule(1, 1, 0.3, 0.5, 1.5) == ([1], f(0.5))
    assert pipeline.terrain_schedule(1, 128, 0.3, 0.5, 1e9)[0] == [1, 2, 4, 8, 16, 32, 64, 128]
    assert pipeline.terrain_schedule(1, 100, 0.3, 0.5, 1e9)[0] == [1, 2, 4, 8, 16, 32, 64, 100]
    assert pipeline.terrain_schedule(1.0, 0, 0.2, 0.5, 3.0, radii=(3, 10, 40)) == ([3, 10, 40], f(0.5, 3.0, 3.0))   # 0.5 + 2.8 capped
    for max_radius in (129, 200, 256, 1000):
        with pytest.raises(ValueError):
            pipeline.terrain_schedule(1, max_radius, 0.3, 0.5, 1.5)              # nine levels and more: the caller passes radii
    assert pipeline.terrain_schedule(1, 1000, 0.3, 0.5, 1.5, radii=(10, 100, 1000))[0] == [10, 100, 1000]
    for radii in ((), (0, 1), (2, 2), (4, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            pipeline.terrain_schedule(1, 8, 0.3, 0.5, 1.5, radii=radii)
    for args in (dict(cell=1, max_radius=8, slope=0.3, initial=0.5, maximum=1.5), dict(cell=0.37, max_radius=50, slope=0.15, initial=0.2, maximum=2.5)):
        radii, thresholds = R.schedule(**args)                                     # the tests' restatement says the same
        assert pipeline.terrain_schedule(**args) == (list(radii), [float(t) for t in thresholds])


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/terrain_test"])
    r = subprocess.run([os.path.join(host, "_build", "terrain_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("static bool terrainSchedule(", "static ptr::value<Unity<float>> morphology(", "static ptr::value<Unity<float>> extractTerrain(",
                   "static ptr::value<Unity<float>> objectHeights(", "ssrlcv_hip_dsm_morphology(", "ssrlcv_hip_dsm_terrain(", "ssrlcv_hip_dsm_subtract(",
                   "initial + slope * cell * 2.0 * (double)(radii[k] - radii[k - 1])"):
        assert member in factory, member


def test_the_library_has_one_path_and_the_documents_exist():
    root = H.ROOT
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "terrain.hip")).read()
    assert "getenv" not in source and "svdev::" not in source                      # no developer switch
    assert "atomic" not in source.replace("no atomics", "")                        # one writer a word
    assert "terrain.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_dsm_terrain" in open(os.path.join(root, doc)).read(), doc
    assert "terrain_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    for tool in ("bench_terrain.py", "terrain_lab.hip"):
        assert os.path.exists(os.path.join(root, "tools", tool)) and tool in open(os.path.join(root, "tools", "README.md")).read()
