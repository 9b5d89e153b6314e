"""The surface model, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "surface model" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace queries follow the header's formulas, the C++ mirror
program compiles, and the documents and the bench tool exist."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERIES = ["ssrlcv_hip_dsm_rasterize_workspace_bytes", "ssrlcv_hip_dsm_points_workspace_bytes"]
NAMES = QUERIES + ["ssrlcv_hip_dsm_rasterize", "ssrlcv_hip_dsm_fuse", "ssrlcv_hip_dsm_points"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    for name in QUERIES:
        getattr(lb, name).restype = csz
    return lb


def a256(n):
    return (n + 255) // 256 * 256


def compaction(n):
    """the header's c(N)"""
    return a256(4 * (4 * ((n + 4095) // 4096) + 3))


def frame(w=64, h=48, cell=0.5, origin=(1, 2, 3), ex=(1, 0, 0), ey=(0, 1, 0), ez=(0, 0, 1)):
    from ssrlcv_amd import capi
    return capi.DsmFrame.make(origin, ex, ey, ez, cell, w, h)


def rasterize(lib, fr=True, n=1000, rule=0, points=BOGUS, height=BOGUS + 0x1000, source=BOGUS + 0x2000, count=BOGUS + 0x3000, ws=BOGUS + 0x4000,
              ws_bytes=1 << 50, **frame_args):
    f = ctypes.byref(frame(**frame_args)) if fr else None
    return lib.ssrlcv_hip_dsm_rasterize(vp(points), u32(n), f, u32(rule), vp(height), vp(source), vp(count), vp(ws), csz(ws_bytes), vp(None))


def fuse(lib, m=3, w=64, h=48, min_views=1, max_spread=1.0, rule=1, maps=True, entries=None, out=BOGUS + 0x9000, views=BOGUS + 0xA000):
    entries = [BOGUS + 0x1000 * k for k in range(max(m, 1))] if entries is None else entries
    arr = (vp * len(entries))(*entries) if maps else None
    return lib.ssrlcv_hip_dsm_fuse(arr, u32(m), u32(w), u32(h), u32(min_views), f32(max_spread), u32(rule), vp(out), vp(views), vp(None))


def points(lib, fr=True, height=BOGUS, out=BOGUS + 0x1000, cap=100, count=BOGUS + 0x2000, ws=BOGUS + 0x3000, ws_bytes=1 << 50, **frame_args):
    f = ctypes.byref(frame(**frame_args)) if fr else None
    return lib.ssrlcv_hip_dsm_points(vp(height), f, vp(out), u32(cap), vp(count), vp(ws), csz(ws_bytes), vp(None))


BAD_FRAMES = [dict(fr=False), dict(cell=0.0), dict(cell=-1.0), dict(cell=NAN), dict(cell=INF), dict(origin=(NAN, 0, 0)), dict(ex=(0, INF, 0)),
              dict(ey=(0, 0, -INF)), dict(ez=(NAN, NAN, NAN))]


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    normals_at, dsm_at = header.index("int ssrlcv_hip_mesh_normals("), header.index("---- surface model")
    assert normals_at < dsm_at < header.index("int ssrlcv_sift_plan_overflow")   # behind the mesh, before the overflow section
    assert "next section" in header[normals_at:dsm_at]                           # the mesh section points to it
    section = re.sub(r"\n \*\s+", " ", header[dsm_at:header.index("int ssrlcv_sift_plan_overflow")])
    for text in ("0x7FC00000", "NOT checked for orthonormality", "either sign of zero", "floorf(u)", "before any conversion", "-0 is inside cell 0",
                 "u == w is outside", "the smallest index", "UINT32_MAX and 0", "HOST array of m device pointers", "hi - lo <= maxSpread",
                 "always one of the inputs", "raster order", "truncation contract", "right-handed", "face +ez", "a256(8 w h)", "c(w h)",
                 "INTEGER atomics only", "bit-equal run to run", "float accumulation", "ortho-image", "pushbroom", "more than 8 maps",
                 "ssrlcv_dsm_frame; /* 60 bytes */"):
        assert text in section, text
    assert ctypes.sizeof(capi.DsmFrame) == 60 and _lib.ABI_VERSION == 4
    sig = inspect.signature
    assert list(sig(capi.dsm_rasterize).parameters)[:5] == ["points_d", "frame", "rule", "want_source", "want_count"]
    assert list(sig(capi.dsm_fuse).parameters) == ["maps", "min_views", "max_spread", "rule", "want_views"]
    assert list(sig(capi.dsm_points).parameters) == ["height_d", "frame", "capacity"]
    assert list(sig(pipeline.dsm_frame).parameters) == ["points", "up", "cell", "margin", "ex"] and sig(pipeline.dsm_frame).parameters["margin"].default == 0
    assert list(sig(pipeline.surface_model).parameters) == ["clouds", "frame", "rule", "fuse", "post"]
    assert list(sig(pipeline.surface_mesh).parameters) == ["model", "frame", "max_jump"]
    with pytest.raises(ValueError):
        pipeline.surface_model([], None, rule="mean")                             # before anything is touched
    with pytest.raises(TypeError):
        pipeline.surface_model([], None, fuse=dict(spread=1))


def test_rasterize_refusals_in_the_contract_s_order(lib):
    for bad in BAD_FRAMES + [dict(rule=2), dict(n=0xFFFFFFFF), dict(w=65536, h=32768)]:
        assert rasterize(lib, **bad) == INVALID_ARG, bad
        assert rasterize(lib, height=None, ws=None, ws_bytes=0, **bad) == INVALID_ARG, bad
    assert rasterize(lib, w=(1 << 24) + 1, h=1, rule=2) == INVALID_ARG            # a parameter before the size
    assert rasterize(lib, w=(1 << 24) + 1, h=1) == UNSUPPORTED and rasterize(lib, w=1, h=(1 << 24) + 1, height=None) == UNSUPPORTED
    assert rasterize(lib, w=(1 << 24) + 1, h=0) == UNSUPPORTED                    # the size before the empty grid
    assert rasterize(lib, w=(1 << 24) + 1, h=1 << 10) == INVALID_ARG              # w h >= 2^31 first
    for empty in (dict(w=0), dict(h=0)):                                          # an empty grid: nothing is looked at
        assert rasterize(lib, points=None, height=None, source=None, count=None, ws=None, ws_bytes=0, **empty) == OK
    for null in ("height", "ws", "points"):
        assert rasterize(lib, **{null: None}) == INVALID_ARG, null
        assert rasterize(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null    # a NULL buffer before a short workspace
    want = lib.ssrlcv_hip_dsm_rasterize_workspace_bytes(u32(64), u32(48))
    assert want == a256(8 * 64 * 48)
    assert rasterize(lib, ws_bytes=want - 1) == WORKSPACE and rasterize(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(source=None), dict(count=None), dict(n=0, points=None), dict(rule=1), dict(w=1 << 24, h=1), dict(w=65536, h=32767),
                  dict(ex=(1, 1, 1), ey=(1, 1, 1), ez=(0, 0, 0)), dict(cell=1e-45), dict(n=0xFFFFFFFE)):
        assert rasterize(lib, ws_bytes=0, **legal) == WORKSPACE, legal            # accepted up to the size check


def test_fuse_refusals_in_the_contract_s_order(lib):
    for bad in (dict(m=0), dict(m=9), dict(min_views=0), dict(min_views=4), dict(max_spread=-1.0), dict(max_spread=-1e-45), dict(max_spread=NAN),
                dict(max_spread=-INF), dict(rule=3), dict(w=65536, h=32768)):
        assert fuse(lib, **bad) == INVALID_ARG, bad
        assert fuse(lib, maps=False, out=None, **bad) == INVALID_ARG, bad
    assert fuse(lib, w=0, maps=False, out=None) == OK and fuse(lib, h=0, maps=False, out=None) == OK
    assert fuse(lib, maps=False) == INVALID_ARG and fuse(lib, out=None) == INVALID_ARG
    assert fuse(lib, entries=[BOGUS, 0, BOGUS + 0x1000]) == INVALID_ARG           # a NULL maps[i]
    for k in range(3):                                                            # out equal to any input
        entries = [BOGUS, BOGUS + 0x1000, BOGUS + 0x2000]
        assert fuse(lib, entries=entries, out=entries[k]) == INVALID_ARG


def test_points_refusals_and_the_workspace_formulas(lib):
    for bad in BAD_FRAMES + [dict(w=65536, h=32768)]:
        assert points(lib, **bad) == INVALID_ARG, bad
        assert points(lib, count=None, height=None, **bad) == INVALID_ARG, bad
    assert points(lib, w=(1 << 24) + 1, h=1) == UNSUPPORTED and points(lib, w=(1 << 24) + 1, h=1, count=None) == UNSUPPORTED
    assert points(lib, count=None) == INVALID_ARG and points(lib, w=0, count=None) == INVALID_ARG   # an empty grid still needs the count
    for null in ("height", "ws", "out"):
        assert points(lib, **{null: None}) == INVALID_ARG, null
        assert points(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null
    want = lib.ssrlcv_hip_dsm_points_workspace_bytes(u32(64), u32(48))
    assert want == compaction(64 * 48)
    assert points(lib, ws_bytes=want - 1) == WORKSPACE and points(lib, out=None, cap=0, ws_bytes=0) == WORKSPACE
    ras, pts = lib.ssrlcv_hip_dsm_rasterize_workspace_bytes, lib.ssrlcv_hip_dsm_points_workspace_bytes
    for (w, h) in ((1, 1), (63, 5), (257, 131), (4096, 4096), (1 << 24, 1), (65536, 32767)):
        assert ras(u32(w), u32(h)) == a256(8 * w * h) and pts(u32(w), u32(h)) == compaction(w * h), (w, h)
    for (w, h) in ((65536, 32768), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        assert ras(u32(w), u32(h)) == 0 and pts(u32(w), u32(h)) == 0, (w, h)
    assert ras(u32(0), u32(9)) == 0 and pts(u32(0), u32(9)) == compaction(0)


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/dsm_test"])
    r = subprocess.run([os.path.join(host, "_build", "dsm_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("ptr::value<Unity<float>> generateHeightMap(const ssrlcv_dsm_frame& frame, unsigned int rule)", "static ptr::value<Unity<float>> fuseHeightMaps(",
                   "void setPointsFromHeightMap(ptr::value<Unity<float>> height, const ssrlcv_dsm_frame& frame)", "ssrlcv_hip_dsm_rasterize(",
                   "ssrlcv_hip_dsm_fuse(", "ssrlcv_hip_dsm_points("):
        assert member in factory, member


def test_the_documents_and_the_bench_tool_exist():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Surface model" in design
    for kernel in ("k_dsm_scatter", "k_dsm_unpack", "k_dsm_fuse"):
        assert kernel in design, kernel
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_dsm_rasterize" in open(os.path.join(root, doc)).read(), doc
    assert "dsm_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_dsm.py")) and os.path.exists(os.path.join(root, "profiles", "dsm_bench.txt"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "dsm.hip")).read()
    assert source.count("atomicMax(") == 1 and "#if" not in source                # one scatter form, not three
    assert "dsm.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
