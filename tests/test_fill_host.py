"""Hole filling, the part that needs no GPU: the header, the loader and the binders name the two entry points, every refusal
of include/ssrlcv_hip.h "hole filling" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace query follows the header's formula, and the C++
mirror program compiles."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H

u32, csz, vp = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p
NAMES = ["ssrlcv_hip_stereo_fill_holes_workspace_bytes", "ssrlcv_hip_stereo_fill_holes"]
OK, INVALID_ARG, WORKSPACE = 0, -1, -3
BOGUS = 0x10  # a "device pointer" nothing may dereference
NO_LIMIT = 0xFFFFFFFF


class Params(ctypes.Structure):
    _fields_ = [("paths", u32), ("maxGap", u32), ("minHits", u32), ("rule", u32)]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, NAMES[0]).restype = csz
    return lb


def fill(lib, w=64, h=48, paths=0xFF, max_gap=32, min_hits=5, rule=0, params=True, src=BOGUS, dst=BOGUS + 0x1000, mask=BOGUS + 0x2000, ws=BOGUS + 0x3000,
         ws_bytes=1 << 50):
    p = ctypes.byref(Params(paths, max_gap, min_hits, rule)) if params else None
    return lib.ssrlcv_hip_stereo_fill_holes(vp(src), vp(dst), vp(mask), u32(w), u32(h), p, vp(ws), csz(ws_bytes), vp(None))


def need(lib, w, h, paths=0xFF, max_gap=32, min_hits=1, rule=0, params=True):
    p = ctypes.byref(Params(paths, max_gap, min_hits, rule)) if params else None
    return lib.ssrlcv_hip_stereo_fill_holes_workspace_bytes(u32(w), u32(h), p)


BAD_PARAMS = [dict(params=False), dict(paths=0), dict(paths=0x100), dict(paths=0xFFFFFFFF), dict(min_hits=0), dict(min_hits=9),
              dict(paths=0x03, min_hits=3), dict(paths=0x10, min_hits=2), dict(rule=2), dict(rule=0xFFFFFFFF)]


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
        assert hasattr(_lib.load(), name), name
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.load().ssrlcv_hip_abi_version() == 4
    median_at, fill_at = header.index("int ssrlcv_hip_stereo_filter_median"), header.index("---- hole filling")
    assert median_at < fill_at < header.index("int ssrlcv_sift_plan_overflow")       # behind the median, before the overflow section
    section = header[fill_at:header.index("int ssrlcv_hip_stereo_fill_holes(")]
    for item in ("0x7FC00000", "MEASURED", "HOLE", "p - t (dx, dy)", "t <= maxGap", "Only `in` is looked at", "NOT idempotent", "n < minHits",
                 "b ^ 0x7FFFFFFF", "rank 0", "(n - 1) / 2", "of the input values: no arithmetic, no tolerance", "out of place", "No cost map is touched",
                 "UINT32_MAX", "popcount(paths) a256(4 w h) bytes", "may hold anything on entry", "no atomics", "bit-equal run to run",
                 "whatever the gap", "plane fits", "weighted by distance", "more than 8 directions", "view's map",
                 "uint32_t paths;", "uint32_t maxGap;", "uint32_t minHits;", "uint32_t rule;", "ssrlcv_fill_params; /* 16 bytes */"):
        assert item in section, item
    post = header[header.index("---- disparity post-filters"):median_at]
    assert '"hole filling"' in post and "hole filling or interpolation" not in post  # the gap it named is a pointer now
    assert ctypes.sizeof(capi.FillParams) == 16 and [f[0] for f in capi.FillParams._fields_] == ["paths", "maxGap", "minHits", "rule"]
    assert (capi.FILL_MIN, capi.FILL_MEDIAN) == (0, 1)
    sig = inspect.signature
    assert list(sig(capi.stereo_fill_holes).parameters) == ["disp_d", "paths", "max_gap", "min_hits", "rule", "want_mask", "workspace"]
    assert (sig(capi.stereo_fill_holes).parameters["want_mask"].default, sig(capi.stereo_fill_holes).parameters["workspace"].default) == (False, None)
    p = sig(pipeline.stereo_fill).parameters
    assert list(p) == ["disp", "paths", "max_gap", "min_hits", "rule", "want_mask"]
    assert [p[k].default for k in list(p)[1:]] == [0xFF, 32, 5, "min", False]
    assert list(sig(pipeline.stereo_filter).parameters) == ["disp", "cost", "median", "speckle_size", "speckle_diff"]   # unchanged


def test_post_takes_fill_and_refuses_every_other_key_before_any_work():
    from ssrlcv_amd import pipeline
    assert pipeline._post_filter("the map", None) == "the map"
    for bad in (dict(median=1, speckle=3), dict(cost=None), dict(fill=dict(want_mask=True)), dict(fill=dict(gap=3)), dict(fill=3),
                dict(fill=dict(), filled=1)):
        with pytest.raises(TypeError, match="^post takes"):
            pipeline._post_filter(None, bad)
    for rule in ("max", 0, None, "MIN"):
        with pytest.raises(ValueError):
            pipeline._post_filter(None, dict(fill=dict(rule=rule)))      # before the map (None here) is touched
        with pytest.raises(ValueError):
            pipeline.stereo_fill(None, rule=rule)


def test_parameters_then_the_size_then_the_buffers_then_the_workspace(lib):
    for bad in BAD_PARAMS:
        assert fill(lib, **bad) == INVALID_ARG, bad
        assert fill(lib, w=0, src=None, dst=None, ws=None, **bad) == INVALID_ARG, bad           # the parameters before the empty map
    assert fill(lib, w=65536, h=32768) == INVALID_ARG                                            # w h = 2^31
    assert fill(lib, w=65536, h=32768, src=None, ws_bytes=0) == INVALID_ARG
    for w, h in ((0, 48), (64, 0), (0, 0)):
        assert fill(lib, w=w, h=h, src=None, dst=None, mask=None, ws=None, ws_bytes=0) == OK    # nothing to do: before the buffers
    assert fill(lib, src=None) == INVALID_ARG and fill(lib, dst=None) == INVALID_ARG and fill(lib, ws=None) == INVALID_ARG
    assert fill(lib, src=BOGUS, dst=BOGUS) == INVALID_ARG                                        # in == out
    assert fill(lib, src=None, ws_bytes=0) == INVALID_ARG                                        # a NULL buffer before a short workspace
    want = need(lib, 64, 48)
    assert want == 8 * a256(4 * 64 * 48)
    assert fill(lib, ws_bytes=want - 1) == WORKSPACE and fill(lib, ws_bytes=0) == WORKSPACE
    assert fill(lib, mask=None, ws_bytes=0) == WORKSPACE                                         # filled may be NULL: not an argument error
    for legal in (dict(max_gap=0), dict(max_gap=NO_LIMIT), dict(paths=0x01, min_hits=1), dict(paths=0xFF, min_hits=8), dict(rule=1),
                  dict(paths=0x80, min_hits=1)):
        assert fill(lib, ws_bytes=0, **legal) == WORKSPACE, legal                                # accepted up to the size check
    assert fill(lib, w=65536, h=32767, ws_bytes=0) == WORKSPACE                                  # just below 2^31 pixels


def a256(n):
    return (n + 255) // 256 * 256


def test_the_workspace_query_follows_the_headers_formula(lib):
    for w, h in [(1, 1), (1, 37), (41, 1), (64, 16), (65, 17), (97, 83), (1024, 1024), (4096, 4096), (65536, 32767), (1, 2 ** 31 - 1)]:
        for paths in (0x01, 0x03, 0x0F, 0xF0, 0xFF, 0xA5, 0x80):
            assert need(lib, w, h, paths) == bin(paths).count("1") * a256(4 * w * h), (w, h, paths)
    assert need(lib, 4096, 4096) == 512 << 20
    assert need(lib, 65536, 32767) == 8 * 4 * 65536 * 32767 > 1 << 35                           # computed in size_t
    assert need(lib, 64, 48, max_gap=0) == need(lib, 64, 48, max_gap=NO_LIMIT) == need(lib, 64, 48, rule=1)
    for w, h in ((65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF), (2 ** 31, 1)):
        assert need(lib, w, h) == 0                                                              # refused sizes
    for bad in BAD_PARAMS:
        assert need(lib, 64, 48, **bad) == 0, bad                                                # refused parameters
    assert need(lib, 0, 48) == 0 and need(lib, 64, 0) == 0                                       # nothing to hold


def test_the_mirror_program_compiles():
    """tests/cpp/fill_test.cpp includes ssrlcv.hpp, so both DisparityFactory::fillHoles compile too"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/fill_test"])
    out = subprocess.run([os.path.join(host, "_build", "fill_test")], stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr        # no arguments: the usage line, no GPU touched
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    one = "ptr::value<Unity<float>> fillHoles(ptr::value<Unity<float>> disparity, unsigned int paths, unsigned int maxGap, unsigned int minHits, unsigned int rule)"
    assert one in factory and factory.count("fillHoles(ptr::value<Unity<float>> disparity") == 2
    assert "ptr::value<Unity<unsigned char>>* filled" in factory
    for name in NAMES:
        assert name in factory, name


def test_the_documents_describe_the_feature():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Hole filling" in design and "k_fill_march" in design and "k_fill_rows" in design and "k_fill_select" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_stereo_fill_holes" in open(os.path.join(root, doc)).read(), doc
    assert os.path.exists(os.path.join(root, "tools", "bench_fill.py"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "disparity_filter.hip")).read()
    fill = source[source.index("---- hole filling"):source.index("---- host side")]
    assert "atomic" not in fill                                   # the contract: no atomics in these passes
