"""The disparity post-filters, the part that needs no GPU: the header, the loader and the binders name the five entry points,
every refusal of include/ssrlcv_hip.h "disparity post-filters" is decided on the host in the contract's order before a buffer
is looked at (the device pointers here are bogus or null, so nothing is launched), the workspace queries follow the header's
formulas, and the C++ mirror program compiles."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
NAMES = ["ssrlcv_hip_disparity_components_workspace_bytes", "ssrlcv_hip_disparity_components",
         "ssrlcv_hip_stereo_filter_speckles_workspace_bytes", "ssrlcv_hip_stereo_filter_speckles", "ssrlcv_hip_stereo_filter_median"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    for name in (NAMES[0], NAMES[2]):
        getattr(lb, name).restype = csz
    return lb


def components(lib, w=64, h=48, max_diff=1.0, disp=BOGUS, labels=BOGUS, sizes=BOGUS, ws=BOGUS, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_disparity_components(vp(disp), u32(w), u32(h), f32(max_diff), vp(labels), vp(sizes), vp(ws), csz(ws_bytes), vp(None))


def speckles(lib, w=64, h=48, max_diff=1.0, max_size=10, disp=BOGUS, cost=BOGUS, ws=BOGUS, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_stereo_filter_speckles(vp(disp), vp(cost), u32(w), u32(h), f32(max_diff), u32(max_size), vp(ws), csz(ws_bytes), vp(None))


def median(lib, w=64, h=48, radius=1, src=BOGUS, dst=BOGUS + 0x1000):
    return lib.ssrlcv_hip_stereo_filter_median(vp(src), vp(dst), u32(w), u32(h), u32(radius), vp(None))


def need_components(lib, w, h):
    return lib.ssrlcv_hip_disparity_components_workspace_bytes(u32(w), u32(h))


def need_speckles(lib, w, h):
    return lib.ssrlcv_hip_stereo_filter_speckles_workspace_bytes(u32(w), u32(h))


BOTH = [components, speckles]


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
        assert hasattr(_lib.load(), name), name
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.load().ssrlcv_hip_abi_version() == 4
    rect_at, post_at = header.index("---- rectification"), header.index("---- disparity post-filters")
    assert rect_at < post_at < header.index("int ssrlcv_sift_plan_overflow")          # behind rectification
    section = header[post_at:header.index("int ssrlcv_hip_stereo_filter_median")]
    for item in ("0x7FC00000", "fabsf(d(p) - d(q)) <= maxDiff", "transitive closure", "smallest raster index", "UINT32_MAX", "idempotent",
                 "LOWER median", "b ^ 0x7FFFFFFF", "(n - 1) / 2", "cost map is NOT touched", "a256(4 w h) bytes", "2 a256(4 w h) bytes",
                 "may hold anything on entry", "atomicMin", "atomicAdd", "bit-equal run to run", "no grid barrier", "8-connectivity"):
        assert item in section, item
    sig = inspect.signature
    assert list(sig(capi.disparity_components).parameters) == ["disp_d", "max_diff", "want_sizes", "workspace"]
    assert list(sig(capi.stereo_filter_speckles).parameters) == ["disp_d", "cost_d", "max_size", "max_diff", "workspace"]
    assert list(sig(capi.stereo_filter_median).parameters) == ["disp_d", "radius"]
    p = sig(pipeline.stereo_filter).parameters
    assert list(p) == ["disp", "cost", "median", "speckle_size", "speckle_diff"]
    assert (p["cost"].default, p["median"].default, p["speckle_size"].default, p["speckle_diff"].default) == (None, 0, 0, 1.0)
    for fn in (pipeline.stereo_cloud, pipeline.stereo_cloud_cameras):
        assert sig(fn).parameters["post"].default is None, fn


def test_post_refuses_an_unknown_key_before_any_work():
    from ssrlcv_amd import pipeline
    assert pipeline._post_filter("the map", None) == "the map"
    with pytest.raises(TypeError):
        pipeline._post_filter(None, dict(median=1, speckle=3))
    with pytest.raises(TypeError):
        pipeline._post_filter(None, dict(cost=None))


@pytest.mark.parametrize("call", BOTH)
def test_max_diff_then_the_size_then_the_buffers_then_the_workspace(lib, call):
    for bad in (NAN, -1.0, -INF, -1e-45):
        assert call(lib, max_diff=bad) == INVALID_ARG
        assert call(lib, max_diff=bad, w=0) == INVALID_ARG                     # the parameter before the empty map
    assert call(lib, w=65536, h=32768) == INVALID_ARG                          # w h = 2^31
    assert call(lib, w=65536, h=32768, max_diff=NAN, disp=None) == INVALID_ARG
    for w, h in ((0, 48), (64, 0), (0, 0)):
        assert call(lib, w=w, h=h, disp=None, ws=None, ws_bytes=0) == OK       # nothing to do: before the buffers
    assert call(lib, disp=None) == INVALID_ARG and call(lib, ws=None) == INVALID_ARG
    assert call(lib, disp=None, ws_bytes=0) == INVALID_ARG                     # a NULL buffer before a short workspace
    need = (need_components if call is components else need_speckles)(lib, 64, 48)
    assert call(lib, ws_bytes=need - 1) == WORKSPACE and call(lib, ws_bytes=0) == WORKSPACE
    for legal in (0.0, -0.0, INF, 1e-45, 3.0e38):                              # accepted up to the size check
        assert call(lib, max_diff=legal, ws_bytes=0) == WORKSPACE, legal
    assert call(lib, w=65536, h=32767, ws_bytes=0) == WORKSPACE                # just below 2^31 pixels


def test_optional_buffers(lib):
    assert components(lib, sizes=None, ws_bytes=0) == WORKSPACE                # sizes may be NULL: not an argument error
    assert components(lib, labels=None) == INVALID_ARG
    assert speckles(lib, cost=None, ws_bytes=0) == WORKSPACE                   # cost may be NULL
    assert speckles(lib, max_size=0, ws_bytes=0) == WORKSPACE and speckles(lib, max_size=0xFFFFFFFF, ws_bytes=0) == WORKSPACE
    assert speckles(lib, max_size=0, disp=None) == INVALID_ARG                 # removing nothing is legal, a NULL map is not


def test_median_refusals_in_order(lib):
    assert median(lib, radius=0) == INVALID_ARG
    assert median(lib, radius=0, w=0) == INVALID_ARG
    assert median(lib, w=65536, h=32768) == INVALID_ARG
    assert median(lib, radius=3, w=65536, h=32768) == INVALID_ARG              # invalid before unsupported
    assert median(lib, radius=3) == UNSUPPORTED and median(lib, radius=0xFFFFFFFF) == UNSUPPORTED
    assert median(lib, radius=3, src=None) == UNSUPPORTED                      # the parameters before the buffers
    assert median(lib, radius=3, w=0) == UNSUPPORTED                           # ... and before the empty map
    for w, h in ((0, 48), (64, 0)):
        assert median(lib, w=w, h=h, src=None, dst=None) == OK
    for r in (1, 2):
        assert median(lib, radius=r, src=None) == INVALID_ARG and median(lib, radius=r, dst=None) == INVALID_ARG
        assert median(lib, radius=r, src=BOGUS, dst=BOGUS) == INVALID_ARG      # in == out


def a256(n):
    return (n + 255) // 256 * 256


def test_workspace_queries_follow_the_headers_formulas(lib):
    for w, h in [(1, 1), (1, 37), (131, 1), (64, 16), (65, 17), (97, 83), (200, 100), (1024, 1024), (4096, 4096), (65536, 32767), (1, 2 ** 31 - 1)]:
        assert need_components(lib, w, h) == a256(4 * w * h), (w, h)
        assert need_speckles(lib, w, h) == 2 * a256(4 * w * h), (w, h)
    assert need_speckles(lib, 4096, 4096) == 128 << 20                          # 8 bytes per pixel
    assert need_speckles(lib, 65536, 32767) == 8 * 65536 * 32767 > 1 << 33      # computed in size_t
    for w, h in ((65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF), (2 ** 31, 1)):
        assert need_components(lib, w, h) == 0 and need_speckles(lib, w, h) == 0   # refused sizes
    assert need_components(lib, 0, 48) == 0 and need_speckles(lib, 64, 0) == 0     # nothing to hold


def test_the_mirror_program_compiles():
    """tests/cpp/speckle_test.cpp includes ssrlcv.hpp, so DisparityFactory::filterSpeckles / medianFilter compile too"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/speckle_test"])
    out = subprocess.run([os.path.join(host, "_build", "speckle_test")], stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr        # no arguments: the usage line, no GPU touched
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    assert "void filterSpeckles(ptr::value<Unity<float>> disparity, ptr::value<Unity<unsigned int>> cost, unsigned int maxSpeckleSize, float maxDiff)" in factory
    assert "ptr::value<Unity<float>> medianFilter(ptr::value<Unity<float>> disparity, unsigned int radius)" in factory
    for name in (NAMES[2], NAMES[3], NAMES[4]):
        assert name in factory, name


def test_the_documents_describe_the_feature():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Disparity post-filters" in design and "union-find" in design
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(root, doc)).read()
        assert "ssrlcv_hip_stereo_filter_speckles" in text and "ssrlcv_hip_stereo_filter_median" in text, doc
    assert os.path.exists(os.path.join(root, "tools", "bench_speckle.py"))
    makefile = open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
    assert "disparity_filter.hip" in makefile
