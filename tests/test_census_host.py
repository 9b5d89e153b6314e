"""The census cost, the part that needs no GPU: the header, the loader and the binders name the five entry points, every
refusal is decided on the host in the contract's order before a buffer is looked at (the device pointers here are bogus or
null, so nothing is launched), the edges of every range are accepted -- an aggregation radius of 0 among them, which the SAD
calls still refuse --, both workspace queries follow the header's formulas, and the C++ mirror program compiles."""
import ctypes
import os
import re
import subprocess

import pytest

import helpers as H

u32, i32, csz, vp = ctypes.c_uint32, ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p
NAMES = ["ssrlcv_hip_census_u8", "ssrlcv_hip_stereo_census_workspace_bytes", "ssrlcv_hip_stereo_census_u8",
         "ssrlcv_hip_stereo_sgm_census_workspace_bytes", "ssrlcv_hip_stereo_sgm_census_u8"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference


class Stereo(ctypes.Structure):
    _fields_ = [("radius", u32), ("minDisparity", i32), ("numDisparities", u32), ("maxCost", u32), ("lrTolerance", i32), ("subpixel", u32)]


class Sgm(ctypes.Structure):
    _fields_ = [("radius", u32), ("minDisparity", i32), ("numDisparities", u32), ("costClamp", u32), ("P1", u32), ("P2", u32),
                ("paths", u32), ("lrTolerance", i32), ("subpixel", u32)]


def stereo(radius=2, dmin=0, D=64, max_cost=0xFFFFFFFF, lr=1, subpixel=1):
    return Stereo(radius, dmin, D, max_cost, lr, subpixel)


def sgm(radius=0, dmin=0, D=64, clamp=24, P1=3, P2=20, paths=0xFF, lr=1, subpixel=1):
    return Sgm(radius, dmin, D, clamp, P1, P2, paths, lr, subpixel)


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    for name in ("ssrlcv_hip_stereo_census_workspace_bytes", "ssrlcv_hip_stereo_sgm_census_workspace_bytes", "ssrlcv_hip_stereo_workspace_bytes",
                 "ssrlcv_hip_stereo_sgm_workspace_bytes"):
        getattr(lb, name).restype = csz
    return lb


def ref(p):
    return ctypes.byref(p) if p is not None else None


def need(lib, w, h, p, c=2):
    fn = lib.ssrlcv_hip_stereo_sgm_census_workspace_bytes if isinstance(p, Sgm) else lib.ssrlcv_hip_stereo_census_workspace_bytes
    return fn(u32(w), u32(h), ref(p), u32(c))


def call(lib, p, c=2, w=64, h=48, left=BOGUS, right=BOGUS, ws=BOGUS, ws_bytes=1 << 50, disp=BOGUS, cost=BOGUS, entry=None):
    fn = entry or (lib.ssrlcv_hip_stereo_sgm_census_u8 if isinstance(p, Sgm) else lib.ssrlcv_hip_stereo_census_u8)
    return fn(vp(left), vp(right), u32(w), u32(h), ref(p), u32(c), vp(ws), csz(ws_bytes), vp(disp), vp(cost), vp(None))


BOTH = [stereo, sgm]


def test_header_loader_and_binders_name_the_entry_points():
    import inspect
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
        assert hasattr(_lib.load(), name), name
    assert ctypes.sizeof(Stereo) == 24 == ctypes.sizeof(capi.StereoParams) and ctypes.sizeof(Sgm) == 36 == ctypes.sizeof(capi.SgmParams)
    assert "} ssrlcv_sgm_params;        /* 36 bytes */" in header
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.load().ssrlcv_hip_abi_version() == 4
    sgm_at, census_at, rect_at = (header.index(t) for t in ("---- semi-global matching", "---- census cost", "---- rectification"))
    assert header.index("---- dense stereo") < sgm_at < census_at < rect_at       # directly behind semi-global matching
    section = header[census_at:rect_at]
    for item in ("censusRadius", "AGGREGATION", "rho = r + c", "strictly", "popcount", "10800", "2 a256(w h) + 256 + 2 a256(8 w h)",
                 "2 a256(w h) + 2 a256(2 w h K) + 256 + 2 a256(8 w h)", "9 x 7", "centre-symmetric", "ternary", "colour", "NCC",
                 "uniqueness ratio", "ssrlcv_hip_stereo_sgm_set_pass_events"):
        assert item in section, item
    for earlier in (header[header.index("---- dense stereo"):sgm_at], header[sgm_at:census_at]):
        assert 'census costs: the section "census cost" below' in earlier      # the two older sections point here now
    # census is the last parameter of the binders, so positional callers of the SAD forms keep working
    for fn in (capi.stereo_disparity, capi.stereo_sgm, pipeline.stereo_disparity, pipeline.stereo_sgm):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-1] == "census" and sig["census"].default == 0, fn
    assert list(inspect.signature(capi.census).parameters) == ["img_d", "census"]


@pytest.mark.parametrize("make", BOTH)
@pytest.mark.parametrize("kw", [dict(D=0), dict(dmin=-32769), dict(dmin=32768), dict(subpixel=2), dict(subpixel=0xFFFFFFFF)])
def test_invalid_parameters(lib, make, kw):
    p = make(**kw)
    assert call(lib, p) == INVALID_ARG and need(lib, 64, 48, p) == 0


@pytest.mark.parametrize("make", BOTH)
def test_census_radius_zero_is_invalid_and_radius_zero_is_not(lib, make):
    assert call(lib, make(), c=0) == INVALID_ARG and need(lib, 64, 48, make(), c=0) == 0
    p = make(radius=0)
    assert need(lib, 64, 48, p) > 0 and call(lib, p, ws_bytes=0) == WORKSPACE          # accepted up to the size check
    assert call(lib, None) == INVALID_ARG and need(lib, 64, 48, None) == 0
    # the SAD calls still refuse it
    sad = lib.ssrlcv_hip_stereo_sgm_u8 if make is sgm else lib.ssrlcv_hip_stereo_sad_u8
    assert sad(vp(BOGUS), vp(BOGUS), u32(64), u32(48), ref(p), vp(BOGUS), csz(1 << 50), vp(BOGUS), vp(BOGUS), vp(None)) == INVALID_ARG
    sad_need = lib.ssrlcv_hip_stereo_sgm_workspace_bytes if make is sgm else lib.ssrlcv_hip_stereo_workspace_bytes
    assert sad_need(u32(64), u32(48), ref(p)) == 0


def test_sgm_invalid_parameters(lib):
    for kw in (dict(P1=21), dict(P1=1, P2=0), dict(paths=0), dict(paths=0x100), dict(paths=0xFFFFFFFF)):
        p = sgm(**kw)
        assert call(lib, p) == INVALID_ARG and need(lib, 64, 48, p) == 0, kw


@pytest.mark.parametrize("make", BOTH)
def test_too_many_pixels(lib, make):
    assert call(lib, make(), w=65536, h=32768) == INVALID_ARG and need(lib, 65536, 32768, make()) == 0   # w h = 2^31
    assert need(lib, 65536, 32767, make()) > 0                                                            # just below


@pytest.mark.parametrize("make", BOTH)
def test_unsupported_parameters(lib, make):
    for c, kw in ((4, {}), (0xFFFFFFFF, {}), (2, dict(radius=8)), (1, dict(radius=15)), (2, dict(D=257)), (4, dict(radius=8, D=1000))):
        p = make(**kw)
        assert call(lib, p, c=c) == UNSUPPORTED and need(lib, 64, 48, p, c=c) == 0, (c, kw)
    if make is sgm:
        for kw in (dict(clamp=8172, P2=20), dict(paths=1, clamp=65516, P2=20), dict(clamp=0xFFFFFFFF, P2=0xFFFFFFFF, P1=0)):
            p = sgm(**kw)
            assert call(lib, p) == UNSUPPORTED and need(lib, 64, 48, p) == 0, kw


@pytest.mark.parametrize("make", BOTH)
def test_the_order_of_the_refusals(lib, make):
    assert call(lib, make(radius=8, subpixel=2)) == INVALID_ARG            # invalid before unsupported
    assert call(lib, make(radius=8), c=0) == INVALID_ARG
    assert call(lib, make(D=257), c=0) == INVALID_ARG
    assert call(lib, make(D=0), c=4) == INVALID_ARG
    assert call(lib, make(), c=4, w=65536, h=32768) == INVALID_ARG         # too many pixels before the unsupported census radius
    assert call(lib, make(radius=8), w=65536, h=32768) == INVALID_ARG
    assert call(lib, make(), c=4, left=None) == UNSUPPORTED                # the parameters before the buffers
    assert call(lib, make(radius=8), disp=None, ws_bytes=0) == UNSUPPORTED
    assert call(lib, make(), left=None, ws_bytes=0) == INVALID_ARG         # a NULL buffer before a short workspace
    if make is sgm:
        assert call(lib, sgm(radius=8, P1=500)) == INVALID_ARG             # P1 > P2 before the unsupported radius
        assert call(lib, sgm(clamp=60000, paths=0)) == INVALID_ARG         # paths 0 before the 16-bit bound
        assert call(lib, sgm(clamp=60000), c=0) == INVALID_ARG
        assert call(lib, sgm(clamp=60000), left=None) == UNSUPPORTED


@pytest.mark.parametrize("make", BOTH)
def test_the_edges_of_the_parameter_ranges_are_taken(lib, make):
    for c, kw in ((1, dict(radius=0)), (3, dict(radius=7)), (1, dict(radius=7)), (3, dict(radius=0)), (2, dict(D=1)), (2, dict(D=256)),
                  (2, dict(dmin=-32768)), (2, dict(dmin=32767)), (2, dict(subpixel=0)), (2, dict(lr=-1)), (2, dict(lr=2147483647))):
        p = make(**kw)
        assert need(lib, 64, 48, p, c=c) > 0, (c, kw)
        assert call(lib, p, c=c, ws_bytes=0) == WORKSPACE, (c, kw)
    if make is sgm:
        for kw in (dict(clamp=0), dict(P1=0, P2=0), dict(paths=0x07, clamp=21445, P2=400, P1=150), dict(paths=1, clamp=65535, P1=0, P2=0)):
            assert need(lib, 64, 48, sgm(**kw)) > 0 and call(lib, sgm(**kw), ws_bytes=0) == WORKSPACE, kw
    assert need(lib, 8, 8, make(radius=7), c=3) > 0 and need(lib, 0, 48, make()) >= 0    # smaller than the footprint, empty: no error


@pytest.mark.parametrize("make", BOTH)
def test_null_buffers_then_short_workspace(lib, make):
    p = make()
    for kw in (dict(left=None), dict(right=None), dict(ws=None), dict(disp=None)):
        assert call(lib, p, **kw) == INVALID_ARG, kw
        assert call(lib, p, ws_bytes=0, **kw) == INVALID_ARG, kw
    n = need(lib, 64, 48, p)
    assert call(lib, p, ws_bytes=n - 1) == WORKSPACE
    assert call(lib, p, ws_bytes=n - 1, cost=None) == WORKSPACE      # cost may be NULL: not an argument error


def test_the_per_kernel_export_refuses_in_the_same_order(lib):
    census = lambda c, w=64, h=48, img=BOGUS, codes=BOGUS: lib.ssrlcv_hip_census_u8(vp(img), u32(w), u32(h), u32(c), vp(codes), vp(None))
    assert census(0) == INVALID_ARG and census(2, w=65536, h=32768) == INVALID_ARG
    assert census(4) == UNSUPPORTED and census(4, img=None) == UNSUPPORTED and census(4, w=65536, h=32768) == INVALID_ARG
    assert census(2, img=None) == INVALID_ARG and census(3, codes=None) == INVALID_ARG
    assert census(2, w=0) == OK and census(1, h=0) == OK            # nothing to do, nothing launched


def a256(n):
    return (n + 255) // 256 * 256


def formula(w, h, D=None):
    """the header's two formulas; D = None: block matching"""
    K = 8
    while D is not None and K < D:
        K *= 2
    volumes = 2 * a256(2 * w * h * K) if D is not None else 0
    return 2 * a256(w * h) + volumes + 256 + 2 * a256(8 * w * h)


def test_workspace_queries_follow_the_headers_formulas(lib):
    for w, h in [(1, 1), (8, 30), (64, 48), (97, 83), (131, 70), (1024, 1024), (4096, 4096), (65536, 32767)]:
        assert need(lib, w, h, stereo()) == formula(w, h), (w, h)
        assert need(lib, w, h, sgm()) == formula(w, h, 64), (w, h)
    assert need(lib, 65536, 32767, sgm(D=256)) == formula(65536, 32767, 256) > 1 << 41     # computed in size_t
    sizes = [need(lib, 64, 48, sgm(D=D)) for D in (1, 8, 9, 16, 17, 64, 100, 128, 129, 256)]
    assert sizes == [formula(64, 48, D) for D in (1, 8, 9, 16, 17, 64, 100, 128, 129, 256)] and sizes == sorted(sizes)
    # the code maps are uint64 whatever the census radius, and the aggregation radius changes nothing
    assert len({need(lib, 64, 48, stereo(radius=r), c=c) for c in (1, 2, 3) for r in (0, 3, 7)}) == 1
    # the SAD layout plus the two code maps
    sad = lib.ssrlcv_hip_stereo_workspace_bytes(u32(97), u32(83), ref(stereo()))
    assert need(lib, 97, 83, stereo()) == sad + 2 * a256(8 * 97 * 83)
    sad = lib.ssrlcv_hip_stereo_sgm_workspace_bytes(u32(97), u32(83), ref(sgm(radius=1)))
    assert need(lib, 97, 83, sgm(radius=1)) == sad + 2 * a256(8 * 97 * 83)


def test_the_mirror_program_compiles():
    """tests/cpp/census_test.cpp includes ssrlcv.hpp, so DisparityFactory::setCensus / clearCensus compile too"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/census_test"])
    out = subprocess.run([os.path.join(host, "_build", "census_test")], stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr        # no arguments: the usage line, no GPU touched
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    assert "void setCensus(unsigned int censusRadius)" in factory and "void clearCensus()" in factory
    for name in NAMES[1:]:
        assert name in factory, name


def test_the_documents_describe_the_feature():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    section7 = design[design.index("## 7. Out of scope"):]
    section7 = section7[:section7.index("\n## ", 5)] if "\n## " in section7[5:] else section7
    assert "census or NCC costs" not in section7 and '"Census cost"' in section7      # it left the not-built list
    for item in ("non-square census", "centre-symmetric census", "ternary census"):
        assert item in section7, item                                                  # what of its family is still not built
    section4 = design[design.index("## 4."):design.index("## 5.")]
    assert "Census cost" in section4
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_stereo_census_u8" in open(os.path.join(root, doc)).read(), doc
