"""Semi-global matching, the part that needs no GPU: the header, the loader and capi.SgmParams agree (36 bytes, the header's
field order), every refusal is decided on the host in the stated order before a buffer is looked at (the device pointers here
are bogus or null), the edges of every range are accepted, the workspace query is 0 for refused parameters and grows with the
image and the disparity count, and the C++ mirror program compiles."""
import ctypes
import os
import re
import subprocess

import pytest

import helpers as H

u32, i32, csz, vp = ctypes.c_uint32, ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p
NAMES = ["ssrlcv_hip_stereo_sgm_workspace_bytes", "ssrlcv_hip_stereo_sgm_u8", "ssrlcv_hip_stereo_sgm_set_pass_events"]
FIELDS = ["radius", "minDisparity", "numDisparities", "costClamp", "P1", "P2", "paths", "lrTolerance", "subpixel"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference


class Params(ctypes.Structure):
    _fields_ = [("radius", u32), ("minDisparity", i32), ("numDisparities", u32), ("costClamp", u32), ("P1", u32), ("P2", u32),
                ("paths", u32), ("lrTolerance", i32), ("subpixel", u32)]


def params(radius=2, dmin=0, D=64, clamp=1000, P1=40, P2=400, paths=0xFF, lr=1, subpixel=1):
    return Params(radius, dmin, D, clamp, P1, P2, paths, lr, subpixel)


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    lb.ssrlcv_hip_stereo_sgm_workspace_bytes.restype = csz
    return lb


def need(lib, w, h, p):
    return lib.ssrlcv_hip_stereo_sgm_workspace_bytes(u32(w), u32(h), ctypes.byref(p) if p is not None else None)


def sgm(lib, p, w=64, h=48, left=BOGUS, right=BOGUS, ws=BOGUS, ws_bytes=1 << 50, disp=BOGUS, cost=BOGUS):
    return lib.ssrlcv_hip_stereo_sgm_u8(vp(left), vp(right), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(ws),
                                        csz(ws_bytes), vp(disp), vp(cost), vp(None))


def test_header_loader_and_binder_agree():
    from ssrlcv_amd import _lib, capi
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
    body = re.search(r"typedef struct \{([^}]*)\} ssrlcv_sgm_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert declared == FIELDS
    assert ctypes.sizeof(Params) == 36 and ctypes.sizeof(capi.SgmParams) == 36
    assert [f[0] for f in capi.SgmParams._fields_] == FIELDS == [f[0] for f in Params._fields_]
    assert [f[1] for f in capi.SgmParams._fields_] == [f[1] for f in Params._fields_]
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header
    section = header[header.index("---- semi-global matching"):header.index("---- rectification")]
    for item in ("uniqueness ratio", "colour", "census", "NCC", "more than 8 paths", "image gradient", "2 a256(w h) + 2 a256(2 w h K) + 256"):
        assert item in section, item


@pytest.mark.parametrize("kw", [dict(radius=0), dict(D=0), dict(dmin=-32769), dict(dmin=32768), dict(subpixel=2), dict(subpixel=0xFFFFFFFF),
                                dict(P1=401), dict(P1=1, P2=0), dict(paths=0), dict(paths=0x100), dict(paths=0xFFFFFFFF)])
def test_invalid_parameters(lib, kw):
    p = params(**kw)
    assert sgm(lib, p) == INVALID_ARG          # bogus device pointers: the parameters are judged first, nothing is launched
    assert need(lib, 64, 48, p) == 0


def test_null_params_and_too_many_pixels(lib):
    assert sgm(lib, None) == INVALID_ARG and need(lib, 64, 48, None) == 0
    assert sgm(lib, params(), w=65536, h=32768) == INVALID_ARG and need(lib, 65536, 32768, params()) == 0   # w h = 2^31
    assert need(lib, 65536, 32767, params()) > 0                                                            # just below


@pytest.mark.parametrize("kw", [dict(radius=16), dict(D=257), dict(radius=1000, D=100000),
                                dict(clamp=7792, P2=400),                       # 8 x 8192 = 65536
                                dict(paths=0x0F, clamp=15984, P2=400),          # 4 x 16384
                                dict(paths=1, clamp=65136, P2=400),             # 1 x 65536
                                dict(clamp=0xFFFFFFFF, P2=0xFFFFFFFF, P1=0),    # the product needs 64 bits
                                dict(clamp=0xFFFFFFFF, P2=1, P1=0),             # and so does the sum
                                dict(paths=1, clamp=0, P2=65536, P1=65536)])
def test_unsupported_parameters(lib, kw):
    p = params(**kw)
    assert sgm(lib, p) == UNSUPPORTED
    assert need(lib, 64, 48, p) == 0


def test_the_order_of_the_refusals(lib):
    assert sgm(lib, params(radius=16, subpixel=2)) == INVALID_ARG
    assert sgm(lib, params(radius=0, D=257)) == INVALID_ARG
    assert sgm(lib, params(radius=16, P1=500)) == INVALID_ARG               # P1 > P2 before the unsupported radius
    assert sgm(lib, params(clamp=60000, paths=0)) == INVALID_ARG            # paths 0 before the 16-bit bound
    assert sgm(lib, params(radius=16), w=65536, h=32768) == INVALID_ARG     # too many pixels before the unsupported radius
    assert sgm(lib, params(clamp=60000), w=65536, h=32768) == INVALID_ARG
    assert sgm(lib, params(radius=16), left=None) == UNSUPPORTED            # the parameters before the buffers
    assert sgm(lib, params(clamp=60000), disp=None, ws_bytes=0) == UNSUPPORTED
    assert sgm(lib, params(), left=None, ws_bytes=0) == INVALID_ARG         # a NULL buffer before a short workspace


def test_the_edges_of_the_parameter_ranges_are_taken(lib):
    for kw in (dict(radius=1), dict(radius=15), dict(D=1), dict(D=256), dict(dmin=-32768), dict(dmin=32767), dict(subpixel=0),
               dict(lr=-1), dict(lr=-2147483648), dict(lr=2147483647), dict(clamp=0), dict(P1=0), dict(P1=400), dict(P1=0, P2=0),
               dict(clamp=0, P1=0, P2=0), dict(paths=1), dict(paths=0x80), dict(paths=0xFF, clamp=7791, P2=400),   # 8 x 8191 = 65528
               dict(paths=0x07, clamp=21445, P2=400),                                                            # 3 x 21845 = 65535
               dict(paths=0x10, clamp=0, P1=65535, P2=65535), dict(paths=0x10, clamp=65535, P1=0, P2=0),
               dict(paths=0x0F, clamp=15983, P2=400)):                                                           # 4 x 16383
        p = params(**kw)
        assert need(lib, 64, 48, p) > 0, kw
        assert sgm(lib, p, ws_bytes=0) == WORKSPACE, kw   # past the parameter and buffer checks, stopped by the size check


def test_null_buffers_then_short_workspace(lib):
    p = params()
    for kw in (dict(left=None), dict(right=None), dict(ws=None), dict(disp=None)):
        assert sgm(lib, p, **kw) == INVALID_ARG, kw
        assert sgm(lib, p, ws_bytes=0, **kw) == INVALID_ARG, kw
    n = need(lib, 64, 48, p)
    assert sgm(lib, p, ws_bytes=n - 1) == WORKSPACE
    assert sgm(lib, p, ws_bytes=n - 1, cost=None) == WORKSPACE      # cost may be NULL: not an argument error


def test_the_pass_event_hook_takes_at_most_twelve(lib):
    hook = lib.ssrlcv_hip_stereo_sgm_set_pass_events
    assert hook(None, u32(1)) == INVALID_ARG
    assert hook((vp * 13)(), u32(13)) == INVALID_ARG
    assert hook((vp * 12)(), u32(12)) == OK          # twelve NULL entries: nothing would be recorded
    assert hook(None, u32(0)) == OK


def formula(w, h, D):
    a256 = lambda n: (n + 255) // 256 * 256
    K = 8
    while K < D:
        K *= 2
    return 2 * a256(w * h) + 2 * a256(2 * w * h * K) + 256


def test_workspace_query_follows_the_headers_formula(lib):
    last = 0
    for w, h in [(1, 1), (8, 30), (64, 48), (97, 83), (131, 70), (1024, 1024), (4096, 4096)]:
        n = need(lib, w, h, params())
        assert n == formula(w, h, 64) and n >= last, (w, h, n)
        last = n
    assert need(lib, 4096, 4096, params()) > 2 * 2 * 4096 * 4096 * 64                # two volumes of 2.1 GB: computed in size_t
    assert need(lib, 65536, 32767, params(D=256)) == formula(65536, 32767, 256) > 1 << 41
    sizes = [need(lib, 64, 48, params(D=D)) for D in (1, 8, 9, 16, 17, 64, 100, 128, 129, 256)]
    assert sizes == sorted(sizes) and sizes == [formula(64, 48, D) for D in (1, 8, 9, 16, 17, 64, 100, 128, 129, 256)]
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3] < sizes[4] and sizes[6] == sizes[7] < sizes[8] == sizes[9]
    assert need(lib, 0, 48, params()) >= 0  # an empty image is no error
    assert need(lib, 64, 48, params(paths=1)) == need(lib, 64, 48, params(paths=0xFF))   # S is one volume whatever the paths


def test_the_mirror_program_compiles():
    """tests/cpp/sgm_test.cpp includes ssrlcv.hpp, so DisparityFactory::setSemiGlobal / clearSemiGlobal compile too"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/sgm_test"])
    out = subprocess.run([os.path.join(host, "_build", "sgm_test")], stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr        # no arguments: the usage line, no GPU touched
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    assert "void setSemiGlobal(unsigned int costClamp, unsigned int P1, unsigned int P2, unsigned int paths = 0xFFu)" in factory
    assert "void clearSemiGlobal()" in factory and "ssrlcv_hip_stereo_sgm_u8" in factory
