"""Surface accuracy, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "surface accuracy" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace query follows the header's formula, the records have
their sizes, the ABI number is still 4, the C++ mirror program compiles, and the tool and the documents exist."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H
from test_dsm_host import BAD_FRAMES, BOGUS, INF, INVALID_ARG, NAN, OK, UNSUPPORTED, WORKSPACE, a256, frame

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERY = "ssrlcv_hip_difference_stats_workspace_bytes"
NAMES = [QUERY, "ssrlcv_hip_dsm_difference", "ssrlcv_hip_difference_stats"]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, QUERY).restype = csz
    return lb


def params(center=0.0, absolute=0, quantiles=(5000,), num=None):
    from ssrlcv_amd import capi
    q = list(quantiles) + [0] * (8 - len(quantiles))
    return capi.DiffStatsParams(center, absolute, len(quantiles) if num is None else num, (u32 * 8)(*q[:8]))


def difference(lib, fr=True, n=1000, points=BOGUS, height=BOGUS + 0x1000, cells=BOGUS + 0x2000, diff=BOGUS + 0x3000, **frame_args):
    f = ctypes.byref(frame(**frame_args)) if fr else None
    return lib.ssrlcv_hip_dsm_difference(vp(points), u32(n), vp(height), f, vp(cells), vp(diff), vp(None))


def stats(lib, p=True, n=1000, values=BOGUS, out=BOGUS + 0x1000, ws=BOGUS + 0x2000, ws_bytes=1 << 50, **param_args):
    prm = ctypes.byref(params(**param_args)) if p else None
    return lib.ssrlcv_hip_difference_stats(vp(values), u32(n), prm, vp(out), vp(ws), csz(ws_bytes), vp(None))


def formula(n):
    """the header's: 256 + 196608 + a256(16 T(n)) + a256(16 T(T(n))), T(n) = ceil(n / 4096)"""
    t = lambda k: (k + 4095) // 4096  # noqa: E731
    return 256 + 196608 + a256(16 * t(n)) + a256(16 * t(t(n)))


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4 and _lib.load().ssrlcv_hip_abi_version() == 4   # additions keep the number
    ortho_at, acc_at = header.index("int ssrlcv_hip_dsm_ortho("), header.index("---- surface accuracy")
    assert ortho_at < acc_at < header.index("int ssrlcv_sift_plan_overflow")      # behind the ortho-image, before the overflow section
    section = re.sub(r"\n \*\s+", " ", header[acc_at:header.index("int ssrlcv_sift_plan_overflow")])
    for text in ("0x7FC00000", "word for word", "floorf(u)", "uu = u - 0.5f", "fi < (float)(w - 1)", "has no inside", "t >= s", "s + t <= 1",
                 "r = za + ((t (zc - za)) + (s (zd - zc)))", "r = za + ((s (zb - za)) + (t (zd - zb)))", "r = za + ((s (zb - za)) + (t (zc - za)))",
                 "r = zd + (((1 - s) (zc - zd)) + ((1 - t) (zb - zd)))", "positive means above the reference", "parts per 10000",
                 "(uint64)q (m - 1) / 10000", "always one of the inputs", "lower median", "l + 256 r", "acc[l] += acc[l + half]", "host float64",
                 "256 + 196608 + a256(16 T(n)) + a256(16 T(T(n)))", "INTEGER atomics", "bit-equal run to run", "other than the frame's ez",
                 "unorganised meshes", "shift search", "float atomics", "weighted statistics", "ssrlcv_diff_stats_params; /* 44 bytes */",
                 "ssrlcv_diff_stats; /* 72 bytes */"):
        assert text in section, text
    assert ctypes.sizeof(capi.DiffStats) == 72 and ctypes.sizeof(capi.DiffStatsParams) == 44
    assert capi.DiffStats.sum.offset == 16 and capi.DiffStats.min.offset == 32 and capi.DiffStats.quantile.offset == 40
    sig = inspect.signature
    assert list(sig(capi.dsm_difference).parameters)[:4] == ["points_d", "height_d", "frame", "cells_d"]
    assert list(sig(capi.difference_stats).parameters)[:4] == ["values_d", "center", "absolute", "quantiles"]
    assert list(sig(pipeline.surface_difference).parameters) == ["points", "reference", "frame", "mesh", "max_jump"]
    assert sig(pipeline.surface_difference).parameters["mesh"].default is True and sig(pipeline.surface_difference).parameters["max_jump"].default is None
    assert list(sig(pipeline.difference_stats).parameters) == ["diff", "center", "absolute", "quantiles"]
    assert sig(pipeline.difference_stats).parameters["quantiles"].default == (5000,)
    assert list(sig(pipeline.surface_accuracy).parameters)[:4] == ["subject", "reference", "frame", "subject_frame"]


def test_difference_refusals_in_the_contract_s_order(lib):
    for bad in BAD_FRAMES + [dict(w=65536, h=32768)]:
        assert difference(lib, **bad) == INVALID_ARG, bad
        assert difference(lib, n=0, points=None, height=None, diff=None, **bad) == INVALID_ARG, bad   # before n = 0
    assert difference(lib, w=(1 << 24) + 1, h=1 << 10) == INVALID_ARG                # w h >= 2^31 before the side
    assert difference(lib, w=(1 << 24) + 1, h=1) == UNSUPPORTED and difference(lib, w=1, h=(1 << 24) + 1, n=0) == UNSUPPORTED
    assert difference(lib, n=0, points=None, height=None, cells=None, diff=None) == OK   # nothing is looked at
    for null in ("points", "height", "diff"):
        assert difference(lib, **{null: None}) == INVALID_ARG, null
        assert difference(lib, cells=None, **{null: None}) == INVALID_ARG, null


def test_stats_refusals_in_the_contract_s_order(lib):
    assert stats(lib, p=False) == INVALID_ARG and stats(lib, p=False, n=0, out=None) == INVALID_ARG
    for bad in (dict(num=9), dict(quantiles=(10001,)), dict(quantiles=(0, 5000, 0xFFFFFFFF)), dict(center=NAN), dict(center=INF), dict(center=-INF),
                dict(absolute=2)):
        assert stats(lib, **bad) == INVALID_ARG, bad
        assert stats(lib, n=0, out=None, values=None, ws=None, ws_bytes=0, **bad) == INVALID_ARG, bad   # the parameters first
    assert stats(lib, out=None) == INVALID_ARG and stats(lib, n=0, out=None) == INVALID_ARG          # the record before n = 0
    for null in ("values", "ws"):
        assert stats(lib, **{null: None}) == INVALID_ARG, null
        assert stats(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null          # a NULL buffer before a short workspace
    want = getattr(lib, QUERY)(u32(1000), ctypes.byref(params()))
    assert want == formula(1000)
    assert stats(lib, ws_bytes=want - 1) == WORKSPACE and stats(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(quantiles=()), dict(quantiles=(0, 10000)), dict(quantiles=(5000,) * 8), dict(absolute=1), dict(center=-3.5),
                  dict(quantiles=(1, 2, 10001), num=2)):                            # an entry behind numQuantiles is not looked at
        assert stats(lib, ws_bytes=0, **legal) == WORKSPACE, legal                  # accepted up to the size check


def test_the_workspace_formula(lib):
    query = getattr(lib, QUERY)
    for n in (0, 1, 4096, 4097, 4096 * 4096, 4096 * 4096 + 5, (1 << 32) - 1):
        for p in (params(), params(quantiles=()), params(quantiles=(5000,) * 8, absolute=1)):
            assert query(u32(n), ctypes.byref(p)) == formula(n), n
    assert formula(4096 * 4096 + 5) == 256 + 196608 + a256(16 * 4097) + 256
    assert query(u32(1000), None) == 0
    for bad in (params(num=9), params(quantiles=(10001,)), params(center=NAN), params(absolute=2)):
        assert query(u32(1000), ctypes.byref(bad)) == 0


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/accuracy_test"])
    r = subprocess.run([os.path.join(host, "_build", "accuracy_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("void setReferenceSurface(ptr::value<Unity<float>> height, const ssrlcv_dsm_frame& frame, float maxJump = ",
                   "ptr::value<Unity<float>> calculatePerPointDifference(ptr::value<Unity<float3>> cloud, float3 planeNormal)",
                   "double calculateAverageDifference(ptr::value<Unity<float3>> cloud, float3 planeNormal)", "AccuracyReport accuracyReport(",
                   "0.999999f", "ssrlcv_hip_dsm_difference(", "ssrlcv_hip_difference_stats(", "ssrlcv_hip_disparity_mesh("):
        assert member in factory, member


def test_the_documents_and_the_bench_tool_exist():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Surface accuracy" in design
    for kernel in ("k_dsm_difference", "k_stats_tiles", "k_stats_hist", "k_stats_narrow", "k_stats_reduce"):
        assert kernel in design, kernel
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(root, doc)).read()
        assert "ssrlcv_hip_dsm_difference" in text and "ssrlcv_hip_difference_stats" in text, doc
    assert "accuracy_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_accuracy.py")) and os.path.exists(os.path.join(root, "profiles", "accuracy_bench.txt"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "accuracy.hip")).read()
    assert "#if" not in source and "atomicAdd(float" not in source and "unsafeAtomicAdd" not in source   # one digit width, no float atomic
    assert "accuracy.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
