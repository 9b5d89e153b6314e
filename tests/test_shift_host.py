"""The shift search, the part that needs no GPU: the header, the loader and the binders name the entry points and agree on the
layouts; the host pick (ssrlcv_shift_pick_host of the release library, through ctypes) equals the Python restatement bit for
bit on hand-made tables -- ties, missing neighbours, flat and one-sided parabolas, no candidate -- and on the tables of the
cases; every refusal of the device call is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, and no call here gets as far as a launch); the workspace query follows the header's formula."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import shift_cases as C
import shift_ref as R

u32, i32, f32, csz, vp = ctypes.c_uint32, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERIES = ["ssrlcv_shift_table_bytes", "ssrlcv_hip_shift_search_workspace_bytes"]
NAMES = QUERIES + ["ssrlcv_hip_shift_search", "ssrlcv_shift_pick_host"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x1000  # a "device pointer" nothing may dereference; 8-byte aligned
INF, NAN = float("inf"), float("nan")


class Params(ctypes.Structure):
    _fields_ = [("scale", f32), ("stride", u32), ("centerX", i32), ("centerY", i32), ("radius", u32), ("centerQ", i32), ("gateQ", u32)]


class Result(ctypes.Structure):
    _fields_ = [("shiftX", ctypes.c_int64), ("shiftY", ctypes.c_int64), ("subX", ctypes.c_double), ("subY", ctypes.c_double), ("bias", ctypes.c_double),
                ("variance", ctypes.c_double), ("second", ctypes.c_double), ("n", u32), ("candidates", u32)]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    for q in QUERIES:
        getattr(lb, q).restype = csz
    return lb


def a256(n):
    return (n + 255) // 256 * 256


def params(scale=64.0, stride=1, center=(0, 0), radius=8, center_q=0, gate_q=R.NO_GATE):
    return Params(scale, stride, center[0], center[1], radius, center_q, gate_q)


def search(lib, w=64, h=48, p="default", moving=BOGUS, reference=BOGUS + 0x10000, table=BOGUS + 0x20000, ws=BOGUS + 0x30000, ws_bytes=0):
    """ws_bytes = 0: a call that passes every other test stops at SSRLCV_ERR_WORKSPACE, before anything is launched"""
    p = params() if p == "default" else p
    return lib.ssrlcv_hip_shift_search(vp(moving), vp(reference), u32(w), u32(h), ctypes.byref(p) if p is not None else None, vp(table), vp(ws),
                                       csz(ws_bytes), vp(None))


def c_pick(lib, entries, p, min_overlap, head=None, out=None):
    raw = R.table_bytes(np.zeros((), R.HEAD) if head is None else head, entries)
    out = Result() if out is None else out
    rc = lib.ssrlcv_shift_pick_host(raw.ctypes.data_as(vp), csz(raw.size), ctypes.byref(p), u32(min_overlap), ctypes.byref(out))
    return rc, out


def assert_pick_equal(lib, entries, scale=64.0, stride=1, center=(0, 0), min_overlap=0):
    """the C entry point and the restatement, field by field, bit for bit -> the restatement's dictionary"""
    S = (entries.shape[0] - 1) // 2
    rc, got = c_pick(lib, entries, params(scale, stride, center, S), min_overlap)
    want = R.pick(entries, scale, stride, center, min_overlap)
    if want is None:
        assert rc == UNSUPPORTED
        return None
    assert rc == OK
    assert (got.shiftX, got.shiftY, got.n, got.candidates) == (want["shift"][0], want["shift"][1], want["n"], want["candidates"])
    for name, value in (("subX", want["sub"][0]), ("subY", want["sub"][1]), ("bias", want["bias"]), ("variance", want["variance"]), ("second", want["second"])):
        assert np.float64(getattr(got, name)).tobytes() == np.float64(value).tobytes(), (name, getattr(got, name), value)
    return want


def table(S, v=None, n=100):
    """entries with sum = 0 and sumSq = n v: the variance is v"""
    side = 2 * S + 1
    e = np.zeros((side, side), R.ENTRY)
    e["n"] = n
    e["sumSq"] = n * (np.full((side, side), 50) if v is None else np.asarray(v))
    return e


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    assert "shift search: shift_search (+ its workspace query), shift_table_bytes, shift_pick_host" in re.sub(
        r"\n \*\s+", " ", header[:header.index("#define SSRLCV_HIP_ABI_VERSION")])
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4        # additions keep the number
    reg_at, at, render_at = header.index("---- surface registration"), header.index("---- shift search"), header.index("---- mesh render")
    assert reg_at < header.index("int ssrlcv_register_compose_host(") < at < render_at     # directly behind "surface registration"
    assert "/* ----" not in header[header.index(";", header.index("int ssrlcv_register_compose_host(")):at]
    section = re.sub(r"\n \*\s+", " ", header[at:render_at])
    for text in ("t = x * scale", "fabsf(t) <= 65536.0f", "(int32)rintf(t)", "ties to even", "CLIPPED", "i < ceil(w / g)", "in sampled cells",
                 "(ky + S) (2S + 1) + (kx + S)", "|d - centerQ| <= gateQ", "gateQ = UINT32_MAX means no test", "holds zeros",
                 "Every byte of it is written", "S = 0 .. 32", "|centerX|, |centerY| <= 2^24", "|centerQ| <= 2^18", "2^28 sampled cells",
                 "n >= max(minOverlap, 1)", "v = (double)sumSq / (double)n - mean * mean", "nothing contracted", "then to the smaller ky",
                 "den = (vminus - v0) + (vplus - v0)", "clamped to -0.5 .. 0.5", "+inf if there is none", "`out` is untouched on error",
                 "moving(x) shows what reference(x + s) shows", "by -bias along ez", "the parameters before the sizes before the buffers",
                 "2 a256(4 ceil(w / g) ceil(h / g))", "It may hold anything on entry", "lanes own shifts, not cells", "no cross-lane reduction",
                 "INTEGER atomics", "no float atomics", "bit-equal run to run", "no block waits for another",
                 "ssrlcv_shift_params; /* 28 bytes */", "ssrlcv_shift_entry; /* 24 bytes */", "ssrlcv_shift_result; /* 64 bytes */"):
        assert text in section, text
    scope = section[section.index("Out of scope, not built:"):]
    for text in ("rotation or scale", "resampling", "correlation coefficients", "truncated costs", "FFT", "radii above 32", "use strides",
                 "reference's mesh", "pushbroom"):
        assert text in scope, text
    # the two lists that named the search as not built point here instead
    accuracy = re.sub(r"\n \*\s+", " ", header[header.index("---- surface accuracy"):reg_at])
    registration = re.sub(r"\n \*\s+", " ", header[reg_at:at])
    assert '"shift search"' in accuracy and '"shift search"' in registration
    for old in ("a shift search; float atomics", "a coarse shift search over many cells (the caller passes an initial pose)"):
        assert old not in accuracy and old not in registration
    assert ctypes.sizeof(Params) == 28 == ctypes.sizeof(capi.ShiftParams) and ctypes.sizeof(Result) == 64 == ctypes.sizeof(capi.ShiftResult)
    assert [f[0] for f in Params._fields_] == [f[0] for f in capi.ShiftParams._fields_]
    assert [f[0] for f in Result._fields_] == [f[0] for f in capi.ShiftResult._fields_]
    assert capi.SHIFT_ENTRY == R.ENTRY and capi.SHIFT_HEAD == R.HEAD and R.ENTRY.itemsize == 24 and R.ENTRY.fields["sum"][1] == 8
    assert capi.SHIFT_NO_GATE == R.NO_GATE == 0xFFFFFFFF and capi.SHIFT_MAX_RADIUS == R.MAX_RADIUS == 32
    sig = inspect.signature
    assert list(sig(capi.shift_search).parameters) == ["moving", "reference", "scale", "stride", "center", "radius", "center_q", "gate_q", "ws"]
    assert {k: p.default for k, p in sig(capi.shift_search).parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        stride=1, center=(0, 0), radius=8, center_q=0, gate_q=None, ws=None)
    assert list(sig(capi.shift_pick).parameters) == ["table", "params", "min_overlap"]
    assert list(sig(pipeline.surface_shift_search).parameters) == ["subject", "reference", "frame", "radius", "strides", "gate", "scale", "min_overlap", "rule",
                                                                   "initial"]
    assert {k: p.default for k, p in sig(pipeline.surface_shift_search).parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        radius=8, strides=(4, 1), gate=3.0, scale=None, min_overlap=0.25, rule="max", initial=None)
    assert list(sig(pipeline.surface_register_coarse).parameters) == ["points", "reference", "frame", "search", "register"]
    assert "orthonormal" in pipeline.surface_shift_search.__doc__


def test_the_pick_resolves_ties_in_the_stated_order(lib):
    e = table(2)
    assert assert_pick_equal(lib, e)["k"] == (0, 0)                    # all equal: the smallest kx^2 + ky^2
    e[2, 2]["n"] = 0
    assert assert_pick_equal(lib, e)["k"] == (0, -1)                   # four at distance 1: the smaller ky
    e[1, 2]["n"] = 0
    assert assert_pick_equal(lib, e)["k"] == (-1, 0)                   # then the smaller kx
    e[2, 1]["n"] = 0
    assert assert_pick_equal(lib, e)["k"] == (1, 0)
    e[2, 3]["n"] = 0
    assert assert_pick_equal(lib, e)["k"] == (0, 1)
    e[3, 2]["n"] = 0
    assert assert_pick_equal(lib, e)["k"] == (-1, -1)                  # distance 2: ky = -1 before ky = 1, kx = -1 before kx = 1
    v = np.full((5, 5), 50)
    v[4, 4] = 49                                                       # a smaller variance beats every distance
    assert assert_pick_equal(lib, table(2, v))["k"] == (2, 2)


def test_the_sub_cell_step(lib):
    v = np.full((5, 5), 90)
    v[2, 2], v[2, 1], v[2, 3], v[1, 2], v[3, 2] = 10, 30, 50, 40, 20     # the best in the middle; both parabolas open upwards
    got = assert_pick_equal(lib, table(2, v), stride=3, center=(4, -2))
    assert got["shift"] == (12, -6) and got["sub"] == ((0.5 * (30 - 50) / 60.0) * 3, (0.5 * (40 - 20) / 40.0) * 3)
    assert got["second"] * 64 * 64 == 90 and got["variance"] * 64 * 64 == 10 and got["candidates"] == 25
    e = table(2, v)
    e[2, 1]["n"] = 7                                                    # a neighbour below the overlap: no step along x, the one along y stays
    got = assert_pick_equal(lib, e, min_overlap=8)
    assert got["sub"] == (0.0, 0.25) and got["candidates"] == 24
    assert assert_pick_equal(lib, e, min_overlap=7)["sub"][0] != 0.0
    v = np.full((5, 5), 90)
    v[0, 4] = 10                                                        # the best in a corner of the table: no neighbour on one side
    got = assert_pick_equal(lib, table(2, v))
    assert got["k"] == (2, -2) and got["sub"] == (0.0, 0.0)
    v = np.full((5, 5), 50)                                             # den = 0: a flat score
    assert assert_pick_equal(lib, table(2, v))["sub"] == (0.0, 0.0)
    v = np.full((5, 5), 90)
    v[2, 2], v[2, 3], v[2, 1] = 10, 10, 70                              # one side as good as the best: the step is the clamp's +0.5 ...
    v[1, 2], v[3, 2] = 10, 33                                           # ... and -0.5
    got = assert_pick_equal(lib, table(2, v))
    assert got["k"] == (0, 0) and got["sub"] == (0.5, -0.5)
    assert got["second"] == 90 / 4096.0                                 # the 3 x 3 around the best does not count
    v = np.full((3, 3), 50)
    assert assert_pick_equal(lib, table(1, v))["second"] == INF         # nothing outside the 3 x 3
    assert assert_pick_equal(lib, table(0))["sub"] == (0.0, 0.0)


def test_the_pick_in_full_64_bit_range_and_on_the_cases_tables(lib):
    rng = np.random.default_rng(5)
    for S in (1, 4, 32):
        side = 2 * S + 1
        e = np.zeros((side, side), R.ENTRY)
        n = rng.integers(0, 1 << 28, (side, side))
        d = rng.integers(-(1 << 17), 1 << 17, (side, side))
        spread = rng.integers(0, 1 << 12, (side, side))
        e["n"], e["sum"] = n, n * d
        e["sumSq"] = (n * (d * d + spread)).astype(np.uint64)            # up to 2^62: beyond the 53 bits of a double
        for min_overlap in (0, 1 << 27):
            assert assert_pick_equal(lib, e, scale=37.5, stride=2, center=(3, -7), min_overlap=min_overlap) is not None
    moving, reference = C.pair(130, 35)
    for p in C.PARAMS:
        head, entries = R.search(moving, reference, C.SCALE, **p)
        for min_overlap in (0, 500):
            assert_pick_equal(lib, entries, C.SCALE, p.get("stride", 1), p.get("center", (0, 0)), min_overlap)
    moving, reference, scale = C.shifted_truth(C.SCENE_SHIFTS[0])
    _, entries = R.search(moving, reference, scale, radius=C.SCENE_RADIUS)
    assert assert_pick_equal(lib, entries, scale, min_overlap=C.SCENE_MIN_OVERLAP)["shift"] == C.SCENE_SHIFTS[0]


def test_the_pick_s_refusals(lib):
    e = table(2)
    untouched = Result(1, 2, 3.0, 4.0, 5.0, 6.0, 7.0, 8, 9)
    rc, out = c_pick(lib, e, params(radius=2), 101, out=untouched)     # no entry has that many cells
    assert rc == UNSUPPORTED and bytes(out) == bytes(Result(1, 2, 3.0, 4.0, 5.0, 6.0, 7.0, 8, 9))
    assert c_pick(lib, np.zeros((5, 5), R.ENTRY), params(radius=2), 0)[0] == UNSUPPORTED    # minOverlap 0 still asks for one cell
    assert R.pick(np.zeros((5, 5), R.ENTRY), 64.0) is None
    for bad in (params(radius=1), params(radius=3), params(radius=33)):  # the size disagrees with the radius
        rc, out = c_pick(lib, e, bad, 0, out=untouched)
        assert rc == INVALID_ARG and out.n == 8
    for bad in (params(scale=0.0, radius=2), params(scale=NAN, radius=2), params(scale=INF, radius=2), params(scale=-1.0, radius=2), params(stride=0, radius=2),
                params(center=((1 << 24) + 1, 0), radius=2), params(center=(0, -(1 << 24) - 1), radius=2), params(center_q=(1 << 18) + 1, radius=2)):
        assert c_pick(lib, e, bad, 0)[0] == INVALID_ARG
    raw = R.table_bytes(np.zeros((), R.HEAD), e)
    p, out = params(radius=2), Result()
    assert lib.ssrlcv_shift_pick_host(None, csz(raw.size), ctypes.byref(p), u32(0), ctypes.byref(out)) == INVALID_ARG
    assert lib.ssrlcv_shift_pick_host(raw.ctypes.data_as(vp), csz(raw.size), None, u32(0), ctypes.byref(out)) == INVALID_ARG
    assert lib.ssrlcv_shift_pick_host(raw.ctypes.data_as(vp), csz(raw.size), ctypes.byref(p), u32(0), None) == INVALID_ARG
    assert lib.ssrlcv_shift_pick_host(raw.ctypes.data_as(vp), csz(raw.size - 1), ctypes.byref(p), u32(0), ctypes.byref(out)) == INVALID_ARG
    assert c_pick(lib, e, params(radius=2, center=(1 << 24, -(1 << 24)), center_q=-(1 << 18), stride=0xFFFFFFFF), 0)[0] == OK   # the limits are legal


def test_search_refusals_in_the_contract_s_order(lib):
    null_all = dict(moving=None, reference=None, table=None, ws=None)
    bad = [None, params(scale=0.0), params(scale=-1.0), params(scale=NAN), params(scale=INF), params(stride=0), params(radius=33),
           params(radius=0xFFFFFFFF), params(center=((1 << 24) + 1, 0)), params(center=(0, -(1 << 24) - 1)), params(center_q=(1 << 18) + 1),
           params(center_q=-(1 << 18) - 1)]
    for p in bad:                                                        # the parameters before everything
        assert search(lib, p=p) == INVALID_ARG
        assert search(lib, p=p, w=(1 << 24) + 1) == INVALID_ARG and search(lib, p=p, w=0, **null_all) == INVALID_ARG
    sizes = [dict(w=(1 << 24) + 1, h=1), dict(w=1, h=(1 << 24) + 1), dict(w=1 << 14, h=(1 << 14) + 1), dict(w=0xFFFFFFFF, h=0)]   # the sizes before the buffers
    for size in sizes:
        assert search(lib, **size) == UNSUPPORTED and search(lib, **size, **null_all) == UNSUPPORTED
    assert search(lib, w=1 << 15, h=1 << 15, p=params(stride=1)) == UNSUPPORTED         # 2^30 sampled cells ...
    assert search(lib, w=1 << 15, h=1 << 15, p=params(stride=2)) == WORKSPACE           # ... 2^28 at stride 2
    assert search(lib, w=1 << 24, h=1 << 24, p=params(stride=1 << 10)) == WORKSPACE
    for empty in (dict(w=0), dict(h=0), dict(w=0, h=0)):                # a NULL table before the empty grid's table of zeros
        assert search(lib, table=None, **empty) == INVALID_ARG
    assert search(lib, table=BOGUS + 4) == INVALID_ARG and search(lib, table=BOGUS + 4, w=0) == INVALID_ARG   # not 8-byte aligned
    for null in ("moving", "reference", "ws"):
        assert search(lib, **{null: None}) == INVALID_ARG, null         # a NULL buffer before a short workspace
    want = lib.ssrlcv_hip_shift_search_workspace_bytes(u32(64), u32(48), ctypes.byref(params()))
    assert want == 2 * a256(4 * 64 * 48)
    assert search(lib, ws_bytes=want - 1) == WORKSPACE and search(lib, ws_bytes=0) == WORKSPACE
    legal = [dict(p=params(radius=0)), dict(p=params(radius=32)), dict(p=params(stride=0xFFFFFFFF)), dict(p=params(center=(1 << 24, -(1 << 24)))),
             dict(p=params(center_q=1 << 18)), dict(p=params(center_q=-(1 << 18), gate_q=0)), dict(p=params(scale=1e-30)), dict(p=params(scale=3.4e38)),
             dict(w=1, h=1), dict(w=1 << 24, h=16), dict(w=1 << 14, h=1 << 14)]
    for kw in legal:
        assert search(lib, **kw) == WORKSPACE, kw                        # accepted up to the size check


def test_the_queries_follow_the_header(lib):
    for S in (0, 1, 7, 8, 32):
        assert lib.ssrlcv_shift_table_bytes(u32(S)) == 16 + 24 * (2 * S + 1) ** 2
    assert lib.ssrlcv_shift_table_bytes(u32(33)) == 0 and lib.ssrlcv_shift_table_bytes(u32(0xFFFFFFFF)) == 0
    query = lambda w, h, p: lib.ssrlcv_hip_shift_search_workspace_bytes(u32(w), u32(h), ctypes.byref(p) if p is not None else None)  # noqa: E731
    for (w, h) in ((1, 1), (63, 5), (257, 131), (4096, 4096), (1 << 24, 16), (16384, 16384)):
        for g in (1, 2, 3, 5, 1000, 0xFFFFFFFF):
            assert query(w, h, params(stride=g)) == 2 * a256(4 * (-(-w // g)) * (-(-h // g))), (w, h, g)
    for (w, h, p) in ((0, 9, params()), (9, 0, params()), ((1 << 24) + 1, 1, params()), (1 << 15, 1 << 15, params()), (64, 64, None), (64, 64, params(stride=0)),
                      (64, 64, params(radius=33)), (64, 64, params(scale=NAN))):
        assert query(w, h, p) == 0


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/shift_test"])
    r = subprocess.run([os.path.join(host, "_build", "shift_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("static ShiftSearch searchShift(", "ssrlcv_hip_shift_search(", "ssrlcv_shift_pick_host(", "const ssrlcv_register_pose& start"):
        assert member in factory, member


def test_the_library_has_one_path_and_the_documents_exist():
    root = H.ROOT
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "shift.hip")).read()
    assert "getenv" not in source and "svdev::" not in source                          # no developer switch
    assert "atomicAdd(float" not in source and "double" not in source[:source.index("// ---- host side")]   # integer kernels
    assert "shift.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_shift_search" in open(os.path.join(root, doc)).read(), doc
    assert "shift_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_shift.py")) and "bench_shift.py" in open(os.path.join(root, "tools", "README.md")).read()
