"""The surface simplification, the part that needs no GPU: the header, the loader and the binders name the entry points, every
refusal of include/ssrlcv_hip.h "surface simplification" is decided on the host in the contract's order before a buffer is looked
at (the device pointers here are bogus or null, so nothing is launched), the workspace query follows the header's formula, and the
C++ mirror program compiles."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERY = "ssrlcv_hip_dsm_simplify_mesh_workspace_bytes"
NAMES = [QUERY, "ssrlcv_hip_dsm_simplify_errors", "ssrlcv_hip_dsm_simplify_mesh"]
OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BOGUS = 0x10  # a "device pointer" nothing may dereference
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, QUERY).restype = csz
    return lb


def a256(n):
    return (n + 255) // 256 * 256


def compaction(n):
    """the header's c(N)"""
    return a256(4 * (4 * ((n + 4095) // 4096) + 3))


def errors(lib, w=64, h=48, height=BOGUS, error=BOGUS + 0x1000):
    return lib.ssrlcv_hip_dsm_simplify_errors(vp(height), u32(w), u32(h), vp(error), vp(None))


def mesh(lib, w=64, h=48, tol=0.5, height=BOGUS, error=BOGUS + 0x1000, node_index=BOGUS + 0x2000, vertex_index=BOGUS + 0x3000, out=BOGUS + 0x4000,
         cap=100, tri_count=BOGUS + 0x5000, kept=BOGUS + 0x6000, kept_cap=100, vertex_count=BOGUS + 0x7000, ws=BOGUS + 0x8000, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_dsm_simplify_mesh(vp(height), vp(error), u32(w), u32(h), f32(tol), vp(node_index), vp(vertex_index), vp(out), u32(cap),
                                            vp(tri_count), vp(kept), u32(kept_cap), vp(vertex_count), vp(ws), csz(ws_bytes), vp(None))


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    render_at, at = header.index("int ssrlcv_hip_image_residual("), header.index("---- surface simplification")
    end = header.index("int ssrlcv_sift_plan_overflow")
    assert render_at < at < end                                                    # behind "mesh render"
    section = re.sub(r"\n \*\s+", " ", header[at:end])
    for text in ("0x7FC00000", "2^L >= max(w - 1, h - 1, 1)", "tz(0) = infinity", "k < L", "t = 2 (L - k - 1)", "I + J is even",
                 "mid = (h(a) + h(b)) * 0.5f", "fabsf(h(m) - mid)", "a NaN becomes +inf", "[+0, +inf]", "never a NaN and never -0",
                 "E(m) <= tol and (t(m) == 0 or !(E(c) <= tol))", "L == 0 or !(E(c) <= tol)", "(2j + 1, 2i + 1)", "truncation contract",
                 "whether or not that triangle fit", "strictly ascending", "(2L - t) tol", "2^-22 max|h|", "the only accuracy promise",
                 "147 on 20 x 34", "46 on 17 x 12", "perimeter term", "w h > 2^29", "2 w (2h - 1)", "c(2 w (2h - 1)) + c(w h)",
                 "Every entry has one writer", "No atomics at all", "bit-equal run to run"):
        assert text in section, text
    scope = section[section.index("Out of scope:"):]
    for text in ("maxJump cuts", "3-D or along the normal", "quadric decimation", "ssrlcv_hip_mesh_render", "normals recomputed",
                 "texture coordinates", "tiling the domain"):
        assert text in scope, text
    assert _lib.ABI_VERSION == 4                                                   # additions keep the number
    sig = inspect.signature
    assert list(sig(capi.dsm_simplify_errors).parameters) == ["height_d", "out"]
    assert list(sig(capi.dsm_simplify_mesh).parameters)[:4] == ["height_d", "error_d", "tolerance", "node_index_d"]
    assert list(sig(pipeline.surface_simplify).parameters)[:5] == ["model_or_height", "frame", "tolerance", "errors", "colors"]


def test_errors_refusals_in_the_contract_s_order(lib):
    assert errors(lib, w=65536, h=32768) == INVALID_ARG and errors(lib, w=65536, h=32768, height=None) == INVALID_ARG
    assert errors(lib, w=(1 << 29) + 1, h=1) == UNSUPPORTED and errors(lib, w=(1 << 29) + 1, h=1, error=None) == UNSUPPORTED
    assert errors(lib, w=(1 << 30), h=0) == OK and errors(lib, w=(1 << 31), h=0) == OK   # w h is 0: a size the limits take
    for empty in (dict(w=0), dict(h=0)):
        assert errors(lib, height=None, error=None, **empty) == OK
    assert errors(lib, height=None) == INVALID_ARG and errors(lib, error=None) == INVALID_ARG


def test_mesh_refusals_in_the_contract_s_order(lib):
    for tol in (NAN, INF, -INF):
        assert mesh(lib, tol=tol) == INVALID_ARG
        assert mesh(lib, tol=tol, w=(1 << 29) + 1, h=1, tri_count=None) == INVALID_ARG   # the tolerance before everything
    assert mesh(lib, w=65536, h=32768) == INVALID_ARG and mesh(lib, w=65536, h=32768, tri_count=None, ws=None) == INVALID_ARG
    assert mesh(lib, w=(1 << 29) + 1, h=1) == UNSUPPORTED and mesh(lib, w=16385, h=32768, tri_count=None) == UNSUPPORTED   # the size before the counts
    assert mesh(lib, tri_count=None) == INVALID_ARG and mesh(lib, vertex_count=None) == INVALID_ARG
    assert mesh(lib, w=0, tri_count=None) == INVALID_ARG and mesh(lib, h=0, vertex_count=None) == INVALID_ARG   # an empty map still needs them
    for null in ("height", "error", "vertex_index", "ws", "out", "kept"):
        assert mesh(lib, **{null: None}) == INVALID_ARG, null
        assert mesh(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null          # a NULL buffer before a short workspace
    want = getattr(lib, QUERY)(u32(64), u32(48))
    assert want == compaction(2 * 64 * (2 * 48 - 1)) + compaction(64 * 48)
    assert mesh(lib, ws_bytes=want - 1) == WORKSPACE and mesh(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(tol=-1.0), dict(tol=-3.0e38), dict(tol=3.4028234e38), dict(tol=0.0), dict(node_index=None), dict(out=None, cap=0),
                  dict(kept=None, kept_cap=0), dict(w=1, h=1), dict(w=1 << 29, h=1), dict(w=16384, h=32768)):
        assert mesh(lib, ws_bytes=0, **legal) == WORKSPACE, legal                  # accepted up to the size check


def test_the_workspace_query_follows_the_header(lib):
    query = getattr(lib, QUERY)
    for (w, h) in ((1, 1), (2, 2), (63, 5), (257, 131), (4096, 4096), (1 << 29, 1), (1, 1 << 29), (16384, 32768)):
        assert query(u32(w), u32(h)) == compaction(2 * w * (2 * h - 1)) + compaction(w * h), (w, h)
    for (w, h) in ((65536, 32768), ((1 << 29) + 1, 1), (16385, 32768), (0, 9), (9, 0)):
        assert query(u32(w), u32(h)) == 0, (w, h)


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/simplify_test"])
    r = subprocess.run([os.path.join(host, "_build", "simplify_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("unsigned long simplifySurface(float tolerance)", "ssrlcv_hip_dsm_simplify_errors(", "ssrlcv_hip_dsm_simplify_mesh(",
                   'refusesSimplified("computeSurfaceNormals")', 'refusesSimplified("renderView")', 'refusesSimplified("photoConsistency")',
                   "if (hasSimplified) return simplifiedFaces;"):
        assert member in factory, member


def test_the_library_has_one_path_and_the_documents_exist():
    root = H.ROOT
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "simplify.hip")).read()
    assert "getenv" not in source and "svdev::" not in source                      # no developer switch
    assert "atomicMax(" not in source and "atomicAdd" not in source                 # one writer an entry: no counter, no float atomics
    assert "simplify.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_dsm_simplify_errors" in open(os.path.join(root, doc)).read(), doc
    assert "simplify_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_simplify.py"))
