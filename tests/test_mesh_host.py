"""The disparity mesh, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "disparity mesh" is decided on the host in the contract's order before a buffer is looked at (the device
pointers here are bogus or null, so nothing is launched), the workspace queries follow the header's formulas, the C++ mirror
program compiles, and the PLY writer with faces round-trips bit for bit."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERIES = ["ssrlcv_hip_disparity_mesh_workspace_bytes", "ssrlcv_hip_mesh_select_workspace_bytes", "ssrlcv_hip_mesh_triangles_workspace_bytes"]
NAMES = QUERIES + ["ssrlcv_hip_disparity_mesh", "ssrlcv_hip_mesh_select", "ssrlcv_hip_mesh_triangles", "ssrlcv_hip_mesh_normals"]
OK, INVALID_ARG, WORKSPACE = 0, -1, -3
BOGUS = 0x10  # a "device pointer" nothing may dereference
INF, NAN = float("inf"), float("nan")


class Params(ctypes.Structure):
    _fields_ = [("step", u32), ("maxJump", f32)]


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


def grid(w, h, step):
    return ((w - 1) // step + 1 if w else 0), ((h - 1) // step + 1 if h else 0)


def mesh(lib, w=64, h=48, step=1, max_jump=1.0, params=True, d=BOGUS, vi=BOGUS + 0x1000, cells=BOGUS + 0x2000, count=BOGUS + 0x3000, ws=BOGUS + 0x4000,
         ws_bytes=1 << 50):
    p = ctypes.byref(Params(step, max_jump)) if params else None
    return lib.ssrlcv_hip_disparity_mesh(vp(d), u32(w), u32(h), p, vp(vi), vp(cells), vp(count), vp(ws), csz(ws_bytes), vp(None))


def need(lib, w, h, step=1, max_jump=1.0, params=True):
    p = ctypes.byref(Params(step, max_jump)) if params else None
    return lib.ssrlcv_hip_disparity_mesh_workspace_bytes(u32(w), u32(h), p)


def triangles(lib, gw=64, gh=48, vi=BOGUS, cells=BOGUS + 0x1000, out=BOGUS + 0x2000, cap=100, count=BOGUS + 0x3000, ws=BOGUS + 0x4000, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_mesh_triangles(vp(vi), vp(cells), u32(gw), u32(gh), vp(out), u32(cap), vp(count), vp(ws), csz(ws_bytes), vp(None))


def select(lib, gw=64, gh=48, n=1000, m=10, vi=BOGUS, cells=BOGUS + 0x1000, kept=BOGUS + 0x2000, ws=BOGUS + 0x3000, ws_bytes=1 << 50):
    return lib.ssrlcv_hip_mesh_select(vp(vi), vp(cells), u32(gw), u32(gh), u32(n), vp(kept), u32(m), vp(ws), csz(ws_bytes), vp(None))


def normals(lib, gw=64, gh=48, n=1000, points=BOGUS, vi=BOGUS + 0x1000, cells=BOGUS + 0x2000, out=BOGUS + 0x3000):
    return lib.ssrlcv_hip_mesh_normals(vp(points), u32(n), vp(vi), vp(cells), u32(gw), u32(gh), vp(out), vp(None))


BAD_PARAMS = [dict(params=False), dict(step=0), dict(max_jump=-1.0), dict(max_jump=-1e-45), dict(max_jump=NAN), dict(max_jump=-INF)]


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED, name
        assert hasattr(_lib.load(), name), name
    assert _lib.ABI_VERSION == 4 and "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.load().ssrlcv_hip_abi_version() == 4
    fill_at, mesh_at = header.index("int ssrlcv_hip_stereo_fill_holes("), header.index("---- disparity mesh")
    assert fill_at < mesh_at < header.index("int ssrlcv_sift_plan_overflow")         # behind hole filling, before the overflow section
    section = re.sub(r"\n \*\s+", " ", header[mesh_at:header.index("int ssrlcv_hip_mesh_normals(")])   # the comment's line breaks are not part of the text
    for item in ("0x7FC00000", "x % step == 0", "(w - 1) / step + 1", "raster order", "UINT32_MAX", "fabsf(d(p) - d(q)) <= maxJump", "inf - inf",
                 "fabsf(d(b) - d(c)) < fabsf(d(a) - d(d))", "T0 = (a, c, d)", "T1 = (a, d, b)", "T0 = (a, c, b)", "T1 = (b, c, d)", "bit 2 = the diagonal is b-c",
                 "negative z", "min(count, capacity)", "out[3 capacity)", "(u.y v.z) - (u.z v.y)", "sqrtf(((s.x s.x) + (s.y s.y)) + (s.z s.z))",
                 "strictly ascending", "nothing is re-triangulated", "!(maxJump >= 0)", "a256(4 (4 ceil(N / 4096) + 3))", "a256(4 nVertices)",
                 "no atomics", "bit-equal run to run", "welding", "texture coordinates", "Poisson", "several pairs",
                 "uint32_t step;", "float maxJump;", "ssrlcv_mesh_params; /* 8 bytes */"):
        assert item in section, item
    assert ctypes.sizeof(capi.MeshParams) == 8 and [f[0] for f in capi.MeshParams._fields_] == ["step", "maxJump"]
    sig = inspect.signature
    assert list(sig(capi.disparity_mesh).parameters) == ["disp_d", "step", "max_jump"]
    assert list(sig(capi.mesh_select).parameters) == ["vertex_index_d", "cells_d", "n_vertices", "kept_index_d"]
    assert list(sig(capi.mesh_triangles).parameters) == ["vertex_index_d", "cells_d", "capacity"]
    assert list(sig(capi.mesh_normals).parameters) == ["points_d", "vertex_index_d", "cells_d", "out"]
    p = sig(pipeline.disparity_mesh).parameters
    assert list(p) == ["disp", "step", "max_jump"] and (p["step"].default, p["max_jump"].default) == (1, None)
    assert list(sig(pipeline.mesh_select).parameters) == ["mesh", "kept_index"] and list(sig(pipeline.mesh_faces).parameters) == ["mesh"]
    assert list(sig(pipeline.mesh_normals).parameters) == ["mesh", "points"]
    # the cloud functions' arguments plus max_jump
    cloud, surf = list(sig(pipeline.stereo_cloud).parameters), list(sig(pipeline.stereo_mesh).parameters)
    assert surf == cloud[:-1] + ["max_jump", cloud[-1]] and sig(pipeline.stereo_mesh).parameters["max_jump"].default is None
    cloud, surf = list(sig(pipeline.stereo_cloud_cameras).parameters), list(sig(pipeline.stereo_mesh_cameras).parameters)
    assert surf == cloud[:-1] + ["max_jump", cloud[-1]]
    assert cloud == ["left", "right", "cam_l", "cam_r", "step", "sgm", "post", "disparity_args"]                  # unchanged
    with pytest.raises(TypeError, match="no cost map"):
        pipeline.stereo_mesh_cameras(None, None, None, None, want_cost=True)                # before anything is touched


def test_parameters_then_the_size_then_the_buffers_then_the_workspace(lib):
    for bad in BAD_PARAMS:
        assert mesh(lib, **bad) == INVALID_ARG, bad
        assert mesh(lib, w=65536, h=32768, d=None, count=None, **bad) == INVALID_ARG, bad
    assert mesh(lib, w=65536, h=32768) == INVALID_ARG                                        # w h = 2^31
    assert mesh(lib, w=65536, h=32768, d=None, ws_bytes=0) == INVALID_ARG
    for null in ("d", "vi", "cells", "count", "ws"):
        assert mesh(lib, **{null: None}) == INVALID_ARG, null
        assert mesh(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null                    # a NULL buffer before a short workspace
    assert mesh(lib, w=0, count=None) == INVALID_ARG and mesh(lib, h=0, count=None) == INVALID_ARG   # an empty map still needs the count
    want = need(lib, 64, 48)
    assert want == compaction(64 * 48)
    assert mesh(lib, ws_bytes=want - 1) == WORKSPACE and mesh(lib, ws_bytes=0) == WORKSPACE
    for legal in (dict(max_jump=0.0), dict(max_jump=-0.0), dict(max_jump=INF), dict(step=7), dict(step=0xFFFFFFFF), dict(max_jump=1e-45)):
        assert mesh(lib, ws_bytes=0, **legal) == WORKSPACE, legal                            # accepted up to the size check
    # cells may be NULL when it has no element: gw or gh below 2
    assert mesh(lib, w=1, h=48, cells=None, ws_bytes=0) == WORKSPACE and mesh(lib, w=64, h=1, cells=None, ws_bytes=0) == WORKSPACE
    assert mesh(lib, step=64, cells=None, ws_bytes=0) == WORKSPACE and mesh(lib, step=47, cells=None, ws_bytes=0) == INVALID_ARG
    assert mesh(lib, w=65536, h=32767, ws_bytes=0) == WORKSPACE                              # just below 2^31 pixels


def test_the_other_calls_refuse_the_size_then_null_buffers_then_a_short_workspace(lib):
    big = dict(gw=65536, gh=32768)
    assert triangles(lib, **big) == INVALID_ARG and select(lib, **big) == INVALID_ARG and normals(lib, **big) == INVALID_ARG
    for null in ("vi", "cells", "out", "count", "ws"):
        assert triangles(lib, **{null: None}) == INVALID_ARG, null
        assert triangles(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null
    want = lib.ssrlcv_hip_mesh_triangles_workspace_bytes(u32(64), u32(48))
    assert want == compaction(2 * 63 * 47)
    assert triangles(lib, ws_bytes=want - 1) == WORKSPACE and triangles(lib, out=None, cap=0, ws_bytes=0) == WORKSPACE   # out may be NULL with capacity 0
    assert triangles(lib, gw=65536, gh=32767, ws_bytes=0) == WORKSPACE
    for null in ("vi", "cells", "kept", "ws"):
        assert select(lib, **{null: None}) == INVALID_ARG, null
        assert select(lib, ws_bytes=0, **{null: None}) == INVALID_ARG, null
    assert select(lib, ws_bytes=a256(4000) - 1) == WORKSPACE and select(lib, kept=None, m=0, ws_bytes=0) == WORKSPACE    # keptIndex may be NULL with m 0
    assert select(lib, gw=1, cells=None, ws_bytes=0) == WORKSPACE                               # no cell: cells may be NULL
    assert select(lib, gw=0, vi=None, cells=None, kept=None, ws=None, ws_bytes=0) == OK       # no node: nothing to do
    for null in ("points", "vi", "cells", "out"):
        assert normals(lib, **{null: None}) == INVALID_ARG, null
    assert normals(lib, n=0, points=None, out=None) == OK and normals(lib, gw=0, vi=None, cells=None) == OK       # no vertex to write


def test_the_workspace_queries_follow_the_headers_formulas(lib):
    for w, h in [(1, 1), (1, 37), (41, 1), (2, 2), (64, 64), (65, 63), (97, 83), (1024, 1024), (4096, 4096), (65536, 32767), (1, 2 ** 31 - 1), (0, 5), (5, 0)]:
        for step in (1, 2, 3, 5, 64, 0xFFFFFFFF):
            gw, gh = grid(w, h, step)
            assert need(lib, w, h, step) == compaction(gw * gh), (w, h, step)
    assert need(lib, 4096, 4096) == a256(4 * (4 * 4096 + 3)) == 65792 and need(lib, 64, 64) == need(lib, 65, 64) == 256
    assert need(lib, 65536, 32767) == compaction(65536 * 32767) == a256(4 * (4 * 524272 + 3))
    assert need(lib, 64, 48, max_jump=0.0) == need(lib, 64, 48, max_jump=INF) == need(lib, 64, 48)
    for w, h in ((65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF), (2 ** 31, 1)):
        assert need(lib, w, h) == 0                                                              # refused sizes
    for bad in BAD_PARAMS:
        assert need(lib, 64, 48, **bad) == 0, bad                                                # refused parameters
    tri = lib.ssrlcv_hip_mesh_triangles_workspace_bytes
    for gw, gh in [(0, 0), (1, 1), (1, 37), (41, 1), (2, 2), (33, 28), (97, 83), (4096, 4096), (65536, 32767), (2 ** 31 - 1, 1)]:
        cells = (gw - 1) * (gh - 1) if gw >= 2 and gh >= 2 else 0
        assert tri(u32(gw), u32(gh)) == compaction(2 * cells), (gw, gh)
    assert tri(u32(65536), u32(32768)) == 0 and tri(u32(0xFFFFFFFF), u32(0xFFFFFFFF)) == 0
    assert tri(u32(65536), u32(32767)) == compaction(2 * 65535 * 32766) > 1 << 22              # 2 (gw - 1) (gh - 1) above 2^32 would wrap: it is below
    sel = lib.ssrlcv_hip_mesh_select_workspace_bytes
    for n in (0, 1, 63, 64, 65, 8051, 2 ** 31 - 1, 0xFFFFFFFF):
        assert sel(u32(n)) == a256(4 * n), n                                                     # computed in size_t


def test_the_mirror_program_compiles_and_the_ply_writer_round_trips(tmp_path):
    """tests/cpp/mesh_grid_test.cpp includes ssrlcv.hpp, so DisparityFactory::generateMesh and MeshFactory's surface compile too"""
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/mesh_grid_test"])
    exe = os.path.join(host, "_build", "mesh_grid_test")
    out = subprocess.run([exe], stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and b"usage" in out.stderr        # no arguments: the usage line, no GPU touched
    assert subprocess.check_output([exe, "ply", str(tmp_path)], timeout=60).decode().splitlines()[-1] == "ok"
    f = np.float32
    points = np.array([[6371.00049, -0.1, 1e-7], [f(1.0) / f(3.0), 2.5, -3.25e5], [0.0, -0.0, 123456.789], [1e-40, 3.4e38, -1.17549435e-38], [0.1, 0.2, 0.3]], f)
    nrm = np.array([[0, 0, -1], [0.577350269, -0.577350269, 0.577350269], [0, 0, 0], [-0.267261242, 0.534522484, -0.801783726], [1, 0, 0]], f)
    lines = open(str(tmp_path / "fan.ply")).read().split("\n")
    end = lines.index("end_header")
    assert lines[:end] == ["ply", "format ascii 1.0", "comment author: SSRLCV simple PLY writer (MI355X build)", "element vertex 5", "property float x",
                           "property float y", "property float z", "property float nx", "property float ny", "property float nz", "element face 3",
                           "property list uchar int vertex_indices"]
    rows = np.array([[f(v) for v in line.split()] for line in lines[end + 1:end + 6]], f)
    assert rows[:, :3].tobytes() == points.tobytes() and rows[:, 3:].tobytes() == nrm.tobytes()   # 9 digits: bit for bit, -0 and a denormal included
    assert lines[end + 6:] == ["3 0 2 3", "3 0 3 1", "3 1 3 4", ""]
    bare = open(str(tmp_path / "bare.ply")).read().split("\n")
    assert "element face 0" in bare and "property float nx" not in bare and len(bare) == bare.index("end_header") + 1 + 5 + 1
    factory = open(os.path.join(host, "DisparityFactory.hpp")).read()
    assert "GridMesh generateMesh(ptr::value<Unity<float>> disparity, unsigned int meshStep, float maxJump)" in factory
    mesh_factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("void setSurface(const GridMesh& mesh)", "void computeSurfaceNormals()", "ptr::value<Unity<uint3>> faces()",
                   "void saveMesh(std::string filename, std::string dir = \"out/\")", "ssrlcv_hip_mesh_select(", "ssrlcv_hip_mesh_normals(",
                   "ssrlcv_hip_mesh_triangles("):
        assert member in mesh_factory, member
    assert "ssrlcv_hip_disparity_mesh(" in factory


def test_the_documents_describe_the_feature():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Disparity mesh" in design
    for kernel in ("k_mesh_cells", "k_mesh_normals", "k_select_cells", "k_select_nodes"):
        assert kernel in design, kernel
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ssrlcv_hip_disparity_mesh" in open(os.path.join(root, doc)).read(), doc
    assert "mesh_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_mesh.py"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "mesh.hip")).read()
    assert "atomic" not in source and "compact.h" in source        # the contract: no atomics; the ordered compactions are compact.h's
    assert "mesh.hip" in open(os.path.join(root, "ssrlcv_amd", "csrc", "Makefile")).read()
