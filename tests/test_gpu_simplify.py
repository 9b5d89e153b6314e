"""The surface simplification on the GPU (ssrlcv_hip_dsm_simplify_errors, _dsm_simplify_mesh; include/ssrlcv_hip.h "surface
simplification") against the numpy restatement of the contract (tests/simplify_ref.py) on the cases of tests/simplify_cases.py
(tests/test_simplify_cases.py holds the restatement to a plain bintree walk without a GPU).  Every comparison is exact: the error
map as bit patterns, vertexIndex, both counts, `kept` and the triangle records in order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import simplify_cases as C
import simplify_ref as R
from test_gpu_dsm import GUARD, PATTERN, Guarded, cframe

pytestmark = pytest.mark.gpu

u32, f32c, vp, csz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
_REF = {}


def reference(name, height):
    """(error map, node index, {tolerance: mesh}) of a case from the restatement, computed once and shared; never modified"""
    if name not in _REF:
        err = R.errors(height)
        index = R.full_node_index(height)
        _REF[name] = (err, index, {tol: R.mesh(height, err, tol, index) for tol in C.tolerances(err)})
    return _REF[name]


def map_d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def errors_call(capi, height):
    """-> the error map's bits (h, w), written between guard words"""
    h, w = height.shape
    out = Guarded(w * h)
    capi.check(capi.LIB.ssrlcv_hip_dsm_simplify_errors(vp(map_d(height).data_ptr()), u32(w), u32(h), out.ptr, capi.stream_ptr()))
    return out.result().view(np.uint32).reshape(h, w)


def mesh_call(capi, height, err, tol, index=None, capacity=None, kept_capacity=None, fill=0xFF):
    """the call with guard words around every output and behind a workspace pre-filled with `fill`; capacity 0 passes NULL
    -> dict(faces (min(count, capacity), 3), n_faces, kept, n_vertices, vertex_index (h, w)), all uint32"""
    h, w = height.shape
    cap = 2 * max(w - 1, 0) * max(h - 1, 0) if capacity is None else capacity
    kcap = w * h if kept_capacity is None else kept_capacity
    need = int(capi.LIB.ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(u32(w), u32(h)))
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    h_d, e_d, i_d = map_d(height), map_d(err), None if index is None else map_d(index.view(np.int32))
    vi, out, kept, counts = Guarded(w * h), Guarded(3 * cap), Guarded(kcap), Guarded(2)
    capi.check(capi.LIB.ssrlcv_hip_dsm_simplify_mesh(vp(h_d.data_ptr()), vp(e_d.data_ptr()), u32(w), u32(h), f32c(tol), vp(i_d.data_ptr() if i_d is not None else 0),
                                                     vi.ptr, out.ptr if cap else vp(0), u32(cap), counts.ptr, kept.ptr if kcap else vp(0), u32(kcap),
                                                     vp(counts.ptr.value + 4), vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    nt, nv = (int(c) for c in counts.result().view(np.uint32))
    faces, keep = out.result().view(np.uint32).reshape(cap, 3), kept.result().view(np.uint32)
    assert (faces[min(nt, cap):] == PATTERN).all() and (keep[min(nv, kcap):] == PATTERN).all(), "an entry behind the count was written"
    return {"faces": faces[:min(nt, cap)], "n_faces": nt, "kept": keep[:min(nv, kcap)], "n_vertices": nv,
            "vertex_index": vi.result().view(np.uint32).reshape(h, w)}


def assert_mesh(got, want, what, capacity=None, kept_capacity=None):
    nt, nv = len(want["faces"]), len(want["kept"])
    assert (got["n_faces"], got["n_vertices"]) == (nt, nv), (what, got["n_faces"], got["n_vertices"], nt, nv)
    assert np.array_equal(got["vertex_index"], want["vertex_index"]), what
    assert np.array_equal(got["faces"], want["faces"][:nt if capacity is None else min(nt, capacity)]), what
    assert np.array_equal(got["kept"], want["kept"][:nv if kept_capacity is None else min(nv, kept_capacity)]), what


def _groups():
    """the contents, white noise -- which runs every size -- one group a width"""
    for name, (_, sizes) in C.CONTENTS.items():
        if name == "noise":
            for w in sorted({s[0] for s in sizes}):
                yield pytest.param(name, w, id="%s-w%d" % (name, w))
        else:
            yield pytest.param(name, None, id=name)


@pytest.mark.parametrize("content,width", list(_groups()))
def test_errors_and_meshes_equal_the_restatement(capi, content, width):
    ran = 0
    for name, height in C.cases((content,)):
        if width is not None and height.shape[1] != width:
            continue
        err, index, meshes = reference(name, height)
        got = errors_call(capi, height)
        ne = got != err.view(np.uint32)
        assert not ne.any(), "%s: the error differs at %d nodes, first (y, x) %s" % (name, int(ne.sum()), tuple(np.argwhere(ne)[0]))
        for tol, want in meshes.items():
            assert_mesh(mesh_call(capi, height, err, tol, index), want, (name, tol))
        ran += 1
    assert ran


def test_the_spikes_reach_the_root_through_every_level(capi):
    """the cases above already compare every node; this names what they must show: on the size whose levels run both as launches
    of their own and in the one-block tail the spike's error stands at every ancestor up to the domain's centre"""
    w, h = C.UPPER
    for content in ("spike_tile_corner", "spike_tile_edge", "spike_tile_interior"):
        height = C.CONTENTS[content][0](w, h)
        got = errors_call(capi, height).view(np.float32)
        assert got[h // 2, w // 2] > 0 and np.isfinite(got[h // 2, w // 2]), content
        assert np.array_equal(got.view(np.uint32), R.errors(height).view(np.uint32)), content


def test_without_a_node_index_kept_holds_raster_indices(capi):
    for name, height in C.cases(("holes",)):
        err, _, _ = reference(name, height)
        tol = C.tolerances(err)[2]
        assert_mesh(mesh_call(capi, height, err, tol), R.mesh(height, err, tol), name)


@pytest.mark.parametrize("content,size", [("relief", (C.TILE + 2, 2 * C.TILE + 1)), ("holes", (2 * C.TILE + 3, 2 * C.TILE + 3)), ("noise", (5, 3))])
def test_truncation(capi, content, size):
    w, h = size
    name, height = "%s-%dx%d" % (content, w, h), C.CONTENTS[content][0](w, h)
    err, index, meshes = reference(name, height)
    for tol in C.tolerances(err)[1:3]:
        want = meshes[tol]
        nt, nv = len(want["faces"]), len(want["kept"])
        assert nt > 1 and nv > 1, name
        for cap, kcap in ((0, 0), (nt - 1, nv - 1), (nt, nv), (0, nv), (nt, 0), (nt + 3, nv + 3)):
            assert_mesh(mesh_call(capi, height, err, tol, index, cap, kcap), want, (name, tol, cap, kcap), cap, kcap)


def test_two_calls_give_the_same_bytes_whatever_the_workspace_held(capi):
    for content, (w, h) in (("noise", C.UPPER), ("holes", (2 * C.TILE + 3, 2 * C.TILE + 3))):
        height = C.CONTENTS[content][0](w, h)
        first = errors_call(capi, height)
        assert np.array_equal(first, errors_call(capi, height))
        err = first.view(np.float32)
        tol = C.tolerances(err)[2]
        a, b, c = (mesh_call(capi, height, err, tol, None, fill=fill) for fill in (0xFF, 0xFF, 0x00))
        for other in (b, c):
            for key in ("faces", "kept", "vertex_index"):
                assert np.array_equal(a[key], other[key]), (content, key)
            assert (a["n_faces"], a["n_vertices"]) == (other["n_faces"], other["n_vertices"])


def test_an_empty_map_writes_two_zero_counts_and_nothing_else(capi):
    for w, h in ((0, 5), (5, 0), (0, 0)):
        counts = Guarded(2)
        capi.check(capi.LIB.ssrlcv_hip_dsm_simplify_mesh(vp(0), vp(0), u32(w), u32(h), f32c(0.5), vp(0), vp(0), vp(0), u32(7), counts.ptr, vp(0), u32(7),
                                                         vp(counts.ptr.value + 4), vp(0), csz(0), capi.stream_ptr()))
        assert counts.result().tolist() == [0, 0]
        capi.check(capi.LIB.ssrlcv_hip_dsm_simplify_errors(vp(0), u32(w), u32(h), vp(0), capi.stream_ptr()))


def _ply_counts(path):
    counts = {}
    with open(path, "rb") as f:
        for line in f:
            words = line.decode("ascii", "replace").split()
            if words[:1] == ["element"]:
                counts[words[1]] = int(words[2])
            if words[:1] == ["end_header"]:
                break
    return counts


def test_the_rendered_scene_s_model_is_simplified_within_the_bound(capi, tmp_path):
    """three pairs of the rendered rig -> surface model -> surface_simplify at a tolerance of one cell of height: the restatement's
    mesh, the deviation bound, the points gathered from dsm_points, and MeshFactory::simplifySurface + saveMesh"""
    import dsm_cases as DC
    import dsm_ref as D
    from ssrlcv_amd import pipeline
    from test_gpu_dsm import FUSE_ARGS, scene_clouds
    from test_simplify_cases import check_properties
    e, fr = scene_clouds(capi), DC.scene_frame()
    frame = cframe(capi, fr)
    model = pipeline.surface_model(e["clouds"], frame, rule="max", fuse=FUSE_ARGS)
    height = model["height"].cpu().numpy()
    tol = float(np.float32(fr.cell))
    full = pipeline.surface_mesh(model, frame, float("inf"))
    got = pipeline.surface_simplify(model, frame, tol, normals=full["normals"])
    err = R.errors(height)
    want = R.mesh(height, err, tol, R.full_node_index(height))
    assert np.array_equal(got["errors"].cpu().numpy().view(np.uint32), err.view(np.uint32))
    assert np.array_equal(got["faces"].cpu().numpy().view(np.uint32), want["faces"])
    assert np.array_equal(got["kept"].cpu().numpy().view(np.uint32), want["kept"])
    assert np.array_equal(got["vertex_index"].cpu().numpy().view(np.uint32), want["vertex_index"])
    worst = check_properties("scene", height, err, tol, want)       # asserts the header's bound, 2L (tol + 2^-22 max|h|)
    kept = want["kept"].astype(np.int64)
    assert np.array_equal(got["points"].cpu().numpy().view(np.uint32), D.bits(D.points(height, fr))[kept])
    assert np.array_equal(got["normals"].cpu().numpy().view(np.uint32), full["normals"].cpu().numpy().view(np.uint32).reshape(-1, 3)[kept])
    again = pipeline.surface_simplify(model, frame, 4 * tol, errors=got["errors"])     # the error map serves every tolerance
    assert 0 < len(again["faces"]) < len(got["faces"])
    n_full, t_full = len(full["points"]), len(full["faces"])
    print("rendered scene %d x %d at a tolerance of one cell (%.4f): %d of %d vertices, %d of %d triangles (%.1f %%), largest deviation %.4f, bound %.4f"
          % (fr.w, fr.h, tol, len(kept), n_full, len(want["faces"]), t_full, 100.0 * len(want["faces"]) / t_full, worst,
             2 * R.levels(fr.w, fr.h) * tol))
    # the class API
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/simplify_test"])
    frame_path, height_path = str(tmp_path / "frame.raw"), str(tmp_path / "height.raw")
    with open(frame_path, "wb") as f:
        f.write(bytes(frame))
    height.tofile(height_path)
    out = subprocess.check_output([os.path.join(host, "_build", "simplify_test"), frame_path, height_path, "%.9g" % tol, str(tmp_path) + os.sep, "thin"],
                                  timeout=120).decode()
    lines = out.splitlines()
    assert lines[-1] == "ok", out
    assert "vertices %d faces %d" % (len(kept), len(want["faces"])) in lines, out
    assert _ply_counts(str(tmp_path / "thin.ply")) == {"vertex": len(kept), "face": len(want["faces"])}
    assert np.array_equal(np.fromfile(str(tmp_path / "thin.faces"), np.uint32).reshape(-1, 3), want["faces"])
