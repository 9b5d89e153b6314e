"""The disparity mesh on the GPU (include/ssrlcv_hip.h "disparity mesh"; csrc/mesh.hip) against the numpy restatement of the
contract (tests/mesh_ref.py) on the cases of tests/mesh_cases.py (tests/test_mesh_cases.py proves without a GPU that they test
something).  Every comparison is exact: indices and cell bytes as integers, normals as bit patterns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fill_scene as S
import helpers as H
import mesh_cases as C
import mesh_ref as R

pytestmark = pytest.mark.gpu

NAMES = sorted(C.CASES)
u32, csz, vp = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p
GUARD = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases and references are read-only


def u32_of(t):
    return t.cpu().numpy().view(np.uint32)


def raw(t):
    return t.cpu().numpy().tobytes()


def assert_same(name, what, got, want):
    assert got.shape == want.shape, (name, what, got.shape, want.shape)
    ne = got != want
    assert not ne.any(), (name, "%s differs at %d of %d entries, first %s: got %s want %s" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4]))


def gpu_mesh(capi, name):
    k = C.CASES[name]
    vi, cells, count = capi.disparity_mesh(dev(k.d), k.step, k.max_jump)
    return vi, cells, int(count.item())


def select_faces(faces, n_vertices, kept):
    """item 6 on a face list: renumber through kept, drop the faces that lose a corner"""
    new_of = np.full(n_vertices + 1, -1, np.int64)
    kept = np.asarray(kept, np.int64)
    inside = kept < n_vertices
    new_of[kept[inside]] = np.nonzero(inside)[0]
    f = new_of[faces.astype(np.int64)]
    return f[(f >= 0).all(1)].astype(np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_equals_the_reference(capi, name):
    k, ref = C.CASES[name], C.reference(name)
    vi, cells, n = gpu_mesh(capi, name)
    assert n == ref["n"]
    assert_same(name, "vertex_index", u32_of(vi), ref["vertex_index"])
    assert_same(name, "cells", cells.cpu().numpy(), ref["cells"])
    faces, t = capi.mesh_triangles(vi, cells)
    assert t == len(ref["faces"]) == len(faces)
    assert_same(name, "faces", u32_of(faces), ref["faces"])
    normals = capi.mesh_normals(dev(ref["points"]), vi, cells)
    assert_same(name, "normals", u32_of(normals), ref["normals"].view(np.uint32))
    # the vertex numbering is the record order of stereo_matches for the same map and step
    records, count = capi.stereo_matches(dev(k.d), k.step)
    assert count == n
    rec = capi.to_host(records, H.MATCH, n)
    js, is_ = np.nonzero(u32_of(vi) != R.NONE)
    at = u32_of(vi)[js, is_]
    assert np.array_equal(rec["kp0_loc"][at, 0], (is_ * k.step).astype(np.float32)) and np.array_equal(rec["kp0_loc"][at, 1], (js * k.step).astype(np.float32))
    # bit-equal run to run
    vi2, cells2, n2 = gpu_mesh(capi, name)
    assert n2 == n and raw(vi2) == raw(vi) and raw(cells2) == raw(cells)
    assert raw(capi.mesh_triangles(vi2, cells2)[0]) == raw(faces) and raw(capi.mesh_normals(dev(ref["points"]), vi2, cells2)) == raw(normals)


@pytest.mark.parametrize("name", ["rand_97x83", "shape_3x2", "all_invalid"])
def test_the_triangle_list_is_truncated_at_the_capacity_and_nothing_behind_it_is_touched(capi, name):
    ref = C.reference(name)
    vi, cells, _ = gpu_mesh(capi, name)
    gh, gw = vi.shape
    t = len(ref["faces"])
    ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_mesh_triangles_workspace_bytes(u32(gw), u32(gh))))
    for cap in sorted({0, 1, max(t - 1, 0), t, t + 1}):
        buf = torch.full((3 * cap + 16,), GUARD, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        capi.check(capi.LIB.ssrlcv_hip_mesh_triangles(capi.ptr(vi), capi.ptr(cells), u32(gw), u32(gh), capi.ptr(buf), u32(cap), capi.ptr(count), capi.ptr(ws),
                                                      csz(ws.numel()), capi.stream_ptr()))
        got = u32_of(buf)
        m = min(t, cap)
        assert int(count.item()) == t, (name, cap)                                    # the full count
        assert np.array_equal(got[:3 * m].reshape(-1, 3), ref["faces"][:m]), (name, cap)
        assert (got[3 * m:] == GUARD).all(), (name, cap)                              # the unused slots and the guard words
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    capi.check(capi.LIB.ssrlcv_hip_mesh_triangles(capi.ptr(vi), capi.ptr(cells), u32(gw), u32(gh), vp(None), u32(0), capi.ptr(count), capi.ptr(ws),
                                                  csz(ws.numel()), capi.stream_ptr()))      # out may be NULL with capacity 0
    assert int(count.item()) == t


@pytest.mark.parametrize("name", ["rand_97x83", "rand_131x70_s2", "ramp", "shape_2x2"])
def test_select_equals_the_reference(capi, name):
    ref = C.reference(name)
    n = ref["n"]
    rng = np.random.default_rng(5)
    subsets = {"random": np.nonzero(rng.random(n) < 0.7)[0], "sparse": np.nonzero(rng.random(n) < 0.2)[0], "empty": np.zeros(0, np.int64),
               "identity": np.arange(n), "past_the_end": np.concatenate([np.nonzero(rng.random(n) < 0.8)[0], [n, n + 7, 0xFFFFFFFE]])}
    for what, kept in subsets.items():
        vi, cells, _ = gpu_mesh(capi, name)
        capi.mesh_select(vi, cells, n, dev(kept.astype(np.uint32).view(np.int32)))
        want_vi, want_cells = R.select(ref["vertex_index"], ref["cells"], n, kept)
        assert_same((name, what), "vertex_index", u32_of(vi), want_vi)
        assert_same((name, what), "cells", cells.cpu().numpy(), want_cells)
        faces = u32_of(capi.mesh_triangles(vi, cells)[0])
        assert_same((name, what), "faces", faces, R.faces(want_vi, want_cells))
        assert_same((name, what), "faces by renumbering the list", faces, select_faces(ref["faces"], n, kept))
        if what == "identity":
            assert np.array_equal(want_vi, ref["vertex_index"]) and np.array_equal(want_cells, ref["cells"])
        if what == "empty":
            assert (u32_of(vi) == R.NONE).all() and not cells.any() and len(faces) == 0


@pytest.mark.parametrize("name", ["rand_97x83", "ramp"])
def test_normals_of_fewer_points_than_vertices_stay_inside_their_rows(capi, name):
    ref = C.reference(name)
    vi, cells, n = gpu_mesh(capi, name)
    for fewer in (n // 2, 1, n - 1):
        out = torch.full((n + 4, 3), 7.5, dtype=torch.float32, device="cuda")
        got = capi.mesh_normals(dev(ref["points"][:fewer]), vi, cells, out=out).cpu().numpy()
        assert (got[fewer:] == 7.5).all(), (name, fewer)                                  # nothing outside normals[0 .. n)
        want = R.normals(ref["points"][:fewer], ref["vertex_index"], ref["cells"])
        assert_same((name, fewer), "normals", got[:fewer].view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(R.normals(ref["points"][:n // 2], ref["vertex_index"], ref["cells"]), ref["normals"][:n // 2])  # the rule bites


def test_an_empty_map_and_a_grid_without_a_cell_write_a_zero_count_and_look_at_nothing_else(capi):
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    p = capi.MeshParams(1, 1.0)
    for w, h in ((0, 5), (5, 0), (0, 0)):
        count.fill_(-1)
        capi.check(capi.LIB.ssrlcv_hip_disparity_mesh(vp(None), u32(w), u32(h), ctypes.byref(p), vp(None), vp(None), capi.ptr(count), vp(None), csz(0),
                                                      capi.stream_ptr()))
        assert int(count.item()) == 0, (w, h)
    for gw, gh in ((1, 1), (1, 37), (41, 1), (0, 0)):
        count.fill_(-1)
        capi.check(capi.LIB.ssrlcv_hip_mesh_triangles(vp(None), vp(None), u32(gw), u32(gh), vp(None), u32(0), capi.ptr(count), vp(None), csz(0),
                                                      capi.stream_ptr()))
        assert int(count.item()) == 0, (gw, gh)


def test_a_side_stream_without_host_synchronisation(capi):
    name = "rand_97x83"
    k, ref = C.CASES[name], C.reference(name)
    d, pts = dev(k.d), dev(ref["points"])
    kept = np.arange(0, ref["n"], 2)
    kept_d = dev(kept.astype(np.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vi, cells, count = capi.disparity_mesh(d, k.step, k.max_jump)
        normals = capi.mesh_normals(pts, vi, cells)
        vi2, cells2 = capi.mesh_select(vi.clone(), cells.clone(), ref["n"], kept_d)
    side.synchronize()
    assert_same(name, "normals", u32_of(normals), ref["normals"].view(np.uint32))
    want_vi, want_cells = R.select(ref["vertex_index"], ref["cells"], ref["n"], kept)
    assert_same(name, "vertex_index", u32_of(vi2), want_vi)
    assert_same(name, "cells", cells2.cpu().numpy(), want_cells)


def test_pipeline_functions_equal_the_c_abi_calls(capi):
    from ssrlcv_amd import pipeline
    name = "rand_131x70_s2"
    k, ref = C.CASES[name], C.reference(name)
    mesh = pipeline.disparity_mesh(dev(k.d), k.step, k.max_jump)
    assert mesh["n_vertices"] == ref["n"] and mesh["vertex_index"].dtype == torch.int32 and mesh["cells"].dtype == torch.uint8
    assert_same(name, "vertex_index", u32_of(mesh["vertex_index"]), ref["vertex_index"])
    assert_same(name, "faces", u32_of(pipeline.mesh_faces(mesh)), ref["faces"])
    assert_same(name, "normals", u32_of(pipeline.mesh_normals(mesh, dev(ref["points"]))), ref["normals"].view(np.uint32))
    default = pipeline.disparity_mesh(dev(k.d), k.step)                                   # max_jump None: float(step)
    assert_same(name, "cells at the default jump", default["cells"].cpu().numpy(), R.mesh(k.d, k.step, 2.0)[1])
    kept = np.arange(1, ref["n"], 3)
    sub = pipeline.mesh_select(mesh, dev(kept))                                           # int64, as filter_cloud's index is
    assert sub["n_vertices"] == len(kept) and raw(mesh["vertex_index"]) == ref["vertex_index"].tobytes()   # `mesh` is left as it is
    assert_same(name, "selected faces", u32_of(pipeline.mesh_faces(sub)), select_faces(ref["faces"], ref["n"], kept))


def scene_args():
    args = dict(S.ARGS)
    args["min_disparity"] = 1                          # with doffset 3.5 every d + doffset is above 0
    return args


def test_stereo_mesh_equals_stereo_cloud_and_the_reference_and_faces_the_camera(capi):
    from ssrlcv_amd import pipeline
    left, right = S.pair()
    left_d, right_d = dev(left), dev(right)
    post = dict(speckle_size=20, speckle_diff=1.0)
    out = pipeline.stereo_mesh(left_d, right_d, step=1, post=post, **S.CAMERA, **scene_args())
    pts, matches, n, disp = pipeline.stereo_cloud(left_d, right_d, step=1, post=post, **S.CAMERA, **scene_args())
    assert out["n"] == n > 1000 and raw(out["points"]) == raw(pts) and raw(out["matches"]) == raw(matches) and raw(out["disparity"]) == raw(disp)
    d = disp.cpu().numpy()
    vi, cells, nv = R.mesh(d, 1, 1.0)
    assert nv == n == out["mesh"]["n_vertices"]
    want = R.faces(vi, cells)
    assert len(want) > 1000
    assert_same("scene", "faces", u32_of(out["faces"]), want)
    p32 = pts.cpu().numpy()
    assert_same("scene", "normals", u32_of(out["normals"]), R.normals(p32, vi, cells).view(np.uint32))
    p = p32.astype(np.float64)
    f = want.astype(np.int64)
    normal = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert ((normal * p[f[:, 0]]).sum(1) < 0).all()                                       # every face's normal faces the camera
    nrm = out["normals"].cpu().numpy().astype(np.float64)
    used = np.unique(f)
    assert ((nrm[used] * p[used]).sum(1) < 0).all() and np.allclose(np.linalg.norm(nrm[used], axis=1), 1.0, atol=1e-6)
    coarse = pipeline.stereo_mesh(left_d, right_d, step=3, max_jump=2.0, **S.CAMERA, **scene_args())
    vi3, cells3, _ = R.mesh(coarse["disparity"].cpu().numpy(), 3, 2.0)
    assert_same("scene", "faces at step 3", u32_of(coarse["faces"]), R.faces(vi3, cells3))


def test_stereo_mesh_cameras_follows_the_records_that_map_back(capi):
    from ssrlcv_amd import pipeline
    import rectify_cases as RC
    s, t = RC.scene_pair(), RC.truth()
    left_d, right_d = torch.from_numpy(s["left"]).cuda(), torch.from_numpy(s["right"]).cuda()
    cam_l, cam_r = s["cams"][0], s["cams"][1]
    args = dict(radius=RC.CHAIN.r, min_disparity=t["dmin"], num_disparities=t["D"], lr_tolerance=RC.CHAIN.lr, subpixel=bool(RC.CHAIN.subpixel))
    step = 2
    out = pipeline.stereo_mesh_cameras(left_d, right_d, cam_l, cam_r, step=step, **args)
    pts, matches, n, disp, rect = pipeline.stereo_cloud_cameras(left_d, right_d, cam_l, cam_r, step=step, **args)
    assert out["n"] == n > 1000 and raw(out["points"]) == raw(pts) and raw(out["matches"]) == raw(matches) and raw(out["disparity"]) == raw(disp)
    assert out["rect"].tobytes() == rect.tobytes()
    # by hand: the records before the compaction say which vertices stay
    m2, n2 = capi.stereo_matches(disp, step, 0, 1)
    capi.matches_apply_homography(m2, n2, rect["Hl"], rect["Hr"])
    kept = np.nonzero(capi.to_host(m2, H.MATCH, n2)["invalid"] == 0)[0]
    assert len(kept) == n
    vi, cells, nv = R.mesh(disp.cpu().numpy(), step, float(step))
    assert nv == n2
    want_vi, want_cells = R.select(vi, cells, nv, kept)
    assert_same("scene", "vertex_index", u32_of(out["mesh"]["vertex_index"]), want_vi)
    assert_same("scene", "cells", out["mesh"]["cells"].cpu().numpy(), want_cells)
    faces = u32_of(out["faces"])
    assert len(faces) > 1000 and (faces < n).all()
    assert_same("scene", "faces", faces, R.faces(want_vi, want_cells))
    assert_same("scene", "normals", u32_of(out["normals"]), R.normals(pts.cpu().numpy(), want_vi, want_cells).view(np.uint32))


def test_a_mesh_follows_its_cloud_through_the_neighbour_filter(capi):
    from ssrlcv_amd import pipeline
    left, right = S.pair()
    out = pipeline.stereo_mesh(dev(left), dev(right), step=1, **S.CAMERA, **scene_args())
    kept = pipeline.filter_cloud(out["points"], k=8, sigma=1.0)
    m = kept["count"]
    assert 0 < m < out["n"]
    sub = pipeline.mesh_select(out["mesh"], kept["index"])
    faces = u32_of(pipeline.mesh_faces(sub))
    index = kept["index"].cpu().numpy()
    old = u32_of(out["faces"])
    assert_same("scene", "faces", faces, select_faces(old, out["n"], index))
    assert 0 < len(faces) < len(old) and (faces < m).all()
    # in step: a kept face names the same three positions in the kept cloud as it did in the whole one
    stays = np.isin(old, index).all(1)
    assert np.array_equal(kept["points"].cpu().numpy()[faces.astype(np.int64)], out["points"].cpu().numpy()[old[stays].astype(np.int64)])
    assert tuple(pipeline.mesh_normals(sub, kept["points"]).shape) == (m, 3)


def read_ply(path):
    """an ASCII PLY -> (vertex rows float32 (n, columns), faces uint32 (T, 3))"""
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    nv = nf = 0
    for line in lines[:end]:
        if line.startswith("element vertex"):
            nv = int(line.split()[2])
        if line.startswith("element face"):
            nf = int(line.split()[2])
    rows = np.array([[np.float32(v) for v in line.split()] for line in lines[end + 1:end + 1 + nv]], np.float32)
    faces = np.array([[int(v) for v in line.split()] for line in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64)
    assert nf == 0 or (faces[:, 0] == 3).all()
    return rows, faces[:, 1:].astype(np.uint32).reshape(-1, 3)


def test_class_api_program_writes_the_python_paths_mesh(capi, tmp_path):
    """DisparityFactory::generateMesh + MeshFactory::setSurface / computeSurfaceNormals / filterByNeighborDistance / saveMesh
    (tests/cpp/mesh_grid_test.cpp): the PLY's points, normals and faces are the Python path's, before and after the filter"""
    from ssrlcv_amd import pipeline
    name = "ramp"
    k = C.CASES[name]
    h, w = k.d.shape
    src = str(tmp_path / "map.f32")
    k.d.tofile(src)
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/mesh_grid_test"])
    cam = S.CAMERA
    a = [os.path.join(host, "_build", "mesh_grid_test"), src, str(w), str(h), str(k.step), repr(float(k.max_jump)), repr(cam["foc"]), repr(cam["baseline"]),
         repr(cam["doffset"]), repr(cam["cx"]), repr(cam["cy"]), "8", "1.0", str(tmp_path) + "/"]
    out = subprocess.check_output(a, timeout=120).decode().splitlines()
    assert out[-1] == "ok", out
    d = dev(k.d)
    matches, n = capi.stereo_matches(d, k.step, 0, 1)
    pts = capi.stereo_points(matches, n, **cam)
    mesh = pipeline.disparity_mesh(d, k.step, k.max_jump)
    rows, faces = read_ply(str(tmp_path / "mesh.ply"))
    assert_same(name, "points", rows[:, :3].view(np.uint32), u32_of(pts))
    assert_same(name, "normals", rows[:, 3:6].view(np.uint32), u32_of(pipeline.mesh_normals(mesh, pts)))
    assert_same(name, "faces", faces, u32_of(pipeline.mesh_faces(mesh)))
    kept = pipeline.filter_cloud(pts, k=8, sigma=1.0, normals=pipeline.mesh_normals(mesh, pts))
    sub = pipeline.mesh_select(mesh, kept["index"])
    rows, faces = read_ply(str(tmp_path / "filtered.ply"))
    assert 0 < kept["count"] < n
    assert_same(name, "filtered points", rows[:, :3].view(np.uint32), u32_of(kept["points"]))
    assert_same(name, "filtered normals", rows[:, 3:6].view(np.uint32), u32_of(kept["normals"]))
    assert_same(name, "filtered faces", faces, u32_of(pipeline.mesh_faces(sub)))
