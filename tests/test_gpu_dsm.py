"""The surface model on the GPU (ssrlcv_hip_dsm_rasterize, _dsm_fuse, _dsm_points; include/ssrlcv_hip.h "surface model") against
the numpy restatement of the contract (tests/dsm_ref.py) on the cases of tests/dsm_cases.py (tests/test_dsm_cases.py proves
without a GPU that they test something).  Every comparison is exact: heights as bit patterns, source, count, views and points as
integers or bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import dsm_cases as C
import dsm_ref as D
import mesh_ref as M

pytestmark = pytest.mark.gpu

u32, f32c, vp, csz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
GUARD = 64          # words on either side of every output
PATTERN = 0x5A5A5A5A


def cframe(capi, fr):
    return capi.DsmFrame.make(fr.origin, fr.ex, fr.ey, fr.ez, fr.cell, fr.w, fr.h)


def cloud_d(points):
    return torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()


class Guarded:
    """`words` 4-byte words in the middle of a buffer of a pattern"""

    def __init__(self, words, dtype=torch.int32, pattern=PATTERN):
        self.words, self.pattern = words, pattern if dtype == torch.int32 else pattern & 0xFF
        self.buf = torch.full((words + 2 * GUARD,), self.pattern, dtype=dtype, device="cuda")
        self.ptr = vp(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def result(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.pattern).all() and (host[GUARD + self.words:] == self.pattern).all(), "a guard word was written"
        return host[GUARD:GUARD + self.words]


def rasterize(capi, points, fr, rule, want_source=True, want_count=True):
    """the call with guard words around every map and behind a workspace pre-filled with 0xFF -> (height bits, source, count)"""
    cells = fr.w * fr.h
    p = cloud_d(points)
    need = int(capi.LIB.ssrlcv_hip_dsm_rasterize_workspace_bytes(u32(fr.w), u32(fr.h)))
    assert need == (8 * cells + 255) // 256 * 256
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    height, source, count = Guarded(cells), Guarded(cells) if want_source else None, Guarded(cells) if want_count else None
    capi.check(capi.LIB.ssrlcv_hip_dsm_rasterize(vp(p.data_ptr()) if len(points) else vp(0), u32(len(points)), ctypes.byref(cframe(capi, fr)), u32(rule),
                                                 height.ptr, source.ptr if source else vp(0), count.ptr if count else vp(0), vp(ws.data_ptr()),
                                                 csz(need), capi.stream_ptr()))
    assert (ws[need:] == 0xFF).all(), "the workspace was written behind its size"
    return (height.result().view(np.uint32).reshape(fr.h, fr.w), source.result().view(np.uint32).reshape(fr.h, fr.w) if source else None,
            count.result().view(np.uint32).reshape(fr.h, fr.w) if count else None)


def assert_maps(got, want, what):
    height, source, count = got
    ne = height != D.bits(want[0])
    assert not ne.any(), "%s: height differs at %d cells, first (j, i) %s" % (what, int(ne.sum()), tuple(np.argwhere(ne)[0]))
    if source is not None:
        ne = source != want[1]
        assert not ne.any(), "%s: source differs at %d cells, first (j, i) %s" % (what, int(ne.sum()), tuple(np.argwhere(ne)[0]))
    if count is not None:
        assert np.array_equal(count, want[2]), what


@pytest.mark.parametrize("name", sorted(C.RASTERIZE))
def test_rasterize_equals_the_reference(capi, name):
    c = C.RASTERIZE[name]
    for rule in (D.MAX, D.MIN):
        assert_maps(rasterize(capi, c.points, c.frame, rule), C.rasterize_reference(name, rule), "%s rule %d" % (name, rule))


@pytest.mark.parametrize("want_source,want_count", [(False, False), (True, False), (False, True)])
def test_rasterize_without_source_or_count(capi, want_source, want_count):
    for name in ("n257", "equal_heights", "runs_cross_waves", "sparse"):
        c = C.RASTERIZE[name]
        assert_maps(rasterize(capi, c.points, c.frame, D.MAX, want_source, want_count), C.rasterize_reference(name, D.MAX), name)
    height, source, count = capi.dsm_rasterize(cloud_d(C.RASTERIZE["n257"].points), cframe(capi, C.RASTERIZE["n257"].frame), D.MIN, want_source, want_count)
    assert (source is None) == (not want_source) and (count is None) == (not want_count)
    assert np.array_equal(H.bits(height.cpu().numpy()), D.bits(C.rasterize_reference("n257", D.MIN)[0]))


def test_the_order_of_the_points_does_not_matter(capi):
    """the same cloud as given, sorted by cell, reversed and shuffled: height and count bit-equal, source equal after mapping
    the indices back (distinct heights, so the winner does not depend on the index)"""
    for rule in (D.MAX, D.MIN):
        fr = C.RASTERIZE["order_given"].frame
        height, source, count = rasterize(capi, C.RASTERIZE["order_given"].points, fr, rule)
        for kind in ("sorted", "reversed", "shuffled"):
            order = C.order_of(kind)
            h2, s2, c2 = rasterize(capi, C.RASTERIZE["order_" + kind].points, fr, rule)
            assert np.array_equal(h2, height) and np.array_equal(c2, count)
            back = np.where(s2 == D.NONE, D.NONE, order[np.minimum(s2, len(order) - 1)].astype(np.uint32))
            assert np.array_equal(back, source)


def test_two_runs_are_bit_equal_and_a_side_stream_needs_no_host_sync(capi):
    c = C.RASTERIZE["large"]
    fr, p = cframe(capi, c.frame), cloud_d(c.points)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # rasterise, fuse and points back to back on the side stream; nothing reads a result in between
        a = capi.dsm_rasterize(p, fr, D.MAX)
        b = capi.dsm_rasterize(p, fr, D.MIN, False, False)
        fused, views = capi.dsm_fuse([a[0], b[0]], 2, 10.0, D.FUSE_MEDIAN)
    side.synchronize()
    want_a, want_b = C.rasterize_reference("large", D.MAX), C.rasterize_reference("large", D.MIN)
    assert_maps(tuple(x.cpu().numpy().view(np.uint32) for x in a), want_a, "side stream")
    want_f = D.fuse([want_a[0], want_b[0]], 2, 10.0, D.FUSE_MEDIAN)
    assert np.array_equal(H.bits(fused.cpu().numpy()), D.bits(want_f[0])) and np.array_equal(views.cpu().numpy(), want_f[1])
    again = capi.dsm_rasterize(p, fr, D.MAX)
    for x, y in zip(a, again):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- fuse
def fuse(capi, c, want_views=True):
    h, w = c.maps[0].shape
    uploaded = {}
    for m in c.maps:   # one upload an array: a map that is passed twice is one pointer twice
        if id(m) not in uploaded:
            uploaded[id(m)] = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    arr = (vp * len(c.maps))(*[uploaded[id(m)].data_ptr() for m in c.maps])
    out, views = Guarded(w * h), Guarded(w * h, torch.uint8) if want_views else None
    capi.check(capi.LIB.ssrlcv_hip_dsm_fuse(arr, u32(len(c.maps)), u32(w), u32(h), u32(c.min_views), f32c(c.max_spread), u32(c.rule), out.ptr,
                                            views.ptr if views else vp(0), capi.stream_ptr()))
    for m in c.maps:
        assert uploaded[id(m)].cpu().numpy().tobytes() == np.ascontiguousarray(m).tobytes()   # the inputs are left alone
    return out.result().view(np.uint32).reshape(h, w), views.result().reshape(h, w) if views else None


@pytest.mark.parametrize("name", sorted(C.FUSE))
def test_fuse_equals_the_reference(capi, name):
    want = C.fuse_reference(name)
    out, views = fuse(capi, C.FUSE[name])
    ne = out != D.bits(want[0])
    assert not ne.any(), "%s: differs at %d cells, first (j, i) %s" % (name, int(ne.sum()), tuple(np.argwhere(ne)[0]))
    assert np.array_equal(views, want[1])


def test_fuse_without_views_and_through_the_binder(capi):
    name = "63x5/m3/rule1/spread1"
    c, want = C.FUSE[name], C.fuse_reference(name)
    assert np.array_equal(fuse(capi, c, want_views=False)[0], D.bits(want[0]))
    maps = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in c.maps]
    out, views = capi.dsm_fuse(maps, c.min_views, c.max_spread, c.rule)
    assert np.array_equal(H.bits(out.cpu().numpy()), D.bits(want[0])) and np.array_equal(views.cpu().numpy(), want[1])
    assert capi.dsm_fuse(maps, c.min_views, c.max_spread, c.rule, want_views=False)[1] is None


# ---- points
def points_call(capi, height, fr, capacity):
    """-> (the written points' bits (min(count, capacity), 3), count); the rows behind them and the guards are untouched"""
    h_d = torch.from_numpy(np.ascontiguousarray(height)).cuda()
    need = int(capi.LIB.ssrlcv_hip_dsm_points_workspace_bytes(u32(fr.w), u32(fr.h)))
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out, count = Guarded(3 * capacity), Guarded(1)
    capi.check(capi.LIB.ssrlcv_hip_dsm_points(vp(h_d.data_ptr()), ctypes.byref(cframe(capi, fr)), out.ptr if capacity else vp(0), u32(capacity), count.ptr,
                                              vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == 0xFF).all()
    n = int(count.result().view(np.uint32)[0])
    rows = out.result().view(np.uint32).reshape(capacity, 3)
    assert (rows[min(n, capacity):] == PATTERN).all()
    return rows[:min(n, capacity)], n


@pytest.mark.parametrize("name", sorted(C.POINTS))
def test_points_equal_the_reference_at_every_capacity(capi, name):
    height, fr = C.POINTS[name]
    want = D.bits(D.points(height, fr))
    for capacity in sorted({0, max(len(want) - 1, 0), len(want), len(want) + 3}):
        rows, n = points_call(capi, height, fr, capacity)
        assert n == len(want) and np.array_equal(rows, want[:capacity]), (name, capacity)
    pts, n = capi.dsm_points(torch.from_numpy(np.ascontiguousarray(height)).cuda(), cframe(capi, fr))
    assert n == len(want) and np.array_equal(H.bits(pts.cpu().numpy()).reshape(-1, 3), want)


def test_the_numbering_is_the_mesh_s_and_the_normals_face_up(capi):
    from ssrlcv_amd import pipeline
    for height, fr in (C.POINTS["257x131"], C.tilted_plane()):
        h_d = torch.from_numpy(np.ascontiguousarray(height)).cuda()
        vertex_index, cells, count = capi.disparity_mesh(h_d, 1, float("inf"))
        vi = vertex_index.cpu().numpy().view(np.uint32)
        valid = D.bits(height) != D.INVALID_BITS
        assert int(count.item()) == valid.sum() and np.array_equal(vi[valid], np.arange(valid.sum())) and (vi[~valid] == D.NONE).all()
    height, fr = C.tilted_plane()
    surf = pipeline.surface_mesh({"height": torch.from_numpy(np.ascontiguousarray(height)).cuda()}, cframe(capi, fr), float("inf"))
    want_vi, want_cells, n = M.mesh(height, 1, np.inf)
    assert np.array_equal(surf["faces"].cpu().numpy().view(np.uint32), M.faces(want_vi, want_cells))
    assert np.array_equal(H.bits(surf["points"].cpu().numpy()).reshape(-1, 3), D.bits(D.points(height, fr)))
    normals = surf["normals"].cpu().numpy()
    assert np.array_equal(H.bits(normals), H.bits(M.normals(D.points(height, fr), want_vi, want_cells)))
    nonzero = np.abs(normals).sum(1) > 0
    assert nonzero.sum() > 100 and (normals[nonzero] @ fr.ez > 0).all()   # the sign of the dot product of every non-zero normal


# ---- end to end: three pairs of the rig
_E2E = {}
SCENE_PAIRS = C.PAIRS   # the rig's three pairs; (0, 1) is taken as (1, 0), the order in which it rectifies


def scene_clouds(capi):
    if not _E2E:
        from ssrlcv_amd import pipeline
        s = C.scene()
        clouds, rects = [], []
        for (a, b) in SCENE_PAIRS:
            lo, num, _ = C.pair_range((a, b))
            pts, _, n, _, rect = pipeline.stereo_cloud_cameras(torch.from_numpy(s["images"][a]).cuda(), torch.from_numpy(s["images"][b]).cuda(),
                                                               s["cams"][a], s["cams"][b], step=1, radius=4, min_disparity=lo,
                                                               num_disparities=num, lr_tolerance=1, subpixel=True)
            assert n > 10000
            clouds.append(pts), rects.append(rect)
        _E2E.update(clouds=clouds, rects=rects, host=[p.cpu().numpy() for p in clouds])
    return _E2E


FUSE_ARGS = dict(min_views=2, max_spread=1.0, rule="median")   # km: the relief is +-2 km, a pixel of disparity 0.25 to 0.5 km of depth


def test_surface_model_of_three_pairs_equals_the_reference_and_lies_on_the_ground(capi):
    from ssrlcv_amd import pipeline
    import scene as scene_mod
    s, e = C.scene(), scene_clouds(capi)
    fr = C.scene_frame()
    model = pipeline.surface_model(e["clouds"], cframe(capi, fr), rule="max", fuse=FUSE_ARGS)
    ref_maps = [D.rasterize(p, fr, D.MAX) for p in e["host"]]
    for k, want in enumerate(ref_maps):
        got = tuple(model[key][k].cpu().numpy().view(np.uint32) for key in ("maps", "sources", "counts"))
        assert_maps(got, want, "pair %s" % (SCENE_PAIRS[k],))
    want_fused, want_views = D.fuse([m[0] for m in ref_maps], FUSE_ARGS["min_views"], FUSE_ARGS["max_spread"], D.FUSE_MEDIAN)
    assert np.array_equal(H.bits(model["height"].cpu().numpy()), D.bits(want_fused)) and np.array_equal(model["views"].cpu().numpy(), want_views)
    assert (D.bits(want_fused) != D.INVALID_BITS).sum() > 1000
    rig, sc = s["rig"], s["scene"]
    centre, e1, e2, down = (np.asarray(v, np.float64) for v in (rig.centre, rig.e1, rig.e2, rig.down))

    def truth(a, b):
        return sc.height(torch.from_numpy(a).float(), torch.from_numpy(b).float()).double().numpy()

    lines = []
    jj, ii = np.mgrid[0:fr.h, 0:fr.w]
    half = C.SCENE_SIZE * rig.gsd / 2.0
    centre_truth = truth((ii.ravel() + 0.5) * float(fr.cell) - half, (jj.ravel() + 0.5) * float(fr.cell) - half).reshape(fr.h, fr.w)
    fused_ok = D.bits(want_fused) != D.INVALID_BITS
    for k, (height, source, count) in enumerate(ref_maps):
        occupied = count > 0
        p = e["host"][k][source[occupied]]
        loc = D.locate(p, fr)
        assert np.array_equal(D.bits(loc["z"]), D.bits(height)[occupied])                       # height = the z of points[source], bit for bit
        assert np.array_equal(loc["cell"], np.nonzero(occupied.ravel())[0])                      # and that point lies in the cell
        # the frame's conventions against the ground truth, in float64: the point's height above the patch at its own (a, b)
        q = p.astype(np.float64) - centre
        a, b, z = q @ e1, q @ e2, -(q @ down)
        h_true = truth(a, b)
        cam = s["cams"][SCENE_PAIRS[k][0]]
        ground = centre + a[:, None] * e1 + b[:, None] * e2 - h_true[:, None] * down
        Z = ((ground - cam["cam_pos"].astype(np.float64)) @ scene_mod._euler_matrix(e["rects"][k]["cam_rot"]))[:, 2]
        per_pixel = Z.mean() ** 2 / (float(e["rects"][k]["foc"]) * float(e["rects"][k]["baseline"]))   # km of depth per pixel of disparity
        err = np.abs(z - h_true)
        both = occupied & fused_ok
        pair_err = np.abs(height[both].astype(np.float64) - centre_truth[both])
        lines.append("pair %s: %d cells, winner's height error median %.4f max %.4f km (bound %.4f = 1.5 px of disparity); at the cell centres "
                     "over the fused cells: median %.4f max %.4f km" % (SCENE_PAIRS[k], int(occupied.sum()), np.median(err), err.max(), 1.5 * per_pixel,
                                                                        np.median(pair_err), pair_err.max()))
        print(lines[-1])
        assert err.max() <= 1.5 * per_pixel
    fused_err = np.abs(want_fused[fused_ok].astype(np.float64) - centre_truth[fused_ok])
    lines.append("fused (min_views 2, max_spread 1 km, median): %d cells, error at the cell centres median %.4f max %.4f km" % (
        int(fused_ok.sum()), np.median(fused_err), fused_err.max()))
    print(lines[-1])
    out = os.environ.get("SSRLCV_DSM_RECORD")   # a path to keep the lines in: the record at the end of profiles/dsm_bench.txt, not a bar
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


POST = dict(median=1, speckle_size=8, speckle_diff=0.5, fill=dict(paths=0xFF, max_gap=4, min_hits=5, rule="median"))


def test_surface_mesh_of_the_filled_map_equals_the_mesh_reference_and_the_class_api_agrees(capi, tmp_path):
    from ssrlcv_amd import pipeline
    e, fr = scene_clouds(capi), C.scene_frame()
    frame = cframe(capi, fr)
    plain = pipeline.surface_model(e["clouds"], frame, rule="max", fuse=FUSE_ARGS)
    model = pipeline.surface_model(e["clouds"], frame, rule="max", fuse=FUSE_ARGS, post=POST)
    # post is stereo_cloud's dictionary, unchanged, on the fused map
    want = pipeline.stereo_fill(pipeline.stereo_filter(plain["fused"].clone(), None, POST["median"], POST["speckle_size"], POST["speckle_diff"]), **POST["fill"])
    assert model["height"].cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and model["fused"].cpu().numpy().tobytes() == plain["height"].cpu().numpy().tobytes()
    height = model["height"].cpu().numpy()
    assert (D.bits(height) != D.INVALID_BITS).sum() > (D.bits(plain["height"].cpu().numpy()) != D.INVALID_BITS).sum()   # the fill filled
    max_jump = 1.0
    surf = pipeline.surface_mesh(model, frame, max_jump)
    vi, cells, n = M.mesh(height, 1, max_jump)
    faces = M.faces(vi, cells)
    assert len(faces) > 1000 and np.array_equal(surf["faces"].cpu().numpy().view(np.uint32), faces)
    assert np.array_equal(H.bits(surf["points"].cpu().numpy()).reshape(-1, 3), D.bits(D.points(height, fr)))
    normals = surf["normals"].cpu().numpy()
    nonzero = np.abs(normals).sum(1) > 0
    assert nonzero.sum() > 1000 and (normals[nonzero] @ fr.ez > 0).all()
    # the class API: MeshFactory::generateHeightMap, fuseHeightMaps, setPointsFromHeightMap, setSurface (tests/cpp/dsm_test.cpp)
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/dsm_test"])
    paths = []
    for k, p in enumerate(e["host"]):
        paths.append(str(tmp_path / ("cloud%d.raw" % k)))
        p.tofile(paths[-1])
    frame_path, prefix = str(tmp_path / "frame.raw"), str(tmp_path / "out")
    with open(frame_path, "wb") as f:
        f.write(bytes(frame))
    out = subprocess.check_output([os.path.join(host, "_build", "dsm_test"), frame_path, str(FUSE_ARGS["min_views"]), repr(FUSE_ARGS["max_spread"]),
                                   repr(max_jump), prefix] + paths, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    fused_plain = plain["height"].cpu().numpy()
    plain_surf = pipeline.surface_mesh(plain, frame, max_jump)
    for k in range(len(paths)):
        assert np.fromfile("%s.map%d" % (prefix, k), np.uint8).tobytes() == plain["maps"][k].cpu().numpy().tobytes()
    assert np.fromfile(prefix + ".fused", np.uint8).tobytes() == fused_plain.tobytes()
    assert np.fromfile(prefix + ".views", np.uint8).tobytes() == plain["views"].cpu().numpy().tobytes()
    assert np.fromfile(prefix + ".points", np.uint8).tobytes() == plain_surf["points"].cpu().numpy().tobytes()
    assert np.fromfile(prefix + ".faces", np.uint8).tobytes() == plain_surf["faces"].cpu().numpy().tobytes()
    assert np.fromfile(prefix + ".normals", np.uint8).tobytes() == plain_surf["normals"].cpu().numpy().tobytes()
    assert ("vertices %d faces %d" % (len(plain_surf["points"]), len(plain_surf["faces"]))) in out
