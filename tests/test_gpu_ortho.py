"""The ortho-image on the GPU (ssrlcv_hip_dsm_ortho; include/ssrlcv_hip.h "ortho-image") against the numpy restatement of the
contract (tests/ortho_ref.py) on the cases of tests/ortho_cases.py (tests/test_ortho_cases.py proves without a GPU that they test
something).  Every comparison is exact, byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import dsm_cases as DC
import dsm_ref as D
import ortho_cases as C
import ortho_ref as R
from test_gpu_dsm import FUSE_ARGS, POST, Guarded, cframe, scene_clouds

pytestmark = pytest.mark.gpu

u32, vp, csz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
OUTPUTS = ("ortho", "seen", "which")


def cviews(capi, views, images_d):
    arr = (capi.OrthoView * len(views))()
    for k, (v, img) in enumerate(zip(views, images_d)):
        h, w = v.image.shape
        arr[k] = capi.OrthoView(img.data_ptr(), w, h, (ctypes.c_float * 9)(*v.M.tolist()), (ctypes.c_float * 3)(*v.pos.tolist()),
                                (ctypes.c_float * 3)(*v.eye.tolist()))
    return arr


def ortho_call(capi, c, want_seen=True, want_which=True, fill=0xFF):
    """the raw call with guard words around every output, a workspace pre-filled with `fill` and checked behind its size, and the
    inputs compared with what was uploaded -> dict of uint8 (h, w), None for an output not asked for"""
    fr = c.frame
    cells = fr.w * fr.h
    height_d = torch.from_numpy(np.ascontiguousarray(c.height)).cuda()
    uploaded = {}
    for v in c.views:   # one upload an image: a view that is passed twice reads one buffer twice
        if id(v.image) not in uploaded:
            uploaded[id(v.image)] = torch.from_numpy(v.image).cuda()
    images_d = [uploaded[id(v.image)] for v in c.views]
    need = int(capi.LIB.ssrlcv_hip_dsm_ortho_workspace_bytes(u32(fr.w), u32(fr.h), u32(len(c.views))))
    assert need == 256
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    out = {"ortho": Guarded(cells, torch.uint8), "seen": Guarded(cells, torch.uint8) if want_seen else None,
           "which": Guarded(cells, torch.uint8) if want_which else None}
    params = capi.OrthoParams(c.max_steps, c.bias, c.rule)
    capi.check(capi.LIB.ssrlcv_hip_dsm_ortho(vp(height_d.data_ptr()), ctypes.byref(cframe(capi, fr)), cviews(capi, c.views, images_d), u32(len(c.views)),
                                             ctypes.byref(params), *[out[k].ptr if out[k] else vp(0) for k in OUTPUTS], vp(ws.data_ptr()), csz(need),
                                             capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    assert height_d.cpu().numpy().tobytes() == np.ascontiguousarray(c.height).tobytes()   # the inputs are left alone
    for v in c.views:
        assert uploaded[id(v.image)].cpu().numpy().tobytes() == v.image.tobytes()
    return {k: out[k].result().reshape(fr.h, fr.w) if out[k] else None for k in OUTPUTS}


def assert_equal(got, want, what):
    for k in OUTPUTS:
        if got[k] is None:
            continue
        ne = got[k] != want[k]
        assert not ne.any(), "%s: %s differs at %d cells, first (j, i) %s: %d for %d" % (
            what, k, int(ne.sum()), tuple(np.argwhere(ne)[0]), got[k][ne][0], want[k][ne][0])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_ortho_equals_the_reference(capi, name):
    assert_equal(ortho_call(capi, C.CASES[name]), C.reference(name), name)


@pytest.mark.parametrize("want_seen,want_which", [(False, False), (True, False), (False, True)])
def test_ortho_without_seen_or_which(capi, want_seen, want_which):
    for name in ("67x41/m3/rule1", "67x41/m8/rule0"):
        got = ortho_call(capi, C.CASES[name], want_seen, want_which)
        assert (got["seen"] is None) == (not want_seen) and (got["which"] is None) == (not want_which)
        assert_equal(got, C.reference(name), name)


def bound(capi, c):
    """a case through the binder's types -> (height tensor, frame, views, image tensors)"""
    images_d = [torch.from_numpy(v.image).cuda() for v in c.views]
    return torch.from_numpy(np.ascontiguousarray(c.height)).cuda(), cframe(capi, c.frame), list(cviews(capi, c.views, images_d)), images_d


def host(t):
    return None if t is None else t.cpu().numpy()


def test_two_runs_are_bit_equal_and_a_side_stream_needs_no_host_sync(capi):
    name = "257x131/m3/rule1"
    c, want = C.CASES[name], C.reference(name)
    height, frame, views, images = bound(capi, c)
    hole = torch.from_numpy(np.full(c.height.shape, D.INVALID_BITS, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # fuse and ortho back to back on the side stream; nothing reads a result in between
        fused, _ = capi.dsm_fuse([hole, height, hole], 1, float("inf"), D.FUSE_MEDIAN)   # the map itself: one valid entry a cell
        a = capi.dsm_ortho(fused, frame, views, images, c.max_steps, c.bias, c.rule)
    side.synchronize()
    assert fused.cpu().numpy().tobytes() == np.ascontiguousarray(c.height).tobytes()
    assert_equal(dict(zip(OUTPUTS, map(host, a))), want, "side stream")
    b = capi.dsm_ortho(height, frame, views, images, c.max_steps, c.bias, c.rule)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_the_binders_agree_with_the_raw_call(capi):
    from ssrlcv_amd import pipeline
    name = "67x41/m3/rule1"
    c, want = C.CASES[name], C.reference(name)
    height, frame, views, images = bound(capi, c)
    assert_equal(dict(zip(OUTPUTS, map(host, capi.dsm_ortho(height, frame, views, images, c.max_steps, c.bias, c.rule)))), want, "capi")
    ortho, seen, which = capi.dsm_ortho(height, frame, views, images, c.max_steps, c.bias, c.rule, want_seen=False, want_which=False)
    assert seen is None and which is None and np.array_equal(host(ortho), want["ortho"])
    # the pipeline makes its views from camera records through ssrlcv_dsm_ortho_view_host: the raw call on the same views
    cams = C.cameras(c.frame)
    records = [cams[n][0] for n in ("oblique45", "nadir", "diagonal")]
    built = [capi.dsm_ortho_view(cam, frame) for cam in records]
    for rule, code in (("first", R.FIRST), ("median", R.MEDIAN)):
        got = pipeline.surface_ortho({"height": height}, frame, images, records, max_steps=64, bias=None, rule=rule)
        raw = capi.dsm_ortho(height, frame, built, images, 64, 0.5 * C.CELL, code)
        ref = R.ortho(c.height, c.frame, [R.view(v.image, list(b.M), list(b.pos), list(b.eye)) for v, b in zip(c.views, built)], 64, 0.5 * C.CELL, code)
        for k, t in zip(OUTPUTS, raw):
            assert host(got[k]).tobytes() == host(t).tobytes() and np.array_equal(host(t), ref[k]), (rule, k)
    assert host(pipeline.surface_ortho(height, frame, images, records, max_steps=64)["ortho"]).tobytes() == host(
        pipeline.surface_ortho({"height": height}, frame, images, records, max_steps=64)["ortho"]).tobytes()   # the map alone
    with pytest.raises(ValueError):
        pipeline.surface_ortho(height, frame, images, records, rule="mean")
    # one grey a vertex, in dsm_points' order
    colors = pipeline.surface_colors(got["ortho"], height)
    valid = D.bits(c.height) != D.INVALID_BITS
    _, n = capi.dsm_points(height, frame)
    assert colors.dtype == torch.uint8 and len(colors) == n == valid.sum() and np.array_equal(host(colors), host(got["ortho"])[valid])


# ---- end to end on the rig's scene
def scene_views(capi, fr):
    """the three views of the scene as the host builder makes them -> (reference views, OrthoView list, image tensors)"""
    s = DC.scene()
    frame = cframe(capi, fr)
    built = [capi.dsm_ortho_view(cam, frame) for cam in s["cams"]]
    return [R.view(img, list(b.M), list(b.pos), list(b.eye)) for img, b in zip(s["images"], built)], built, [torch.from_numpy(i).cuda() for i in s["images"]]


def mad(a, b, where):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64))[where].mean())


def test_the_ortho_image_of_the_true_heights_is_the_texture(capi):
    """the scene's own heights at the cell centres, so the reference runs on the CPU: the ortho-image of every view lies nearer the
    true texture than any of its one-cell shifts and than the ortho-image over a flat map, and two views agree better over the
    true heights than over the flat map.  Relative statements; nothing is gated on an absolute DN value."""
    s, fr = DC.scene(), DC.scene_frame()
    rig, sc = s["rig"], s["scene"]
    half = DC.SCENE_SIZE * rig.gsd / 2.0
    jj, ii = np.mgrid[0:fr.h, 0:fr.w]
    a, b = (ii + 0.5) * float(fr.cell) - half, (jj + 0.5) * float(fr.cell) - half
    height = sc.height(torch.from_numpy(a).float(), torch.from_numpy(b).float()).numpy().astype(np.float32)
    texture = sc.texture(torch.from_numpy(a).float(), torch.from_numpy(b).float()).numpy().astype(np.float64)
    flat = np.zeros_like(height)
    views, built, images = scene_views(capi, fr)
    frame = cframe(capi, fr)
    STEPS, BIAS = 64, 0.0
    lines, per_view, per_view_flat = [], [], []

    def run(h, which_views):
        got = capi.dsm_ortho(torch.from_numpy(h).cuda(), frame, [built[k] for k in which_views], [images[k] for k in which_views], STEPS, BIAS, R.FIRST)
        want = R.ortho(h, fr, [views[k] for k in which_views], STEPS, BIAS, R.FIRST)
        assert_equal(dict(zip(OUTPUTS, map(host, got))), want, "scene views %s" % (which_views,))
        return want

    for k in range(3):
        true, level = run(height, [k]), run(flat, [k])
        per_view.append(true), per_view_flat.append(level)
        inner = np.zeros(true["seen"].shape, bool)
        inner[1:-1, 1:-1] = True
        seen = (true["seen"] == 1) & inner
        assert seen.sum() > 1000
        own = mad(true["ortho"], texture, seen)
        shifts = [mad(np.roll(true["ortho"], (dj, di), (0, 1)), texture, seen) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dj, di) != (0, 0)]
        over_flat = mad(level["ortho"], texture, seen & (level["seen"] == 1))
        lines.append("view %d: %d seen cells; MAD to the texture %.3f DN over the true heights, %.3f .. %.3f over the eight one-cell shifts, "
                     "%.3f over a flat map" % (k, int(seen.sum()), own, min(shifts), max(shifts), over_flat))
        print(lines[-1])
        assert own < min(shifts)
        if k != 0:   # the two oblique views
            assert own < over_flat
    run(height, [0, 1, 2])
    for p, q in ((0, 1), (0, 2), (1, 2)):
        both = (per_view[p]["seen"] == 1) & (per_view[q]["seen"] == 1) & (per_view_flat[p]["seen"] == 1) & (per_view_flat[q]["seen"] == 1)
        true, level = mad(per_view[p]["ortho"], per_view[q]["ortho"], both), mad(per_view_flat[p]["ortho"], per_view_flat[q]["ortho"], both)
        lines.append("views %d and %d: MAD between their ortho-images %.3f DN over the true heights, %.3f over a flat map" % (p, q, true, level))
        print(lines[-1])
        assert true < level
    out = os.environ.get("SSRLCV_ORTHO_RECORD")   # a path to keep the lines in: the record at the end of profiles/ortho_bench.txt, not a bar
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def test_the_surface_model_of_three_pairs_gets_its_picture_and_the_class_api_agrees(capi, tmp_path):
    from ssrlcv_amd import pipeline
    s, e, fr = DC.scene(), scene_clouds(capi), DC.scene_frame()
    frame = cframe(capi, fr)
    model = pipeline.surface_model(e["clouds"], frame, rule="max", fuse=FUSE_ARGS, post=POST)
    views, built, images = scene_views(capi, fr)
    height = host(model["height"])
    got = pipeline.surface_ortho(model, frame, images, s["cams"], max_steps=64, rule="median")
    want = R.ortho(height, fr, views, 64, 0.5 * float(fr.cell), R.MEDIAN)
    assert_equal({k: host(got[k]) for k in OUTPUTS}, want, "surface model")
    filled = (D.bits(height) != D.INVALID_BITS) & (D.bits(host(model["fused"])) == D.INVALID_BITS)
    # cells no cloud reached, made by the fill: they received a grey (how many there are is the fill's business: a dozen here)
    assert filled.sum() >= 1 and (host(got["seen"])[filled] != 0).sum() >= 1
    assert (host(got["which"])[filled & (host(got["seen"]) != 0)] != 0xFF).all()
    # the class API: MeshFactory::generateOrthoImage, setVertexColors, saveMesh (tests/cpp/ortho_test.cpp)
    hostdir = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", hostdir, "_build/ortho_test"])
    paths = {k: str(tmp_path / k) for k in ("height", "frame", "cams", "out")}
    height.tofile(paths["height"])
    with open(paths["frame"], "wb") as f:
        f.write(bytes(frame))
    np.ascontiguousarray(s["cams"]).tofile(paths["cams"])
    image_paths = []
    for k, img in enumerate(s["images"]):
        image_paths.append(str(tmp_path / ("image%d.raw" % k)))
        img.tofile(image_paths[-1])
    out = subprocess.check_output([os.path.join(hostdir, "_build", "ortho_test"), paths["frame"], paths["height"], paths["cams"], "64",
                                   repr(0.5 * float(fr.cell)), "1", paths["out"]] + image_paths, timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    assert np.fromfile(paths["out"] + ".ortho", np.uint8).tobytes() == want["ortho"].tobytes()
    colors = host(pipeline.surface_colors(got["ortho"], model["height"]))
    ply = open(paths["out"] + ".ply", "rb").read()
    head, body = ply[:ply.index(b"end_header\n") + 11].decode(), ply[ply.index(b"end_header\n") + 11:].decode().splitlines()
    assert ("element vertex %d" % len(colors)) in head and "property uchar red" in head and "property uchar blue" in head
    rows = np.array([line.split() for line in body[:len(colors)]])
    assert rows.shape[1] >= 6
    rgb = rows[:, -3:].astype(np.int64)
    assert (rgb[:, 0] == colors).all() and (rgb[:, 1] == colors).all() and (rgb[:, 2] == colors).all()
