"""Mesh render on the GPU (ssrlcv_hip_mesh_render, ssrlcv_hip_image_residual; include/ssrlcv_hip.h "mesh render") against the numpy
restatement of the contract (tests/render_ref.py) on the cases of tests/render_cases.py (tests/test_render_cases.py proves without
a GPU that they test something).  Every comparison is exact, byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import dsm_cases as DC
import dsm_ref as D
import render_cases as C
import render_ref as R
from test_gpu_dsm import Guarded, cframe, cloud_d

pytestmark = pytest.mark.gpu

u32, f32c, vp, csz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
OUTPUTS = ("depth", "triangle", "shade", "counts")


def cview(capi, v):
    """the render reads M, pos, w and h: the image is NULL and the eye a NaN"""
    return capi.OrthoView(0, v.w, v.h, (f32c * 9)(*v.M.tolist()), (f32c * 3)(*v.pos.tolist()), (f32c * 3)(float("nan"), float("nan"), float("nan")))


def dev(a):
    """a numpy array on the device; an empty one as a byte nobody reads, so that its pointer is not NULL"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(1, np.uint8)).cuda()


def render_call(capi, c, want=OUTPUTS, grey=True, fill=0xFF):
    """the raw call with guard words around every output, a workspace pre-filled with `fill` and checked behind its size, and the
    inputs compared with what was uploaded -> dict of arrays, None for an output not asked for"""
    n, pixels = len(c.points), c.view.w * c.view.h
    gh, gw = c.vertex_index.shape
    inputs = dict(points=c.points, grey=c.grey, vertex_index=c.vertex_index, cells=c.cells)
    d = {k: dev(a) for k, a in inputs.items()}
    need = int(capi.LIB.ssrlcv_hip_mesh_render_workspace_bytes(u32(n), u32(c.view.w), u32(c.view.h)))
    assert need == 256 + a256(8 * pixels) + a256(16 * n)
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    out = {"depth": Guarded(pixels), "triangle": Guarded(pixels) if "triangle" in want else None,
           "shade": Guarded(pixels, torch.uint8) if "shade" in want else None, "counts": Guarded(3) if "counts" in want else None}
    params = capi.RenderParams(c.max_extent)
    capi.check(capi.LIB.ssrlcv_hip_mesh_render(vp(d["points"].data_ptr()), u32(n), vp(d["grey"].data_ptr()) if grey else vp(0), vp(d["vertex_index"].data_ptr()),
                                               vp(d["cells"].data_ptr()), u32(gw), u32(gh), ctypes.byref(cview(capi, c.view)), ctypes.byref(params),
                                               *[out[k].ptr if out[k] else vp(0) for k in OUTPUTS], vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    for k, a in inputs.items():      # the inputs are left alone
        assert d[k].cpu().numpy().tobytes()[:a.nbytes] == np.ascontiguousarray(a).tobytes(), k
    shape = (c.view.h, c.view.w)
    return {"depth": out["depth"].result().view(np.uint32).reshape(shape),
            "triangle": out["triangle"].result().view(np.uint32).reshape(shape) if out["triangle"] else None,
            "shade": out["shade"].result().reshape(shape) if out["shade"] else None,
            "counts": out["counts"].result().view(np.uint32) if out["counts"] else None}


def assert_equal(got, want, what):
    for k in OUTPUTS:
        if got[k] is None:
            continue
        ne = got[k] != want[k]
        assert not ne.any(), "%s: %s differs at %d entries, first %s: %#x for %#x" % (
            what, k, int(ne.sum()), tuple(np.argwhere(ne)[0]), int(got[k][ne][0]), int(want[k][ne][0]))


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_render_equals_the_reference_twice(capi, name):
    c, want = C.CASES[name], C.reference(name)
    first = render_call(capi, c)
    assert_equal(first, want, name)
    again = render_call(capi, c, fill=0x00)          # run to run, and whatever the workspace held
    for k in OUTPUTS:
        assert again[k].tobytes() == first[k].tobytes(), (name, k)


@pytest.mark.parametrize("name", ["cell_bytes", "fold", "stale_index", "off_image"])
def test_every_optional_buffer_may_be_null(capi, name):
    c, want = C.CASES[name], C.reference(name)
    for leave_out in ("triangle", "shade", "counts"):
        got = render_call(capi, c, want=[k for k in OUTPUTS if k != leave_out])
        assert got[leave_out] is None
        assert_equal(got, want, "%s without %s" % (name, leave_out))
    assert_equal(render_call(capi, c, want=("depth",)), want, name + ", depth alone")
    # without greys the shade is 0 everywhere and nothing else changes
    plain = render_call(capi, c, grey=False)
    assert (plain["shade"] == 0).all() and (want["shade"] != 0).any()
    assert_equal(dict(plain, shade=None), want, name + " without greys")
    assert_equal(plain, R.render(c.points, None, c.vertex_index, c.cells, c.view, c.max_extent), name + " without greys, the reference's")


def test_an_empty_view_writes_the_counts_alone(capi):
    c = C.CASES["cell_bytes"]
    for w, h in ((0, 0), (0, 5), (5, 0)):
        counts = Guarded(3)
        view = cview(capi, c.view._replace(w=w, h=h))
        assert capi.LIB.ssrlcv_hip_mesh_render(vp(0), u32(len(c.points)), vp(0), vp(0), vp(0), u32(2), u32(14), ctypes.byref(view),
                                               ctypes.byref(capi.RenderParams(8)), vp(0), vp(0), vp(0), counts.ptr, vp(0), csz(0), capi.stream_ptr()) == 0
        assert counts.result().tolist() == [0, 0, 0]


def test_a_mesh_after_mesh_select(capi):
    """the mesh of the fold restricted on the GPU (ssrlcv_hip_mesh_select), drawn with the kept vertices: the reference's own
    selection, "fold/selected" """
    whole, c = C.CASES["fold"], C.CASES["fold/selected"]
    n = len(whole.points)
    kept = torch.from_numpy(np.array([k for k in range(n) if k % 3 != 1], np.int32)).cuda()
    vi = torch.from_numpy(whole.vertex_index.view(np.int32).copy()).cuda()
    cells = torch.from_numpy(whole.cells.copy()).cuda()
    capi.mesh_select(vi, cells, n, kept)
    assert np.array_equal(vi.cpu().numpy().view(np.uint32), c.vertex_index) and np.array_equal(cells.cpu().numpy(), c.cells)
    depth, triangle, shade, counts = capi.mesh_render(cloud_d(c.points), vi, cells, cview(capi, c.view), torch.from_numpy(c.grey).cuda(), c.max_extent)
    got = dict(depth=H.bits(depth.cpu().numpy()), triangle=triangle.cpu().numpy().view(np.uint32), shade=shade.cpu().numpy(),
               counts=counts.cpu().numpy().view(np.uint32))
    assert_equal(got, C.reference("fold/selected"), "fold/selected")


def residual_call(capi, image, shade, depth_bits):
    h, w = image.shape
    out = Guarded(w * h)
    i_d, s_d, d_d = (torch.from_numpy(np.array(a)).cuda() for a in (image, shade, depth_bits.view(np.float32)))   # copies: the reference's arrays are read-only
    capi.check(capi.LIB.ssrlcv_hip_image_residual(vp(i_d.data_ptr()), vp(s_d.data_ptr()), vp(d_d.data_ptr()), u32(w), u32(h), out.ptr, capi.stream_ptr()))
    for t, a in ((i_d, image), (s_d, shade), (d_d, depth_bits)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    return out.result().view(np.uint32).reshape(h, w)


@pytest.mark.parametrize("name", ["fold", "view_1x1", "view_65x3", "grid_1x1"])
def test_the_residual_of_a_map_with_holes(capi, name):
    r = C.reference(name)
    image = np.random.RandomState(9).randint(0, 256, r["shade"].shape).astype(np.uint8)
    depth = r["depth"].copy()
    if name == "fold":       # NaNs that are values, an infinity and a zero among the depths: only 0x7FC00000 is a hole
        depth[0, :5] = (0x7FC00001, 0xFFC00000, 0x7F800000, 0x00000000, 0x7FC00000)
    want = R.residual(image, r["shade"], depth)
    assert name != "fold" or ((want == R.INVALID_BITS).any() and (want[0, :4] != R.INVALID_BITS).all() and want[0, 4] == R.INVALID_BITS)
    got = residual_call(capi, image, r["shade"], depth)
    assert np.array_equal(got, want)
    # the statistics take the map as it is: the holes are left out, nothing else
    rec = capi.difference_stats(torch.from_numpy(got.view(np.float32).copy()).cuda().reshape(-1), quantiles=(5000,))
    assert (rec.n, rec.valid, rec.finite) == (want.size, int((want != R.INVALID_BITS).sum()), int((want != R.INVALID_BITS).sum()))
    if rec.finite:
        assert rec.quantile[0] == R.stats(want)["median"]


def test_the_binders_a_side_stream_and_the_pipeline(capi):
    from ssrlcv_amd import pipeline
    name = "fold"
    c, want = C.CASES[name], C.reference(name)
    p, g = cloud_d(c.points), torch.from_numpy(c.grey).cuda()
    vi, cells = torch.from_numpy(c.vertex_index.view(np.int32).copy()).cuda(), torch.from_numpy(c.cells.copy()).cuda()
    image = torch.from_numpy(np.random.RandomState(9).randint(0, 256, want["shade"].shape).astype(np.uint8)).cuda()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    as_dict = lambda r: dict(depth=H.bits(host(r[0])), triangle=None if r[1] is None else host(r[1]).view(np.uint32), shade=host(r[2]),  # noqa: E731
                             counts=host(r[3]).view(np.uint32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):       # render and residual back to back on a side stream; nothing reads a result in between
        r = capi.mesh_render(p, vi, cells, cview(capi, c.view), g, c.max_extent)
        res = capi.image_residual(image, r[2], r[0])
    side.synchronize()
    assert_equal(as_dict(r), want, "side stream")
    assert np.array_equal(H.bits(host(res)), R.residual(host(image), want["shade"], want["depth"]))
    ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")      # a workspace that is large enough is reused, whatever it holds
    r = capi.mesh_render(p, vi, cells, cview(capi, c.view), g, c.max_extent, want_triangle=False, want_shade=False, workspace=ws)
    assert r[1] is None and r[2] is None
    assert_equal(as_dict(r), want, "reused workspace")
    with pytest.raises(capi.SsrlcvError):
        capi.mesh_render(p, vi, cells, cview(capi, c.view), g, 65)
    with pytest.raises(capi.SsrlcvError):
        capi.mesh_render(p, vi, cells, cview(capi, c.view), g, 0)


# ---- end to end on the rig's scene
def test_the_scene_s_model_predicts_a_source_view_and_a_displaced_model_does_not(capi):
    """The scene's own heights, meshed, textured with the ortho-image of all three views and drawn into the camera of view 1: the
    GPU equals the reference bit for bit, through the raw binder and through pipeline.surface_photo_check, and on the reference the
    residual's NMAD of the model where it is lies below that of the model shifted by 2 cells along either axis and of the model
    raised by 2 cells.  A comparison between reference runs; no threshold.  Measured on the reference: NMAD 1.4826 grey levels where
    it is, 8.8956 and 10.3782 shifted along ex and ey, 2.9652 raised (integers times 1.4826: the residuals are whole grey levels)."""
    from ssrlcv_amd import pipeline
    s, m = DC.scene(), C.scene_model()
    fr, frame = m["frame"], cframe(capi, m["frame"])
    here = C.scene_check()
    moved = {"shifted 2 cells along ex": C.scene_check((2, 0)), "shifted 2 cells along ey": C.scene_check((0, 2)), "raised 2 cells": C.scene_check((0, 0), 2.0)}
    lines = ["the scene's model in view %d: coverage %.4f, median %.1f, NMAD %.4f, RMS %.3f grey levels" % (
        C.CHECK_VIEW, here["stats"]["coverage"], here["stats"]["median"], here["stats"]["nmad"], here["stats"]["rms"])]
    for what, r in moved.items():
        lines.append("%s: coverage %.4f, median %.1f, NMAD %.4f, RMS %.3f" % (what, r["stats"]["coverage"], r["stats"]["median"], r["stats"]["nmad"], r["stats"]["rms"]))
    print("\n".join(lines))
    # the GPU, on the same inputs, every variant
    cam = s["cams"][C.CHECK_VIEW]
    view = capi.dsm_ortho_view(cam, frame)
    v = C.scene_views()[C.CHECK_VIEW]
    assert list(view.M) == v.M.tolist() and list(view.pos) == v.pos.tolist()        # the host builder's view is the restated one
    vi, cells = torch.from_numpy(m["vertex_index"].view(np.int32).copy()).cuda(), torch.from_numpy(m["cells"].copy()).cuda()
    grey, image = torch.from_numpy(m["grey"].copy()).cuda(), torch.from_numpy(s["images"][C.CHECK_VIEW]).cuda()
    for what, r in [("where it is", here)] + list(moved.items()):
        depth, triangle, shade, counts = capi.mesh_render(cloud_d(r["points"]), vi, cells, view, grey, 8)
        got = dict(depth=H.bits(depth.cpu().numpy()), triangle=triangle.cpu().numpy().view(np.uint32), shade=shade.cpu().numpy(),
                   counts=counts.cpu().numpy().view(np.uint32))
        assert_equal(got, r["render"], what)
        assert np.array_equal(H.bits(capi.image_residual(image, shade, depth).cpu().numpy()), r["residual"]), what
    # the whole chain: heights -> points, mesh, ortho-image, colours, render, residual, statistics
    height = torch.from_numpy(m["height"]).cuda()
    images = [torch.from_numpy(i).cuda() for i in s["images"]]
    ortho = pipeline.surface_ortho(height, frame, [images[k] for k in C.TEXTURE_VIEWS], [s["cams"][k] for k in C.TEXTURE_VIEWS], max_steps=C.ORTHO_STEPS,
                                   bias=C.ORTHO_BIAS, rule="first")["ortho"]
    assert np.array_equal(ortho.cpu().numpy(), m["ortho"])
    check = pipeline.surface_photo_check({"height": height}, frame, ortho, image, cam, want_map=True)
    assert np.array_equal(H.bits(check["residual"].cpu().numpy()), here["residual"])
    assert {k: check[k] for k in ("coverage", "median", "nmad", "rms")} == here["stats"]
    assert check["counts"] == dict(zip(("drawn", "too_large", "unusable"), here["render"]["counts"].tolist()))
    drawn = pipeline.surface_render(height, frame, cam, pipeline.surface_colors(ortho, height))
    assert np.array_equal(H.bits(drawn["depth"].cpu().numpy()), here["render"]["depth"]) and np.array_equal(drawn["shade"].cpu().numpy(), here["render"]["shade"])
    assert (pipeline.surface_render(height, frame, cam)["shade"] == 0).all()
    # the comparison, on the reference alone
    for what, r in moved.items():
        assert here["stats"]["nmad"] < r["stats"]["nmad"], what
    out = os.environ.get("SSRLCV_RENDER_RECORD")   # a path to keep the lines in: the record at the end of profiles/render_bench.txt, not a bar
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def test_the_mirror_program_gives_the_pipeline_s_maps_and_figures(capi, tmp_path):
    """MeshFactory::renderView and MeshFactory::photoConsistency through tests/cpp/render_test.cpp"""
    s, m = DC.scene(), C.scene_model()
    here = C.scene_check()
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/render_test"])
    frame = cframe(capi, m["frame"])
    paths = {n: str(tmp_path / (n + ".raw")) for n in ("frame", "height", "ortho", "image", "camera")}
    with open(paths["frame"], "wb") as f:
        f.write(bytes(frame))
    m["height"].tofile(paths["height"]), m["ortho"].tofile(paths["ortho"]), s["images"][C.CHECK_VIEW].tofile(paths["image"])
    np.asarray(s["cams"][C.CHECK_VIEW]).tofile(paths["camera"])
    prefix = str(tmp_path / "out")
    out = subprocess.check_output([os.path.join(host, "_build", "render_test"), paths["frame"], paths["height"], paths["ortho"], paths["image"], paths["camera"],
                                   "inf", "8", prefix], timeout=120).decode()
    assert out.splitlines()[-1] == "ok", out
    assert np.array_equal(np.fromfile(prefix + ".depth", np.uint32), here["render"]["depth"].reshape(-1))
    assert np.array_equal(np.fromfile(prefix + ".triangle", np.uint32), here["render"]["triangle"].reshape(-1))
    assert np.array_equal(np.fromfile(prefix + ".shade", np.uint8), here["render"]["shade"].reshape(-1))
    assert np.array_equal(np.fromfile(prefix + ".residual", np.uint32), here["residual"].reshape(-1))
    figures = np.fromfile(prefix + ".figures", np.float64)      # coverage, median, nmad, rms, drawn, too large, unusable
    assert figures[:4].tolist() == [here["stats"][k] for k in ("coverage", "median", "nmad", "rms")]
    assert figures[4:].tolist() == here["render"]["counts"].tolist()
