"""The map kernels of the stereo and the surface chains past the caps of their launch grids, on the GPU: the cases of
tests/large_cases.py (tests/test_large_cases.py proves without a GPU that each reaches the later trips of its kernels' grid-stride
loops) against the numpy restatements the small cases are held to.  Every comparison is exact, over the whole map.  Every call
runs twice, on a workspace pre-filled with 0xFF and with 0x00, its outputs between guard words, nothing written behind the
queried workspace size, its inputs compared with what was uploaded."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import large_cases as L
from test_gpu_dsm import GUARD, Guarded
from test_gpu_ortho import assert_equal as assert_ortho_equal
from test_gpu_ortho import ortho_call
from test_gpu_render import assert_equal as assert_render_equal
from test_gpu_render import render_call

pytestmark = pytest.mark.gpu

u32, vp, csz, cint, f32c = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
FILLS = (0xFF, 0x00)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases and references are read-only


def workspace(need, fill):
    return torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")


def guarded_copy(a):
    """a Guarded buffer that holds the words of `a`: the map of an in-place call"""
    a = np.ascontiguousarray(a)
    g = Guarded(a.size)
    g.buf[GUARD:GUARD + a.size].copy_(torch.from_numpy(a.reshape(-1).view(np.int32).copy()))
    return g


def words(g, shape):
    return g.result().view(np.uint32).reshape(shape)


def assert_same(what, got, want):
    ne = got != want
    assert not ne.any(), "%s differs at %d of %d entries, first %s: got %s want %s" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][:4], want[ne][:4])


def unchanged(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


# ---- 1. block matching, semi-global matching and the matches of the map
def stereo_call(capi, entry, query, params, fill):
    """-> (disparity bits, cost) of one matching call on the large pair"""
    c = L.stereo_case()
    left, right = L.stereo_scene()
    left_d, right_d = dev(left), dev(right)
    need = int(query(u32(c.w), u32(c.h), ctypes.byref(params)))
    ws, disp, cost = workspace(need, fill), Guarded(c.w * c.h), Guarded(c.w * c.h)
    capi.check(entry(vp(left_d.data_ptr()), vp(right_d.data_ptr()), u32(c.w), u32(c.h), ctypes.byref(params), vp(ws.data_ptr()), csz(need), disp.ptr,
                     cost.ptr, capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    assert unchanged(left_d, left) and unchanged(right_d, right)
    return words(disp, (c.h, c.w)), words(cost, (c.h, c.w))


def test_block_matching_past_the_fill_and_the_left_right_grids(capi):
    c, ref = L.stereo_case(), L.stereo_reference()
    p = capi.StereoParams(c.r, c.dmin, c.D, c.max_cost, c.lr, c.subpixel)
    for fill in FILLS:
        disp, cost = stereo_call(capi, capi.LIB.ssrlcv_hip_stereo_sad_u8, capi.LIB.ssrlcv_hip_stereo_workspace_bytes, p, fill)
        assert_same("disparity (workspace %#x)" % fill, disp, H.bits(ref["disparity"]))
        assert_same("cost (workspace %#x)" % fill, cost, ref["cost"])


def test_semi_global_matching_past_the_fill_and_the_left_right_grids(capi):
    c, ref = L.stereo_case(), L.sgm_reference()
    p = capi.SgmParams(c.r, c.dmin, c.D, L.SGM["clamp"], L.SGM["P1"], L.SGM["P2"], L.SGM["paths"], c.lr, c.subpixel)
    for fill in FILLS:
        disp, cost = stereo_call(capi, capi.LIB.ssrlcv_hip_stereo_sgm_u8, capi.LIB.ssrlcv_hip_stereo_sgm_workspace_bytes, p, fill)
        assert_same("disparity (workspace %#x)" % fill, disp, H.bits(ref["disparity"]))
        assert_same("cost (workspace %#x)" % fill, cost, ref["cost"])


def test_the_matches_of_the_large_map_pass_the_second_scan_round(capi):
    c, want = L.stereo_case(), L.matches_reference()
    disparity = L.stereo_reference()["disparity"]      # the reference's map: this test is about the compaction
    disp_d = dev(disparity)
    cap = c.w * c.h
    need = int(capi.LIB.ssrlcv_hip_stereo_matches_workspace_bytes(u32(c.w), u32(c.h), u32(1)))
    for fill in FILLS:
        ws, out, count = workspace(need, fill), Guarded(cap * 10), Guarded(1)
        capi.check(capi.LIB.ssrlcv_hip_stereo_matches(vp(disp_d.data_ptr()), u32(c.w), u32(c.h), u32(1), cint(L.MATCH_IDS[0]), cint(L.MATCH_IDS[1]), out.ptr,
                                                      u32(cap), count.ptr, vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
        assert (ws[need:] == fill).all(), "the workspace was written behind its size"
        assert int(count.result()[0]) == len(want)
        records = out.result()
        assert records[:10 * len(want)].tobytes() == want.tobytes()      # the records' bytes, padding (zero) included
        assert (records[10 * len(want):] == out.pattern).all()           # nothing behind the count
    assert unchanged(disp_d, disparity)


# ---- 2. census codes
@pytest.mark.parametrize("c", L.CENSUS_RADII)
def test_census_codes_past_the_grid(capi, c):
    img, want = L.census_image(), L.census_reference(c)
    h, w = img.shape
    img_d = dev(img)
    for fill in (-1, 0):     # every byte of the output 0xFF, then 0x00
        codes = Guarded(2 * w * h)
        codes.buf[GUARD:GUARD + 2 * w * h].fill_(fill)
        capi.check(capi.LIB.ssrlcv_hip_census_u8(vp(img_d.data_ptr()), u32(w), u32(h), u32(c), codes.ptr, capi.stream_ptr()))
        got = codes.result().view(np.uint64).reshape(h, w)
        assert_same("census %d codes (output pre-filled with %d)" % (c, fill), got, want)
    assert unchanged(img_d, img)


# ---- 3. components, speckles, fill
def components_call(capi, d, max_diff, fill, want_sizes=True):
    h, w = d.shape
    d_d = dev(d)
    need = int(capi.LIB.ssrlcv_hip_disparity_components_workspace_bytes(u32(w), u32(h)))
    ws, labels, sizes = workspace(need, fill), Guarded(w * h), Guarded(w * h) if want_sizes else None
    capi.check(capi.LIB.ssrlcv_hip_disparity_components(vp(d_d.data_ptr()), u32(w), u32(h), f32c(max_diff), labels.ptr, sizes.ptr if sizes else vp(0),
                                                        vp(ws.data_ptr()), csz(need), capi.stream_ptr()))
    assert (ws[need:] == fill).all(), "the workspace was written behind its size"
    assert unchanged(d_d, d)
    return words(labels, (h, w)), words(sizes, (h, w)) if sizes else None


@pytest.mark.parametrize("name", L.COMPONENT_NAMES)
def test_labels_and_sizes_over_17_x_75_tiles(capi, name):
    k = L.component_case(name)
    want_labels, want_sizes = L.component_reference(name)
    for fill in FILLS:
        labels, sizes = components_call(capi, k.d, k.max_diff, fill)
        assert_same("%s labels (workspace %#x)" % (name, fill), labels, want_labels)
        assert_same("%s sizes (workspace %#x)" % (name, fill), sizes, want_sizes)
    only, none = components_call(capi, k.d, k.max_diff, 0xFF, want_sizes=False)       # sizes NULL: the same labels
    assert none is None
    assert_same("%s labels without sizes" % name, only, want_labels)


def test_the_speckle_filter_with_a_cost_map_past_the_grid(capi):
    k, cost = L.component_case("noise"), L.speckle_cost()
    want_d, want_c = L.speckle_reference()
    h, w = k.d.shape
    need = int(capi.LIB.ssrlcv_hip_stereo_filter_speckles_workspace_bytes(u32(w), u32(h)))
    for fill in FILLS:
        ws, d, c = workspace(need, fill), guarded_copy(k.d), guarded_copy(cost)
        capi.check(capi.LIB.ssrlcv_hip_stereo_filter_speckles(d.ptr, c.ptr, u32(w), u32(h), f32c(k.max_diff), u32(k.max_size), vp(ws.data_ptr()), csz(need),
                                                              capi.stream_ptr()))
        assert (ws[need:] == fill).all(), "the workspace was written behind its size"
        assert_same("disparity (workspace %#x)" % fill, words(d, (h, w)), H.bits(want_d))
        assert_same("cost (workspace %#x)" % fill, words(c, (h, w)), want_c)
    d = guarded_copy(k.d)                                                              # cost NULL: the same map
    ws = workspace(need, 0xFF)
    capi.check(capi.LIB.ssrlcv_hip_stereo_filter_speckles(d.ptr, vp(0), u32(w), u32(h), f32c(k.max_diff), u32(k.max_size), vp(ws.data_ptr()), csz(need),
                                                          capi.stream_ptr()))
    assert_same("disparity without a cost map", words(d, (h, w)), H.bits(want_d))


@pytest.mark.parametrize("call", [0, 1])
def test_hole_filling_over_ten_strips_past_the_grid(capi, call):
    import fill_ref as F
    d, args = L.fill_map(), L.fill_calls()[call]
    want, want_mask = L.fill_reference(call)
    h, w = d.shape
    d_d = dev(d)
    p = capi.FillParams(args["paths"], args["max_gap"], args["min_hits"], args["rule"])
    need = int(capi.LIB.ssrlcv_hip_stereo_fill_holes_workspace_bytes(u32(w), u32(h), ctypes.byref(p)))
    for fill in FILLS:
        ws, out, mask = workspace(need, fill), Guarded(w * h), Guarded(w * h, torch.uint8)
        capi.check(capi.LIB.ssrlcv_hip_stereo_fill_holes(vp(d_d.data_ptr()), out.ptr, mask.ptr, u32(w), u32(h), ctypes.byref(p), vp(ws.data_ptr()), csz(need),
                                                         capi.stream_ptr()))
        assert (ws[need:] == fill).all(), "the workspace was written behind its size"
        assert_same("out (workspace %#x)" % fill, words(out, (h, w)), F.bits_of(want))
        assert_same("filled (workspace %#x)" % fill, mask.result().reshape(h, w), want_mask)
    assert unchanged(d_d, d)


# ---- 4. the ortho-image under a tower that one load of k_ortho_top sees
@pytest.mark.parametrize("variant", L.ORTHO_VARIANTS)
def test_the_ortho_image_behind_a_tower_only_one_load_sees(capi, variant):
    c, want = L.ortho_case(variant), L.ortho_reference(variant)
    for fill in FILLS:
        assert_ortho_equal(ortho_call(capi, c, fill=fill), want, "%s (workspace %#x)" % (variant, fill))


# ---- 5. render scatter
def test_render_with_triangles_of_the_second_trip(capi):
    c, (want, _) = L.render_case(), L.render_reference()
    for fill in FILLS:
        got = render_call(capi, c, fill=fill)
        assert_render_equal(got, want, "workspace %#x" % fill)
        assert got["counts"].tolist() == [6, 1, 1]


# ---- 6. subtract
def test_subtract_past_the_grid_also_in_place(capi):
    a, b = L.subtract_pair()
    want = L.subtract_reference()
    h, w = a.shape
    a_d, b_d = dev(a), dev(b)
    for pattern in (0x5A5A5A5A, 0x3C3C3C3C):
        out = Guarded(w * h, pattern=pattern)
        capi.check(capi.LIB.ssrlcv_hip_dsm_subtract(vp(a_d.data_ptr()), vp(b_d.data_ptr()), u32(w), u32(h), out.ptr, capi.stream_ptr()))
        assert_same("subtract (output pre-filled with %#x)" % pattern, words(out, (h, w)), want)
    assert unchanged(a_d, a) and unchanged(b_d, b)
    for alias in (0, 1):                                                               # out == a, then out == b
        x, y = guarded_copy(a), guarded_copy(b)
        capi.check(capi.LIB.ssrlcv_hip_dsm_subtract(x.ptr, y.ptr, u32(w), u32(h), (x, y)[alias].ptr, capi.stream_ptr()))
        assert_same("subtract onto input %d" % alias, words((x, y)[alias], (h, w)), want)
        assert_same("the other input", words((y, x)[alias], (h, w)), H.bits((b, a)[alias]))
