"""Mesh render, the part that needs no GPU: the header, the loader and the binders name the entry points, every refusal of
include/ssrlcv_hip.h "mesh render" is decided on the host in the contract's order before a buffer is looked at (the device pointers
here are bogus or null, so nothing is launched), the workspace query follows the header's formula, empty grids and views need
nothing, the kernels use no scratch, the difference statistics leave out exactly the pattern the residual writes, and the tool and
the documents exist."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import helpers as H
from test_dsm_host import BOGUS, INF, INVALID_ARG, NAN, OK, WORKSPACE, a256

u32, f32, csz, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
QUERY = "ssrlcv_hip_mesh_render_workspace_bytes"
NAMES = [QUERY, "ssrlcv_hip_mesh_render", "ssrlcv_hip_image_residual"]


@pytest.fixture(scope="module")
def lib():
    from ssrlcv_amd import _lib
    lb = _lib.load()
    getattr(lb, QUERY).restype = csz
    return lb


def cview(w=96, h=64, **change):
    """an OrthoView with a bogus image and a NaN eye, which the render ignores; M3=NAN, pos1=INF change an entry"""
    from ssrlcv_amd import capi
    v = capi.OrthoView(BOGUS, w, h, (f32 * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (f32 * 3)(0, 0, 0), (f32 * 3)(NAN, NAN, NAN))
    for k, x in change.items():
        (v.M if k[0] == "M" else v.pos)[int(k.lstrip("Mpos"))] = x
    return v


def render(lib, view=True, prm=True, max_extent=8, n=1000, gw=64, gh=48, points=BOGUS, grey=BOGUS + 0x100, vertex_index=BOGUS + 0x200, cells=BOGUS + 0x300,
           depth=BOGUS + 0x400, triangle=BOGUS + 0x500, shade=BOGUS + 0x600, counts=BOGUS + 0x700, ws=BOGUS + 0x800, ws_bytes=1 << 50, **view_args):
    from ssrlcv_amd import capi
    v = ctypes.byref(cview(**view_args)) if view else None
    p = ctypes.byref(capi.RenderParams(max_extent)) if prm else None
    return lib.ssrlcv_hip_mesh_render(vp(points), u32(n), vp(grey), vp(vertex_index), vp(cells), u32(gw), u32(gh), v, p, vp(depth), vp(triangle), vp(shade),
                                      vp(counts), vp(ws), csz(ws_bytes), vp(None))


def residual(lib, w=96, h=64, image=BOGUS, shade=BOGUS + 0x100, depth=BOGUS + 0x200, out=BOGUS + 0x300):
    return lib.ssrlcv_hip_image_residual(vp(image), vp(shade), vp(depth), u32(w), u32(h), vp(out), vp(None))


def formula(n, w, h):
    """the header's: 256 + a256(8 w h) + a256(16 n)"""
    return 256 + a256(8 * w * h) + a256(16 * n)


NULL_ALL = dict(points=None, grey=None, vertex_index=None, cells=None, depth=None, triangle=None, shade=None, counts=None, ws=None, ws_bytes=0)


def test_header_loader_and_binders_name_the_entry_points():
    from ssrlcv_amd import _lib, capi, pipeline
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name), name
    assert "#define SSRLCV_HIP_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4      # additions keep the number
    assert "mesh render: mesh_render (+ its workspace query), image_residual" in re.sub(r"\n \*\s+", " ", header[:header.index("#define SSRLCV_HIP_ABI_VERSION")])
    reg_at, at, over_at = header.index("---- surface registration"), header.index("---- mesh render"), header.index("int ssrlcv_sift_plan_overflow")
    assert reg_at < header.index("int ssrlcv_register_compose_host(") < at < over_at
    section = re.sub(r"\n \*\s+", " ", header[at:over_at])
    for text in ("word for word", "iw = 1.0f / W", "W > 0, W <= 2^60", "fabsf(sx) <= 1048576", "and iw is finite", "fx = (int32)rintf(sx * 256.0f)", "ties to even",
                 "(256 x, 256 y)", "2 cellIndex + t", "E(a, b; c) = (b.x - a.x) (c.y - a.y) - (b.y - a.y) (c.x - a.x)", "max - min > 256 maxExtent",
                 "under 2^29", "A = E(p, q; r) = 0", "no face culling", "Edges are inclusive", "no fill rule", "lp = (float)Ep / (float)A",
                 "v = ((lp iwp) + (lq iwq)) + (lr iwr)", "smallest id", "1.0f / v", "floorf((((lp gp) + (lq gq)) + (lr gr)) + 0.5f)", "clamped to 0 .. 255",
                 "(float)image - (float)shade", "256 + a256(8 w h) + a256(16 n)", "INTEGER atomics", "(bits(v) << 32) | (0xFFFFFFFF - id)", "bit-equal run to run",
                 "no host synchronisation", "perspective-correct shading", "near-plane clipping", "triangles above 64 pixels", "anti-aliasing", "pushbroom views",
                 "triangle soups", "predicted disparities", "ssrlcv_render_params; /* 4 bytes */"):
        assert text in section, text
    assert ctypes.sizeof(capi.RenderParams) == 4 and capi.RENDER_NO_TRIANGLE == 0xFFFFFFFF
    sig = inspect.signature
    assert list(sig(capi.mesh_render).parameters) == ["points_d", "vertex_index_d", "cells_d", "view", "grey_d", "max_extent", "want_triangle", "want_shade", "workspace"]
    assert list(sig(capi.image_residual).parameters) == ["image_d", "shade_d", "depth_d", "out"]
    assert list(sig(pipeline.surface_render).parameters) == ["model_or_height", "frame", "camera", "colors", "max_jump", "max_extent"]
    defaults = {k: p.default for k, p in sig(pipeline.surface_render).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(colors=None, max_jump=None, max_extent=8)
    assert list(sig(pipeline.surface_photo_check).parameters)[:5] == ["model", "frame", "ortho", "image", "camera"]


def test_render_refusals_in_the_contract_s_order(lib):
    # the parameters and the view, before any size and any buffer
    too_many = dict(w=65536, h=32768)
    for bad in (dict(prm=False), dict(max_extent=0), dict(max_extent=65), dict(max_extent=0xFFFFFFFF), dict(view=False), dict(M0=NAN), dict(M8=INF), dict(M4=-INF),
                dict(pos0=NAN), dict(pos2=INF)):
        assert render(lib, **bad) == INVALID_ARG, bad
        assert render(lib, **NULL_ALL, **bad) == INVALID_ARG, bad
        if "view" not in bad:
            assert render(lib, **too_many, **bad) == INVALID_ARG, bad
            assert render(lib, w=0, h=0, **NULL_ALL, **bad) == INVALID_ARG, bad          # before the empty view is accepted
    # the sizes: the view, then the grid, before the empty view and before any buffer
    assert render(lib, **too_many) == INVALID_ARG and render(lib, **too_many, **NULL_ALL) == INVALID_ARG
    assert render(lib, w=1 << 31, h=1, **NULL_ALL) == INVALID_ARG and render(lib, w=46341, h=46341, **NULL_ALL) == INVALID_ARG
    assert render(lib, gw=65536, gh=32768) == INVALID_ARG and render(lib, w=0, h=5, gw=65536, gh=32768, **NULL_ALL) == INVALID_ARG
    # an empty view needs nothing (counts NULL here: nothing is written at all)
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert render(lib, w=w, h=h, **NULL_ALL) == OK
    # the buffers: depth and the workspace always ...
    short = dict(ws_bytes=0)
    assert render(lib, depth=None, **short) == INVALID_ARG and render(lib, ws=None, **short) == INVALID_ARG
    # ... the mesh and the points where something can be drawn ...
    for missing in ("points", "vertex_index", "cells"):
        assert render(lib, **{missing: None}, **short) == INVALID_ARG, missing
        for nothing in (dict(n=0), dict(gw=1), dict(gh=1), dict(gw=0, gh=0)):
            assert render(lib, **{missing: None}, **nothing, **short) == WORKSPACE, (missing, nothing)
    # ... and the optional ones never: then the size of the workspace
    assert render(lib, grey=None, triangle=None, shade=None, counts=None, **short) == WORKSPACE
    for n, w, h in ((1000, 96, 64), (0, 1, 1), (1, 65, 3)):
        assert render(lib, n=n, w=w, h=h, ws_bytes=formula(n, w, h) - 1) == WORKSPACE


def test_the_workspace_formula(lib):
    q = getattr(lib, QUERY)
    for n, w, h in ((0, 0, 0), (0, 1, 1), (1, 1, 1), (16, 32, 1), (17, 33, 1), (1000, 96, 64), (4096 * 4096, 4096, 4096), (0xFFFFFFFF, 46340, 46340),
                    (5, 0, 9), (5, 1 << 24, 127)):
        assert q(u32(n), u32(w), u32(h)) == formula(n, w, h), (n, w, h)
    assert formula(0xFFFFFFFF, 46340, 46340) > 1 << 36                                  # computed in size_t
    for w, h in ((65536, 32768), (1 << 31, 1), (46341, 46341), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert q(u32(7), u32(w), u32(h)) == 0, (w, h)


def test_residual_refusals(lib):
    assert residual(lib, w=65536, h=32768) == INVALID_ARG and residual(lib, w=65536, h=32768, image=None, shade=None, depth=None, out=None) == INVALID_ARG
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert residual(lib, w=w, h=h, image=None, shade=None, depth=None, out=None) == OK
    for missing in ("image", "shade", "depth", "out"):
        assert residual(lib, **{missing: None}) == INVALID_ARG, missing


def test_the_statistics_leave_out_exactly_the_residual_s_pattern():
    """"surface accuracy" item 2, validity: an entry is valid iff its bits are not 0x7FC00000 -- the pattern ssrlcv_hip_image_residual
    writes where nothing was drawn, and no other NaN; accuracy.hip is used as it is"""
    header = open(os.path.join(H.ROOT, "include", "ssrlcv_hip.h")).read()
    accuracy = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header[header.index("---- surface accuracy"):header.index("---- surface registration")]))
    assert "validity an entry is valid iff its bits are not 0x7FC00000" in accuracy
    source = open(os.path.join(H.ROOT, "ssrlcv_amd", "csrc", "render.hip")).read()
    assert "depth[px] != kNaN ? __float_as_uint((float)image[px] - (float)shade[px]) : kNaN" in source and "kNaN = 0x7FC00000u" in source


def test_the_kernels_use_no_scratch():
    """the method of tests/test_capi_symbols.py test_matcher_kernels_register_budget: the compiler's resource report"""
    csrc = os.path.join(H.ROOT, "ssrlcv_amd", "csrc")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
                          "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(csrc, "render.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    kernels = {k: [v for n, v in usage.items() if k in n] for k in ("k_render_project", "k_render_scatter", "k_render_resolve", "k_image_residual")}
    for k, found in kernels.items():
        assert len(found) == 1 and found[0]["ScratchSize [bytes/lane]"] == 0 and found[0]["VGPRs Spill"] == 0, (k, found)
        assert found[0]["LDS Size [bytes/block]"] == (48 if k == "k_render_scatter" else 0), (k, found)      # the block's three counts
        print("%s: %d VGPRs, %d waves/SIMD" % (k, found[0]["VGPRs"], found[0]["Occupancy [waves/SIMD]"]))
        assert found[0]["Occupancy [waves/SIMD]"] >= 7, (k, found)


def test_the_mirror_program_compiles_and_the_class_api_names_the_calls():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/render_test"])
    r = subprocess.run([os.path.join(host, "_build", "render_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    factory = open(os.path.join(host, "MeshFactory.hpp")).read()
    for member in ("RenderedView renderView(const Image::Camera& camera", "PhotoConsistency photoConsistency(ptr::value<Unity<unsigned char>> image, const Image::Camera& camera",
                   "ssrlcv_hip_mesh_render(", "ssrlcv_hip_image_residual(", "ssrlcv_hip_difference_stats("):
        assert member in factory, member


def test_the_documents_and_the_bench_tool_exist():
    root = H.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "Mesh render" in design
    for kernel in ("k_render_project", "k_render_scatter", "k_render_resolve", "k_image_residual"):
        assert kernel in design, kernel
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(root, doc)).read()
        assert "ssrlcv_hip_mesh_render" in text and "ssrlcv_hip_image_residual" in text and "surface_photo_check" in text, doc
    assert "render_bench.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(root, "tools", "bench_render.py"))
    source = open(os.path.join(root, "ssrlcv_amd", "csrc", "render.hip")).read()
    assert "atomicAdd(float" not in source and "unsafeAtomicAdd" not in source and "atomicAdd(double" not in source      # no float atomic
    assert '#include "mesh_corners.h"' in source and '#include "mesh_corners.h"' in open(os.path.join(root, "ssrlcv_amd", "csrc", "mesh.hip")).read()
