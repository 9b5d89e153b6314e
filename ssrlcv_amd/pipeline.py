"""N-view reconstruction flow (BASELINE.json configs[1..4]) over the HIP C ABI, single- or multi-GPU.

Mirrors src/Pipeline.cu doFeatureGeneration -> doFeatureMatching -> doTriangulation (+ the bundle-adjustment error
sweep of doBundleAdjust) with the sharding of ssrlcv_amd/dist.py:

  stage A   SIFT per image on its owner rank                         exchange 1: all-gather of the feature arrays
  stage B   pair matching on the pair's owner rank (pairs balanced   exchange 2: all-gather of the uint2_pair arrays
            by nq * nt, all queued, one synchronisation)
  merge     generateMatchesExhaustive's merge on the device, replicated (deterministic: csrc/merge.hip); KeyPoint table
            gathered on the device
  stage C   bundle-range triangulation                                exchange 3: all-gather of the cloud
  BA sweep  the K finite-difference evaluations of f(cameras) over this rank's bundle range of the first image pair
            (calculateImageGradient / Hessian, src/PointCloudFactory.cu:1059-1504)   all-reduce(sum) of the K sums

With world size 1 (no process group) every exchange is the identity.  Python here is plumbing (device buffers,
torch.distributed); all compute is libssrlcv_hip.so.  A `Workspace` keeps the per-rank plans, matcher workspaces and
seed descriptors between calls: creating and freeing them per pair / per image was a third of a step.
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as tdist

from . import capi
from . import dist as sd

KEYPOINT = np.dtype([("parentId", "<i4"), ("pad", "<i4"), ("loc", "<f4", (2,))])
MULTIMATCH = np.dtype([("numKeyPoints", "<u4"), ("index", "<i4")])
FEATURE_BYTES = 152


def _world():
    if tdist.is_available() and tdist.is_initialized():
        return tdist.get_world_size(), tdist.get_rank()
    return 1, 0


class Workspace:
    """Per-rank cache: SIFT plans by image size, one grow-only matcher workspace / output buffer, the seed features on
    the device.  One flow at a time per Workspace."""

    def __init__(self):
        self.plans = {}
        self._plan_bytes = {}
        self.match_ws = None
        self.match_out = None
        self.match2_ws = None
        self.seed = None
        self.seed_key = None
        self.times = {}

    def plan(self, w, h, slot=0):
        key = (w, h, slot)
        if key not in self.plans:
            self.plans[key] = capi.SiftPlan(w, h)
        return self.plans[key]

    def plan_bytes(self, w, h):
        """Workspace + feature buffer a plan of this size holds (from a layout-only plan: no device memory)."""
        key = (w, h)
        if key not in self._plan_bytes:
            probe = capi.SiftPlan(w, h, alloc=False)
            self._plan_bytes[key] = probe.workspace_bytes + probe.max_features * FEATURE_BYTES
        return self._plan_bytes[key]

    def matcher(self, shapes, out_bytes):
        need = max(capi.LIB.ssrlcv_hip_match_workspace_bytes(capi.c_u32(nq), capi.c_u32(nt)) for nq, nt in shapes)
        if self.match_ws is None or self.match_ws.numel() < need:
            self.match_ws = capi.dev_bytes(need)
        if self.match_out is None or self.match_out.numel() < out_bytes:
            self.match_out = capi.dev_bytes(out_bytes)
        return self.match_ws, self.match_out

    def seed_features(self, seed_np):
        if seed_np is None:
            return None
        key = (id(seed_np), len(seed_np))
        if self.seed_key != key:
            self.seed, self.seed_key = capi.to_dev(seed_np), key
        return self.seed

    def tick(self, name, t0):
        self.times[name] = self.times.get(name, 0.0) + (time.perf_counter() - t0)


def extract_features(pixel_tensors, ws=None, plan_budget_bytes=None):
    """SIFT on the images this rank owns.  pixel_tensors: {image index: u8 CUDA tensor (H, W)} -> {index: feature bytes}.
    While the plans' workspaces fit the budget (default: 40 % of the device's memory) every owned image gets its own plan
    and the extracts are queued back to back and synchronised once; past it (eight 8192^2 views on one GPU need 8 x 22 GB)
    one plan per image size is reused: extract, copy the features out, next image."""
    ws = ws or Workspace()
    if plan_budget_bytes is None:
        plan_budget_bytes = int(0.4 * torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory)
    items = list(pixel_tensors.items())
    need = 0
    for k, (v, pix) in enumerate(items):
        h, w = pix.shape
        need += ws.plan_bytes(w, h)
    out = {}
    if need <= plan_budget_bytes:
        plans = {}
        for k, (v, pix) in enumerate(items):
            h, w = pix.shape
            plans[v] = ws.plan(w, h, k)
            plans[v].extract(pix)
        for v, plan in plans.items():
            n = plan.count()   # synchronises; raises if a key-point list overflowed
            out[v] = plan.features[: n * FEATURE_BYTES].clone()
        return out
    for v, pix in items:
        h, w = pix.shape
        plan = ws.plan(w, h, 0)
        plan.extract(pix)
        n = plan.count()
        out[v] = plan.features[: n * FEATURE_BYTES].clone()
    return out


def extract_features_dense(pixel_tensors, stride=1, sigma=1.6, max_orientations=2, orientation_threshold=0.8,
                           orientation_contrib_width=1.5, descriptor_contrib_width=6.0):
    """Dense SIFT on the images this rank owns: one key point every `stride` pixels, all at scale `sigma`, on the image itself
    (capi.sift_dense).  Same shape as extract_features -- {image index: u8 CUDA tensor (H, W)} -> {index: feature bytes} --
    so the result goes into match_pairs / two_view_uncalibrated unchanged.  One workspace serves images of one size."""
    out, workspaces = {}, {}
    for v, pix in pixel_tensors.items():
        h, w = pix.shape
        p = capi.DenseParams(stride, sigma, max_orientations, orientation_threshold, orientation_contrib_width, descriptor_contrib_width)
        capi.dense_grid(w, h, p)
        if (w, h) not in workspaces:
            workspaces[(w, h)] = capi.dense_workspace(w, h, p)
        feats, n = capi.sift_dense(pix, stride, sigma, max_orientations, orientation_threshold, orientation_contrib_width,
                                   descriptor_contrib_width, workspace=workspaces[(w, h)])
        out[v] = feats[: n * FEATURE_BYTES].clone()
    return out


def stereo_disparity(left, right, radius=4, min_disparity=0, num_disparities=64, max_cost=capi.STEREO_NO_LIMIT, lr_tolerance=1,
                     subpixel=True, want_cost=True, census=0):
    """Dense stereo on a rectified pair (u8 CUDA tensors (H, W)): SAD block matching over (2 radius + 1)^2 windows, the
    disparities min_disparity .. min_disparity + num_disparities - 1, with the cost limit, left-right check and sub-pixel
    step of include/ssrlcv_hip.h "dense stereo".  census = 1, 2 or 3: the cost is the Hamming distance of (2 census + 1)^2
    census codes instead ("census cost"), unchanged by any strictly increasing map of either image's grey levels; `radius` is then the
    AGGREGATION radius, 0 .. 7, and the footprint is radius + census.  -> (disparity float32 (H, W), cost or None): invalid
    pixels hold the bit pattern capi.STEREO_INVALID_BITS (a NaN) and cost 0xFFFFFFFF."""
    return capi.stereo_disparity(left, right, radius, min_disparity, num_disparities, max_cost, lr_tolerance, subpixel, want_cost, census=census)


def stereo_sgm(left, right, radius=2, min_disparity=0, num_disparities=64, cost_clamp=1000, p1=40, p2=400, paths=0xFF, lr_tolerance=1,
               subpixel=True, want_cost=False, census=0):
    """Dense stereo by semi-global matching on a rectified pair (u8 CUDA tensors (H, W)): the SAD costs of stereo_disparity,
    clamped at cost_clamp, aggregated along the directions of the bit mask `paths` (0x0F: 4 paths, 0xFF: 8) with the penalties
    p1 <= p2, then the winner, left-right check and sub-pixel step on the summed costs (include/ssrlcv_hip.h "semi-global
    matching"; popcount(paths) (cost_clamp + p2) <= 65535).  census = 1, 2 or 3: the census costs of stereo_disparity instead,
    `radius` then being the AGGREGATION radius, 0 .. 7 (0: each pixel's own Hamming distance, the usual form here).
    -> (disparity float32 (H, W), cost or None) like stereo_disparity."""
    return capi.stereo_sgm(left, right, radius, min_disparity, num_disparities, cost_clamp, p1, p2, paths, lr_tolerance, subpixel, want_cost,
                           census=census)


def _dense_disparity(left, right, sgm, disparity_args):
    """stereo_cloud's and stereo_cloud_cameras' disparity map: SAD winners, or semi-global matching when sgm is a dict"""
    if sgm is None:
        return stereo_disparity(left, right, want_cost=False, **disparity_args)[0]
    if "max_cost" in disparity_args:
        raise TypeError("semi-global matching has no cost limit: max_cost cannot be combined with sgm")
    unknown = set(sgm) - {"cost_clamp", "p1", "p2", "paths"}
    if unknown or not {"cost_clamp", "p1", "p2"} <= set(sgm):
        raise TypeError("sgm takes cost_clamp, p1, p2 and optionally paths")
    return stereo_sgm(left, right, want_cost=False, **sgm, **disparity_args)[0]


def stereo_filter(disp, cost=None, median=0, speckle_size=0, speckle_diff=1.0):
    """The map-domain post-filters of include/ssrlcv_hip.h "disparity post-filters" on a disparity map (float32 CUDA tensor
    (H, W)): median = 1 or 2 first takes every valid pixel to the lower median of the valid pixels of its (2 median + 1)^2 window
    (a new tensor; holes stay holes; the cost map is not touched); speckle_size > 0 then invalidates, in place on that result
    (on `disp` itself when no median ran) and on `cost` if given, the connected components of at most speckle_size pixels, two
    neighbours being connected when their disparities differ by at most speckle_diff.  -> the filtered map."""
    if median > 0:
        disp = capi.stereo_filter_median(disp, median)
    if speckle_size > 0:
        capi.stereo_filter_speckles(disp, cost, speckle_size, speckle_diff)
    return disp


_FILL_RULES = {"min": capi.FILL_MIN, "median": capi.FILL_MEDIAN}


def stereo_fill(disp, paths=0xFF, max_gap=32, min_hits=5, rule="min", want_mask=False):
    """Fills the holes of a disparity map (float32 CUDA tensor (H, W); include/ssrlcv_hip.h "hole filling"): a hole looks up to
    max_gap steps along each direction of the bit mask `paths` (semi-global matching's numbering) for the first measured
    pixel; with at least min_hits such sources it takes the smallest of them (rule "min": the background, which is what an
    occlusion hides) or their lower median ("median"); any other rule is a ValueError.  Only measured pixels are sources, never
    filled ones.  min_hits = 5 of 8 is the count a hole next to the image border still reaches; a pixel outside a straight edge
    of the valid region sees 3 and stays a hole.  -> the filled map, a new tensor; with want_mask (map, uint8 mask of the
    filled holes).  A cost map is not touched: a filled pixel keeps its 0xFFFFFFFF."""
    if rule not in _FILL_RULES:
        raise ValueError("rule is 'min' or 'median', not %r" % (rule,))
    out, mask = capi.stereo_fill_holes(disp, paths, max_gap, min_hits, _FILL_RULES[rule], want_mask)
    return (out, mask) if want_mask else out


def _post_filter(disp, post):
    """stereo_cloud's and stereo_cloud_cameras' post = dict(median=, speckle_size=, speckle_diff=, fill=): stereo_filter's
    arguments, and fill = dict(...) of stereo_fill's (without want_mask), which runs last"""
    if post is None:
        return disp
    unknown = set(post) - {"median", "speckle_size", "speckle_diff", "fill"}
    fill = post.get("fill")
    if unknown or (fill is not None and (not isinstance(fill, dict) or set(fill) - {"paths", "max_gap", "min_hits", "rule"})):
        raise TypeError("post takes median, speckle_size, speckle_diff and fill = dict(paths=, max_gap=, min_hits=, rule=)")
    if fill is not None and fill.get("rule", "min") not in _FILL_RULES:
        raise ValueError("rule is 'min' or 'median', not %r" % (fill["rule"],))
    disp = stereo_filter(disp, None, **{k: v for k, v in post.items() if k != "fill"})
    return disp if fill is None else stereo_fill(disp, **fill)


def stereo_cloud(left, right, foc, baseline, doffset=0.0, cx=None, cy=None, step=1, left_id=0, right_id=1, sgm=None, post=None,
                 **disparity_args):
    """Rectified pair -> dense cloud: stereo_disparity, then capi.stereo_matches (the valid pixels of the `step` grid as Match
    records), then capi.stereo_points (upstream's stereo_disparity: Z = foc baseline / (d + doffset)).  cx, cy default to the
    image centre.  disparity_args: stereo_disparity's radius, min_disparity, num_disparities, max_cost, lr_tolerance, subpixel,
    census (radius is the aggregation radius when census is set; the cost map is not computed: want_cost is not taken).  sgm = dict(cost_clamp=, p1=, p2=[, paths=]): the disparity comes
    from stereo_sgm with the remaining disparity_args (max_cost is then a TypeError).  post = dict(median=, speckle_size=,
    speckle_diff=, fill=): stereo_filter on the disparity map before the matches are taken from it, then, with fill =
    dict(paths=, max_gap=, min_hits=, rule=), stereo_fill (any other key is a TypeError); the returned map is the filtered one.  -> (points float32 (n, 3), Match bytes, n, disparity).
    The Match records are the sparse path's: with real cameras they also go through capi.matchset_from_matches and
    triangulate() unchanged (tests/test_gpu_stereo.py does)."""
    h, w = left.shape
    if "want_cost" in disparity_args:
        raise TypeError("stereo_cloud computes no cost map: call stereo_disparity for one")
    disp = _post_filter(_dense_disparity(left, right, sgm, disparity_args), post)
    matches, n = capi.stereo_matches(disp, step, left_id, right_id)
    pts = capi.stereo_points(matches, n, foc, baseline, doffset, w / 2.0 if cx is None else cx, h / 2.0 if cy is None else cy)
    return pts, matches, n, disp


def rectify_pair(left, right, cam_l, cam_r):
    """Two views (u8 CUDA tensors (H, W)) of a converging pinhole pair and their Image::Camera records -> (left_r, right_r, rect):
    the pair warped by the homographies of capi.rectify_cameras (include/ssrlcv_hip.h "rectification"), row-aligned, with
    rect's foc, baseline, doffset, cx, cy as capi.stereo_points' parameters."""
    rect = capi.rectify_cameras(cam_l, cam_r)
    shape = (int(rect["h"]), int(rect["w"]))
    assert tuple(left.shape) == shape and tuple(right.shape) == shape, "the images have the cameras' size"
    return capi.warp_homography(left, rect["Hl"], shape), capi.warp_homography(right, rect["Hr"], shape), rect


def stereo_cloud_cameras(left, right, cam_l, cam_r, step=1, sgm=None, post=None, **disparity_args):
    """Unrectified pair -> dense cloud in the world frame of triangulate()'s clouds: rectify_pair, stereo_disparity, the mask
    of the windows that left a source image (capi.stereo_mask_rectified), capi.stereo_matches, the records mapped back into
    source pixels (capi.matches_apply_homography), compacted, then capi.matchset_from_matches and the two-view triangulation
    (capi.generate_bundles, capi.triangulate) with the two original cameras.  disparity_args, sgm and post as for stereo_cloud
    (post runs behind the mask; a median-moved pixel that no longer maps back leaves with the compaction; after a fill the
    mask runs once more, so a value extrapolated to where a window leaves a source image is removed again); with
    census set, radius is the aggregation radius and the mask takes the footprint radius + census.  -> (points float32 (n, 3), Match bytes, n, disparity, rect); the
    matches are in source pixels with parent ids 0 (cam_l) and 1 (cam_r); the disparity map is the rectified left view's."""
    if "want_cost" in disparity_args:
        raise TypeError("stereo_cloud_cameras computes no cost map: call stereo_disparity for one")
    return _cloud_cameras(left, right, cam_l, cam_r, step, sgm, post, disparity_args)


def _cloud_cameras(left, right, cam_l, cam_r, step, sgm, post, disparity_args, on_records=None):
    """stereo_cloud_cameras' chain.  on_records(disp, matches, n): stereo_mesh_cameras' look at the records mapped back into
    source pixels, before the ones that did not map are compacted away"""
    left_r, right_r, rect = rectify_pair(left, right, cam_l, cam_r)
    disp = _dense_disparity(left_r, right_r, sgm, disparity_args)
    footprint = disparity_args.get("radius", 4 if sgm is None else 2) + disparity_args.get("census", 0)
    capi.stereo_mask_rectified(disp, None, footprint, rect)
    disp = _post_filter(disp, post)    # behind the mask: it removes pixels whose evidence left a source image before the filters look at neighbourhoods
    if post is not None and post.get("fill") is not None:
        capi.stereo_mask_rectified(disp, None, footprint, rect)   # the fill extrapolates past the mask's edge: the mask only removes, never adds
    matches, n = capi.stereo_matches(disp, step, 0, 1)
    capi.matches_apply_homography(matches, n, rect["Hl"], rect["Hr"])
    if on_records is not None:
        on_records(disp, matches, n)
    if n:
        n = capi.compact_matches(capi.OUT_MATCH, matches, n, capi.match_workspace(n, 1))   # a record that did not map back
        matches = matches[: 40 * n]
    pts = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    if n:
        kp_d, mm_d, _ = capi.matchset_from_matches(capi.OUT_MATCH, matches, n)
        # the two 80-byte records as bytes (numpy would repack a padded record dtype when concatenating)
        cameras = np.concatenate([capi.camera_bytes(cam_l), capi.camera_bytes(cam_r)])
        # triangulate()'s two-view path on the device copies (the dense match set never travels to the host)
        b_d, l_d = capi.generate_bundles(mm_d, kp_d, n, capi.to_dev(cameras), 2, 2 * n)
        pts = capi.triangulate(l_d, b_d, n, nview=False)[0].view(-1, 3)
    return pts, matches, n, disp, rect


def disparity_mesh(disp, step=1, max_jump=None):
    """The triangle mesh of a disparity map (float32 CUDA tensor (H, W); include/ssrlcv_hip.h "disparity mesh"): the nodes are
    the pixels of the `step` grid, the vertices its valid nodes in stereo_matches' order, and every grid cell gives up to two
    triangles, cut wherever two corners' disparities differ by more than max_jump (None: float(step), one disparity a pixel).
    -> dict(vertex_index int32 (gh, gw), -1 where there is no vertex; cells uint8 (gh - 1, gw - 1): bit 0 / 1 = the cell's first /
    second triangle exists, bit 2 = its diagonal runs b-c; n_vertices).  One synchronisation (the count)."""
    vertex_index, cells, count = capi.disparity_mesh(disp, step, float(step) if max_jump is None else max_jump)
    return {"vertex_index": vertex_index, "cells": cells, "n_vertices": int(count.item())}


def mesh_select(mesh, kept_index):
    """A mesh restricted to the vertices kept_index names (old vertex indices, strictly ascending: an integer device tensor,
    e.g. filter_cloud's `index`): vertex kept_index[j] becomes j, a triangle that loses a corner goes, nothing is
    re-triangulated.  -> a new mesh dict; `mesh` is left as it is."""
    vertex_index, cells = mesh["vertex_index"].clone(), mesh["cells"].clone()
    kept = kept_index.to(torch.int32).contiguous()
    capi.mesh_select(vertex_index, cells, mesh["n_vertices"], kept)
    return {"vertex_index": vertex_index, "cells": cells, "n_vertices": int(kept.numel())}


def mesh_faces(mesh):
    """The triangles of a mesh -> int32 (T, 3) device tensor of vertex indices, in cell raster order; every face winds so that
    its normal (q - p) x (r - p) faces the camera."""
    return capi.mesh_triangles(mesh["vertex_index"], mesh["cells"])[0]


def mesh_normals(mesh, points):
    """Unit normals of the vertices of a mesh at the positions `points` ((n, 3) float32 device tensor, row v = vertex v): the
    normalised sum of the cross products of the triangles around each vertex, facing the camera; (0, 0, 0) for a vertex without
    a triangle.  -> (n, 3) float32 device tensor.  Stream-ordered."""
    return capi.mesh_normals(points, mesh["vertex_index"], mesh["cells"])


def stereo_mesh(left, right, foc, baseline, doffset=0.0, cx=None, cy=None, step=1, left_id=0, right_id=1, sgm=None, post=None,
                max_jump=None, **disparity_args):
    """stereo_cloud with the surface: the same arguments (and the same points, matches, n and disparity), then disparity_mesh of
    the map at the same step with max_jump, its faces and the normals of the cloud's points.  Normals face the camera where
    every d + doffset is above 0 (min_disparity + doffset > 0).  -> dict(points, faces int32 (T, 3), normals, matches, n,
    disparity, mesh)."""
    pts, matches, n, disp = stereo_cloud(left, right, foc, baseline, doffset, cx, cy, step, left_id, right_id, sgm, post, **disparity_args)
    mesh = disparity_mesh(disp, step, max_jump)
    return {"points": pts, "faces": mesh_faces(mesh), "normals": mesh_normals(mesh, pts), "matches": matches, "n": n, "disparity": disp,
            "mesh": mesh}


def stereo_mesh_cameras(left, right, cam_l, cam_r, step=1, sgm=None, post=None, max_jump=None, **disparity_args):
    """stereo_cloud_cameras with the surface: the same arguments (and the same points, matches, n, disparity and rect).  The mesh
    is taken from the disparity map the records come from, restricted to the records that map back into the sources (their
    `invalid` byte, before the compaction), and only then come the faces and the normals over the world-frame points.
    -> dict(points, faces, normals, matches, n, disparity, mesh, rect)."""
    if "want_cost" in disparity_args:
        raise TypeError("stereo_mesh_cameras computes no cost map: call stereo_disparity for one")
    found = {}

    def on_records(disp, matches, n):
        mesh = disparity_mesh(disp, step, max_jump)
        kept = torch.nonzero(matches[: 40 * n].view(-1, 40)[:, 0] == 0).view(-1)   # ascending
        found["mesh"] = mesh_select(mesh, kept)

    pts, matches, n, disp, rect = _cloud_cameras(left, right, cam_l, cam_r, step, sgm, post, disparity_args, on_records)
    mesh = found["mesh"]
    return {"points": pts, "faces": mesh_faces(mesh), "normals": mesh_normals(mesh, pts), "matches": matches, "n": n, "disparity": disp,
            "mesh": mesh, "rect": rect}


_DSM_RULES = {"max": capi.DSM_MAX, "min": capi.DSM_MIN}
_DSM_FUSE_RULES = {"min": capi.DSM_FUSE_MIN, "median": capi.DSM_FUSE_MEDIAN, "max": capi.DSM_FUSE_MAX}


def dsm_frame(points, up, cell, margin=0, ex=None):
    """The ground grid of a cloud ((n, 3) float32 device tensor; include/ssrlcv_hip.h "surface model" frame): ez = `up`
    normalised, ex perpendicular to it (the given `ex` made so, or the world axis furthest from `up`), ey such that
    (ex, ey, -up) is right-handed -- x east, y south, height up -- and origin, w and h from the bounding box of the cloud's
    usable points (finite, not (0, 0, 0)) in that frame, `margin` world units wider on every side.  The origin has no component
    along ez, so a height is the point's own coordinate along `up`.  Host arithmetic on two torch reductions.
    -> capi.DsmFrame."""
    up = np.asarray(up, np.float64).reshape(3)
    up = up / np.linalg.norm(up)
    axis = np.eye(3)[int(np.argmin(np.abs(up)))] if ex is None else np.asarray(ex, np.float64).reshape(3)
    ex = axis - np.dot(axis, up) * up
    if not np.linalg.norm(ex) > 0:
        raise ValueError("ex is parallel to up")
    ex = ex / np.linalg.norm(ex)
    ey = np.cross(-up, ex)
    if not (np.isfinite(cell) and cell > 0 and np.isfinite(margin) and margin >= 0):
        raise ValueError("cell is positive and margin is not negative")
    p = points.view(-1, 3).to(torch.float64)
    p = p[torch.isfinite(p).all(1) & (p != 0).any(1)]
    if p.shape[0] == 0:
        return capi.DsmFrame.make((0, 0, 0), ex, ey, up, cell, 0, 0)
    ab = p @ torch.tensor(np.stack([ex, ey], 1), dtype=torch.float64, device=p.device)
    lo, hi = ab.min(0).values.cpu().numpy() - margin, ab.max(0).values.cpu().numpy() + margin
    w, h = (int(np.floor((hi[k] - lo[k]) / cell)) + 1 for k in range(2))
    return capi.DsmFrame.make(lo[0] * ex + lo[1] * ey, ex, ey, up, cell, w, h)


def surface_model(clouds, frame, rule="max", fuse=None, post=None):
    """The surface model of several pairs' world-frame clouds (each (n, 3) float32 device tensor, e.g. stereo_cloud_cameras'
    points) on the grid of `frame` (include/ssrlcv_hip.h "surface model"): every cloud is rasterised into its own height map
    (rule "max": the top surface, or "min"), the maps are fused per cell -- fuse = dict(min_views=1, max_spread=inf,
    rule="median"): a cell seen by at least min_views clouds whose heights agree within max_spread takes their "min", lower
    "median" or "max" -- and post (stereo_cloud's dictionary: median, speckle_size, speckle_diff, fill) then runs on the fused
    map unchanged, a height map being a disparity map in form.  -> dict(height float32 (h, w), 0x7FC00000 where there is none;
    fused: the map before post; views uint8 (h, w): the clouds that saw the cell; maps, sources, counts: one (h, w) tensor a
    cloud, sources holding the index of the winning point, -1 in an empty cell)."""
    if rule not in _DSM_RULES:
        raise ValueError("rule is 'max' or 'min', not %r" % (rule,))
    fuse = dict(fuse or {})
    if set(fuse) - {"min_views", "max_spread", "rule"}:
        raise TypeError("fuse takes min_views, max_spread and rule")
    if fuse.get("rule", "median") not in _DSM_FUSE_RULES:
        raise ValueError("fuse's rule is 'min', 'median' or 'max', not %r" % (fuse["rule"],))
    clouds = list(clouds)
    if not 1 <= len(clouds) <= 8:
        raise ValueError("1 to 8 clouds, not %d" % len(clouds))
    maps, sources, counts, ws = [], [], [], None
    for cloud in clouds:
        if ws is None:
            ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_dsm_rasterize_workspace_bytes(capi.c_u32(frame.w), capi.c_u32(frame.h))))
        height, source, count = capi.dsm_rasterize(cloud, frame, _DSM_RULES[rule], True, True, ws)
        maps.append(height), sources.append(source), counts.append(count)
    fused, views = capi.dsm_fuse(maps, fuse.get("min_views", 1), fuse.get("max_spread", float("inf")), _DSM_FUSE_RULES[fuse.get("rule", "median")])
    return {"height": _post_filter(fused, post), "fused": fused, "views": views, "maps": maps, "sources": sources, "counts": counts}


def surface_mesh(model, frame, max_jump):
    """The surface of a surface model: the valid cells of model["height"] as world-frame vertices (capi.dsm_points), the mesh of
    the height map at step 1 (two cells whose heights differ by more than max_jump are not joined), its faces and normals.
    With (ex, ey, -ez) right-handed the normals face +ez.  -> dict(points float32 (n, 3), faces int32 (T, 3), normals, mesh)."""
    height = model["height"]
    pts, n = capi.dsm_points(height, frame)
    mesh = disparity_mesh(height, 1, max_jump)
    assert mesh["n_vertices"] == n
    return {"points": pts, "faces": mesh_faces(mesh), "normals": mesh_normals(mesh, pts), "mesh": mesh}


_ORTHO_RULES = {"first": capi.ORTHO_FIRST, "median": capi.ORTHO_MEDIAN}


def surface_ortho(model_or_height, frame, images, cameras, max_steps=256, bias=None, rule="first"):
    """The ortho-image of a surface model (surface_model's dictionary, or its height map alone) from 1 to 8 source images (uint8
    (h, w) device tensors) and their Image::Camera records (include/ssrlcv_hip.h "ortho-image"): every valid cell of the
    filled map -- cells the fill or the median created included -- takes the grey of the "first" view, in the order given, that
    sees it, or the lower "median" of the views that do.  A view sees a cell if the cell projects into its image and no height
    within max_steps cells towards the camera stands more than `bias` above the line of sight (None: half a cell).
    -> dict(ortho uint8 (h, w), 0 where no view sees the cell; seen uint8 (h, w): bit k = view k sees it; which uint8 (h, w): the
    view the grey came from, 0xFF for none)."""
    if rule not in _ORTHO_RULES:
        raise ValueError("rule is 'first' or 'median', not %r" % (rule,))
    images, cameras = list(images), list(cameras)
    if not 1 <= len(images) <= 8 or len(images) != len(cameras):
        raise ValueError("1 to 8 images and as many cameras, not %d and %d" % (len(images), len(cameras)))
    height = model_or_height["height"] if isinstance(model_or_height, dict) else model_or_height
    views = [capi.dsm_ortho_view(cam, frame) for cam in cameras]
    ortho, seen, which = capi.dsm_ortho(height, frame, views, images, max_steps, 0.5 * float(frame.cell) if bias is None else bias, _ORTHO_RULES[rule])
    return {"ortho": ortho, "seen": seen, "which": which}


def surface_colors(ortho, height):
    """The ortho-image's bytes of the valid cells of `height` in raster order: one grey a vertex of capi.dsm_points and of
    surface_mesh (the mesh's numbering at step 1).  -> uint8 (n,) device tensor."""
    assert ortho.shape == height.shape and ortho.dtype == torch.uint8 and height.dtype == torch.float32
    return ortho[height.view(torch.int32) != capi.STEREO_INVALID_BITS]


def surface_render(model_or_height, frame, camera, colors=None, max_jump=None, max_extent=8):
    """The surface of a surface model (surface_model's dictionary, or its height map alone) drawn into the view of an Image::Camera
    record (include/ssrlcv_hip.h "mesh render"): the valid cells as vertices (capi.dsm_points), the mesh of the map at step 1, cut
    where two cells differ by more than max_jump (None: nowhere), z-buffered into the camera's image.  colors: one grey a vertex
    (surface_colors'), or None.  A triangle above max_extent pixels is skipped and counted.
    -> dict(depth float32 (h, w): the distance along the optical axis, 0x7FC00000 where nothing was drawn; triangle int32 (h, w):
    2 cell + t of the grid's cell raster, -1 for none; shade uint8 (h, w); counts: dict(drawn, too_large, unusable))."""
    height = model_or_height["height"] if isinstance(model_or_height, dict) else model_or_height
    pts, n = capi.dsm_points(height, frame)
    vertex_index, cells, _ = capi.disparity_mesh(height, 1, float("inf") if max_jump is None else max_jump)
    depth, triangle, shade, counts = capi.mesh_render(pts, vertex_index, cells, capi.dsm_ortho_view(camera, frame), colors, max_extent)
    drawn, too_large, unusable = (int(c) for c in counts.cpu().tolist())
    return {"depth": depth, "triangle": triangle, "shade": shade, "counts": {"drawn": drawn, "too_large": too_large, "unusable": unusable}}


def surface_simplify(model_or_height, frame, tolerance, errors=None, colors=None, normals=None):
    """The surface of a surface model (surface_model's dictionary, or its height map alone) thinned to a right-triangle mesh whose
    midpoint errors stay within `tolerance`, in the map's height units (include/ssrlcv_hip.h "surface simplification"): full
    resolution where the map is rough and at hole boundaries, large triangles where it is flat.  No vertex is created: the
    points are capi.dsm_points' gathered by `kept`.  errors: capi.dsm_simplify_errors' map of the same height map from an earlier
    call -- it does not depend on the tolerance --, or None.  colors (surface_colors'), normals (surface_mesh's): one a vertex of
    the full mesh, gathered too where given.
    -> dict(points float32 (m, 3), faces int32 (T, 3) indexing them, kept int32 (m,): the vertices' indices in capi.dsm_points'
    numbering, strictly ascending; vertex_index int32 (h, w): a kept cell's new index, -1 elsewhere; errors; colors, normals)."""
    height = model_or_height["height"] if isinstance(model_or_height, dict) else model_or_height
    pts, n = capi.dsm_points(height, frame)
    node_index = capi.disparity_mesh(height, 1, float("inf"))[0]
    errors = capi.dsm_simplify_errors(height) if errors is None else errors
    faces, _, kept, _, vertex_index = capi.dsm_simplify_mesh(height, errors, tolerance, node_index)
    gather = kept.to(torch.int64)
    out = {"points": pts[gather], "faces": faces, "kept": kept, "vertex_index": vertex_index, "errors": errors}
    if colors is not None:
        out["colors"] = colors[gather]
    if normals is not None:
        out["normals"] = normals.view(-1, 3)[gather]
    return out


def terrain_schedule(cell, max_radius, slope, initial, maximum, radii=None):
    """The windows and thresholds of the progressive morphological filter (Zhang et al. 2003) for capi.dsm_terrain; host only.
    cell: the side of a cell in the map's height units; slope: the steepest terrain to keep, rise over run; initial, maximum: the
    first and the largest threshold.  radii default to 1, 2, 4, ... with max_radius as the last entry if it is not one of them;
    ValueError if that takes more than 8 levels -- pass `radii` then.  t_1 = initial, t_k = min(initial + slope cell 2 (r_k -
    r_{k-1}), maximum): Zhang's dh_k for windows of 2r + 1 cells, computed in double and rounded to float32 once.
    -> (radii, thresholds): lists of int and of float."""
    if radii is None:
        radii, r = [], 1
        while r < int(max_radius):
            radii.append(r)
            r *= 2
        radii.append(int(max_radius))
    radii = [int(r) for r in radii]
    if not 1 <= len(radii) <= 8:
        raise ValueError("the filter has 1 to 8 levels, not %d: pass radii" % len(radii))
    if radii[0] < 1 or any(b <= a for a, b in zip(radii, radii[1:])):
        raise ValueError("radii are at least 1 and strictly ascending, not %r" % (radii,))
    thresholds = [float(np.float32(float(initial)))]
    for a, b in zip(radii, radii[1:]):
        thresholds.append(float(np.float32(min(float(initial) + float(slope) * float(cell) * 2.0 * (b - a), float(maximum)))))
    return radii, thresholds


def surface_terrain(model_or_height, frame, max_radius, slope, initial, maximum, radii=None,
                    fill=dict(paths=0xFF, max_gap=None, min_hits=1, rule="median"), want_level=True):
    """The bare earth under a surface model (surface_model's dictionary, or its height map alone) and the heights of what stands
    on it (include/ssrlcv_hip.h "terrain filter"): the progressive morphological filter on terrain_schedule(frame.cell,
    max_radius, slope, initial, maximum, radii), the footprints it cuts out closed by capi.stereo_fill_holes -- fill =
    dict(paths=, max_gap=, min_hits=, rule=), max_gap None for no limit; fill=None leaves them open --, and height - terrain.
    An object that holds a whole window of max_radius is ground: choose max_radius above half the widest building, in cells.
    -> dict(ground: bool (h, w), the valid cells no level flagged; level: uint8 (h, w) or None, 0 ground, k the first level that
    flagged the cell, 255 no cell; bare: the height at the ground cells, 0x7FC00000 elsewhere; terrain: `bare` with its holes
    filled; objects: height - terrain; radii, thresholds).  `terrain` is a height map like any other: surface_mesh and
    surface_simplify take dict(height=terrain), surface_accuracy measures it against a bare-earth reference, and
    difference_stats(objects) gives the statistics of the object heights."""
    height = model_or_height["height"] if isinstance(model_or_height, dict) else model_or_height
    radii, thresholds = terrain_schedule(float(frame.cell), max_radius, slope, initial, maximum, radii)
    bare, level, _ = capi.dsm_terrain(height, radii, thresholds, want_level=want_level)
    terrain = bare
    if fill is not None:
        if not isinstance(fill, dict) or set(fill) - {"paths", "max_gap", "min_hits", "rule"}:
            raise TypeError("fill = dict(paths=, max_gap=, min_hits=, rule=) or None")
        if fill.get("rule", "median") not in _FILL_RULES:
            raise ValueError("rule is 'min' or 'median', not %r" % (fill["rule"],))
        gap = fill.get("max_gap")
        terrain = capi.stereo_fill_holes(bare, fill.get("paths", 0xFF), capi.FILL_NO_LIMIT if gap is None else gap, fill.get("min_hits", 1),
                                         _FILL_RULES[fill.get("rule", "median")])[0]
    ground = bare.view(torch.int32) != 0x7FC00000
    return {"ground": ground, "level": level, "bare": bare, "terrain": terrain, "objects": capi.dsm_subtract(height, terrain),
            "radii": radii, "thresholds": thresholds}


_MEASURES = ("area", "perimeterLength", "compactness", "centroidX", "centroidY", "meanHeight", "volume", "rmsHeight", "mxx", "mxy", "myy",
             "lambdaMajor", "lambdaMinor", "axisX", "axisY", "elongation")


def surface_objects(terrain_or_objects, frame, min_height, max_diff=float("inf"), min_cells=1, scale=256.0):
    """What stands on the terrain (include/ssrlcv_hip.h "surface objects"): the inventory of surface_terrain's dictionary, or of its
    `objects` map alone.  An object is a 4-connected footprint of cells at least min_height above the ground, joined where
    neighbours differ by at most max_diff (inf: a footprint whatever its roof does); those of fewer than min_cells cells are
    dropped; heights are summed as rint(height x scale).  A first call counts the objects, a second one writes their records.
    -> dict(count; ids int32 (h, w): the object's number, in raster order of the objects' first cells, -1 for a cell of none;
    records: a capi.OBJECT_RECORD array; measures: one dictionary a record -- area, perimeterLength, compactness, centroidX,
    centroidY, world (3 floats), meanHeight, volume, rmsHeight, mxx, mxy, myy, lambdaMajor, lambdaMinor, axisX, axisY, elongation
    -- in the frame's units, from capi.object_measures)."""
    objects = terrain_or_objects["objects"] if isinstance(terrain_or_objects, dict) else terrain_or_objects
    count, ids, records = capi.dsm_objects(objects, min_height, max_diff, int(min_cells), scale)
    measures = []
    for record in records:
        m = capi.object_measures(record, frame, scale)
        measures.append(dict({name: float(getattr(m, name)) for name in _MEASURES}, world=[float(v) for v in m.world]))
    return {"count": count, "ids": ids, "records": records, "measures": measures}


def surface_photo_check(model, frame, ortho, image, camera, max_jump=None, max_extent=8, want_map=False):
    """How well a textured surface model predicts a view's own pixels -- an accuracy measure that needs no reference surface: the
    model's mesh takes the greys of its ortho-image (surface_colors of surface_ortho's `ortho`), is drawn into `camera`
    (surface_render) and subtracted from `image` (uint8 (h, w) device tensor, the camera's picture: a view held out of the
    ortho-image is an independent check); the residuals go through difference_stats as they are.
    -> dict(coverage: the share of the image's pixels the model covers; median: of the residuals, image minus model, in grey
    levels; nmad = 1.4826 x the median absolute deviation about it, host float64; rms; counts: surface_render's); with want_map
    also residual: float32 (h, w), 0x7FC00000 where nothing was drawn."""
    height = model["height"] if isinstance(model, dict) else model
    drawn = surface_render(height, frame, camera, surface_colors(ortho, height), max_jump, max_extent)
    residual = capi.image_residual(image, drawn["shade"], drawn["depth"])
    signed = difference_stats(residual, quantiles=(5000,))
    nan = float("nan")
    median = signed["quantiles"][0] if signed["finite"] else nan
    mad = difference_stats(residual, center=median, absolute=True, quantiles=(5000,))["quantiles"][0] if signed["finite"] else nan
    out = {"coverage": signed["finite"] / signed["n"] if signed["n"] else nan, "median": median, "nmad": float(np.float64(1.4826) * np.float64(mad)),
           "rms": signed["rms"], "counts": drawn["counts"]}
    if want_map:
        out["residual"] = residual
    return out


def surface_difference(points, reference, frame, mesh=True, max_jump=None):
    """The signed height difference of every point of a cloud ((n, 3) float32 device tensor) to a reference height map (float32
    (h, w) device tensor in `frame`; include/ssrlcv_hip.h "surface accuracy" item 1), positive above the reference along the
    frame's ez.  With `mesh` the reference is the triangle mesh of the map at step 1, cut where two cells differ by more than
    max_jump (None: nowhere); without, the height of the cell under the point.  -> float32 (n,) device tensor, 0x7FC00000 where
    there is no difference."""
    cells = capi.disparity_mesh(reference, 1, float("inf") if max_jump is None else max_jump)[1] if mesh else None
    return capi.dsm_difference(points, reference, frame, cells)


def difference_stats(diff, center=0.0, absolute=False, quantiles=(5000,)):
    """Exact statistics of a tensor of differences ("surface accuracy" item 2): the valid entries become y = x - center (|y| with
    `absolute`), and over the finite y -> dict(n, valid, finite, sum, sum_sq, min, max, quantiles: one float a quantile, in parts
    per 10000, each one of the inputs; mean and rms in host float64 from sum, sum_sq and finite, nan when finite is 0)."""
    quantiles = tuple(quantiles)
    rec = capi.difference_stats(diff, center, absolute, quantiles)
    m = int(rec.finite)
    mean = float(np.float64(rec.sum) / np.float64(m)) if m else float("nan")
    rms = float(np.sqrt(np.float64(rec.sumSq) / np.float64(m))) if m else float("nan")
    return {"n": int(rec.n), "valid": int(rec.valid), "finite": m, "sum": float(rec.sum), "sum_sq": float(rec.sumSq), "min": float(rec.min),
            "max": float(rec.max), "quantiles": [float(rec.quantile[k]) for k in range(len(quantiles))], "mean": mean, "rms": rms}


_REGISTER_DOF = {"shift": capi.REGISTER_SHIFT, "rigid": capi.REGISTER_RIGID, "similarity": capi.REGISTER_SIMILARITY}


def transform_cloud(points, pose):
    """A pose (capi.RegisterPose: p' = M p + T) applied to a cloud ((n, 3) float32 device tensor; include/ssrlcv_hip.h "surface
    registration" item 2).  "No result" points stay what they are.  -> a new (n, 3) float32 device tensor."""
    return capi.transform_points(points, pose)


def _pose64(pose):
    m = np.array(list(pose.m), np.float64).reshape(3, 4)
    return m[:, :3], m[:, 3]


def surface_register(points, reference, frame, max_jump=None, dof="rigid", iterations=8, gate=3.0, initial=None, damping=0.0):
    """The pose that aligns a cloud ((n, 3) float32 device tensor) to a reference height map (float32 (h, w) device tensor in
    `frame`) by point-to-plane Gauss-Newton steps (include/ssrlcv_hip.h "surface registration").  The reference is the triangle
    mesh of the map at step 1, cut where two cells differ by more than max_jump (None: nowhere).  dof: "shift" (translation),
    "rigid" (and rotation), "similarity" (and scale), or a mask of capi.register_step's bits.  initial: a capi.RegisterPose to
    start from (None: the identity); from many cells off, surface_register_coarse finds it by a coarse search first.  The pivot is the float64 mean of the points
    that have a difference under the initial pose, rounded to float.  Every iteration: with a gate (None: without), one
    surface_difference of the posed cloud and two statistics calls give center = the median and width = gate x NMAD, and only
    points with |d - center| <= width take part; then one capi.register_terms (one 304-byte read-back), capi.register_step with
    `damping`, capi.register_compose.  The loop ends early when a step is refused, or -- converged -- when a step moves no corner
    of the cloud's bounding box by more than 1e-3 cell.  -> dict(pose: capi.RegisterPose; converged; history: per iteration
    dict(used, inside, rms = sqrt(ee / used), center, gate, delta: the step or None when it was refused, terms: the record)).
    Deterministic: the same inputs give the same bytes."""
    mask = _REGISTER_DOF[dof] if isinstance(dof, str) else int(dof)
    inf = float("inf")
    cells = capi.disparity_mesh(reference, 1, inf if max_jump is None else max_jump)[1]
    pose = capi.RegisterPose()
    ctypes.memmove(ctypes.byref(pose), ctypes.byref(capi.RegisterPose.make() if initial is None else initial), ctypes.sizeof(capi.RegisterPose))
    pts = points.reshape(-1, 3)
    kept = torch.isfinite(pts).all(1) & ~(pts == 0).all(1)       # the points the skip rule keeps
    posed = capi.transform_points(points, pose)
    has = (capi.dsm_difference(posed, reference, frame, cells).view(torch.int32) != capi.STEREO_INVALID_BITS) & kept
    # masked reductions, no compaction: one read-back of the pivot's sums, the two counts and the box
    inf32 = torch.tensor(inf, dtype=torch.float32, device=pts.device)
    head = torch.cat([torch.where(has[:, None], posed.reshape(-1, 3), torch.zeros_like(inf32)).double().sum(0),
                      torch.stack([has.sum(), kept.sum()]).double(),
                      torch.where(kept[:, None], pts, inf32).min(0).values.double() if pts.shape[0] else torch.zeros(3, dtype=torch.float64, device=pts.device),
                      torch.where(kept[:, None], pts, -inf32).max(0).values.double() if pts.shape[0] else torch.zeros(3, dtype=torch.float64, device=pts.device)]).cpu().numpy()
    count = int(head[3])
    pivot = head[:3] / count if count else np.zeros(3)
    pose.pivot[:] = [float(np.float32(x)) for x in pivot]
    if int(head[4]):
        lo, hi = head[5:8], head[8:11]
        corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    else:
        corners = np.zeros((0, 3))
    history, converged, ws = [], False, None
    for _ in range(int(iterations)):
        center, width = 0.0, inf
        if gate is not None:
            diff = capi.dsm_difference(capi.transform_points(points, pose, out=posed), reference, frame, cells)
            signed = capi.difference_stats(diff, quantiles=(5000,))
            if signed.finite == 0:
                break
            center = float(signed.quantile[0])
            mad = capi.difference_stats(diff, center=center, absolute=True, quantiles=(5000,)).quantile[0]
            width = float(np.float32(np.float64(gate) * (np.float64(1.4826) * np.float64(mad))))
        if ws is None:
            ws = capi.dev_bytes(int(capi.LIB.ssrlcv_hip_register_terms_workspace_bytes(capi.c_u32(pts.shape[0]))))
        terms = capi.register_terms(points, pose, reference, frame, cells, center, width, ws)
        delta = capi.register_step(terms, mask, damping)
        used = int(terms.used)
        history.append({"used": used, "inside": int(terms.inside), "rms": float(np.sqrt(np.float64(terms.ee) / used)) if used else float("nan"),
                        "center": center, "gate": width, "delta": None if delta is None else delta.tolist(), "terms": terms})
        if delta is None:
            break
        nxt = capi.register_compose(pose, delta)
        (m0, t0), (m1, t1) = _pose64(pose), _pose64(nxt)
        step = (corners @ m1.T + t1) - (corners @ m0.T + t0)
        pose = nxt
        if len(corners) == 0 or float(np.sqrt((step ** 2).sum(1)).max()) <= 1e-3 * float(frame.cell):
            converged = True
            break
    return {"pose": pose, "converged": converged, "history": history}


def _shift_gate(moving, reference, g, center, gate, scale):
    """(centerQ, gateQ) of one level of surface_shift_search: the median and gate x NMAD of the differences of the two sampled
    maps at the shift `center`, in quanta; no gate where that shift has no finite difference"""
    m, r = moving[::g, ::g], reference[::g, ::g]
    h, w = m.shape
    (x0, x1), (y0, y1) = ((max(0, -s), min(n, n - s)) for s, n in zip(center, (w, h)))
    if x1 <= x0 or y1 <= y0:
        return 0, None
    diff = capi.dsm_subtract(m[y0:y1, x0:x1].contiguous(), r[y0 + center[1]:y1 + center[1], x0 + center[0]:x1 + center[0]].contiguous())
    signed = capi.difference_stats(diff, quantiles=(5000,))
    if signed.finite == 0:
        return 0, None
    median = float(signed.quantile[0])
    mad = float(capi.difference_stats(diff, center=median, absolute=True, quantiles=(5000,)).quantile[0])
    center_q = int(np.rint(np.float64(median) * np.float64(scale)))
    gate_q = int(np.floor(np.float64(gate) * (np.float64(1.4826) * np.float64(mad)) * np.float64(scale)))
    return max(-(1 << 18), min(1 << 18, center_q)), max(0, min(gate_q, capi.SHIFT_NO_GATE - 1))


def surface_shift_search(subject, reference, frame, radius=8, strides=(4, 1), gate=3.0, scale=None, min_overlap=0.25, rule="max", initial=None):
    """The whole-cell shift that lays a subject tens of cells off onto a reference height map (float32 (h, w) device tensor in
    `frame`), coarse to fine (include/ssrlcv_hip.h "shift search"): what surface_register needs before its first step.  subject: a
    cloud ((n, 3) float32 device tensor), which goes through transform_cloud(initial) when an initial pose is given and then
    through capi.dsm_rasterize (rule "max" or "min"), or a height map of the grid of `frame`.  scale: quanta a height unit,
    64 / cell by default.  One capi.shift_search a level: the first at strides[0], centred on 0 with `radius`; each later one
    at its stride g centred on the shift found so far, floor(best / g + 0.5), with radius ceil(g_prev / g) + 1.  With a gate
    (None: without) only differences within gate x NMAD of the median take part, both taken from capi.dsm_subtract of the two
    sampled maps at the level's centre shift and two statistics calls.  A shift is a candidate if it has at least min_overlap x
    the level's valid subject cells; the best is the one of least variance of the differences (capi.shift_pick).
    -> dict(shift: (x, y) in cells, the last level's best shift with its sub-cell step; bias: the subject's height above the
    reference; variance; second: the least variance outside the 3 x 3 around the best; pose: a capi.RegisterPose, M = the
    identity (or initial's) and T moved by cell (x ex + y ey) - bias ez, which is exact for the orthonormal frames dsm_frame
    makes; levels: per level dict(params, result, table)).  Raises SsrlcvError when a level has no candidate."""
    if rule not in _DSM_RULES:
        raise ValueError("rule is 'max' or 'min', not %r" % (rule,))
    strides = [int(g) for g in strides]
    if not strides or any(g < 1 for g in strides):
        raise ValueError("strides are at least 1, not %r" % (strides,))
    is_map = subject.dim() == 2 and tuple(subject.shape) == (int(frame.h), int(frame.w))
    if is_map:
        moving = subject
    else:
        cloud = subject if initial is None else transform_cloud(subject, initial)
        moving = capi.dsm_rasterize(cloud, frame, _DSM_RULES[rule], want_source=False, want_count=False)[0]
    cell = float(frame.cell)
    scale = float(np.float32(64.0 / cell if scale is None else scale))
    best, levels, ws = (0, 0), [], None
    for k, g in enumerate(strides):
        center = (0, 0) if k == 0 else tuple(int(np.floor(b / g + 0.5)) for b in best)
        level_radius = int(radius) if k == 0 else -(-strides[k - 1] // g) + 1
        center_q, gate_q = (0, None) if gate is None else _shift_gate(moving, reference, g, center, gate, scale)
        table = capi.shift_search(moving, reference, scale, g, center, level_radius, center_q, gate_q, ws)
        result = capi.shift_pick(table, table["params"], int(float(min_overlap) * int(table["head"]["validMoving"])))
        if result is None:
            raise capi.SsrlcvError("surface_shift_search: no shift of level %d (stride %d) has the overlap asked for" % (k, g))
        best = (int(result.shiftX), int(result.shiftY))
        levels.append({"params": table["params"], "result": result, "table": table})
    x, y = best[0] + float(result.subX), best[1] + float(result.subY)
    start = capi.RegisterPose.make() if initial is None else initial
    m = np.array(list(start.m), np.float64).reshape(3, 4)
    ex, ey, ez = (np.array(list(v), np.float64) for v in (frame.ex, frame.ey, frame.ez))
    pose = capi.RegisterPose.make(m[:, :3], m[:, 3] + cell * (x * ex + y * ey) - float(result.bias) * ez, list(start.pivot))
    return {"shift": (x, y), "bias": float(result.bias), "variance": float(result.variance), "second": float(result.second), "pose": pose,
            "levels": levels}


def surface_register_coarse(points, reference, frame, search, **register):
    """surface_register behind a coarse search, for a cloud that lies many cells off: surface_shift_search(points, reference,
    frame, **search) runs first -- on the cloud under register's `initial`, if there is one -- and its pose is the `initial` of
    the loop.  -> surface_register's dictionary, which gains `search` (surface_shift_search's)."""
    found = surface_shift_search(points, reference, frame, **dict(search, initial=register.get("initial")))
    out = surface_register(points, reference, frame, **dict(register, initial=found["pose"]))
    out["search"] = found
    return out


def surface_accuracy(subject, reference, frame, subject_frame=None, want_map=False, register=None, **kw):
    """How far a surface lies from a reference height map (`reference` in `frame`): `subject` is a cloud ((n, 3) float32 device
    tensor) or a height map (float32 (h, w): any tensor when subject_frame is given, one of the grid of `frame` without), which
    goes through capi.dsm_points of its own frame.  kw is surface_difference's (mesh, max_jump).  Three statistics calls on the differences: the signed ones with
    the median; the absolute ones about the median; the absolute ones with three quantiles.
    -> dict(n; coverage = finite / n; bias: the median; nmad = 1.4826 x the median absolute deviation about it, host float64;
    mean, rms; le68, le90, le95: the 6827 / 9000 / 9500 quantiles of |diff|; min, max; diff: the differences).  With want_map and a
    height-map subject also error_map: the differences scattered back into the subject's grid by its validity mask, a map in
    the form of every map here.  With register = a dict of surface_register's arguments (dof, iterations, gate, initial, damping;
    max_jump is kw's) the subject's points are registered to the reference first and the differences are those of the registered
    points: the report gains pose and registration (surface_register's dictionary).  register may also hold search = a dict of
    surface_shift_search's arguments, for a subject that lies many cells off: the registration is surface_register_coarse's."""
    sub_frame = frame if subject_frame is None else subject_frame
    is_map = subject_frame is not None or (subject.dim() == 2 and tuple(subject.shape) == (int(frame.h), int(frame.w)))
    if want_map and not is_map:
        raise ValueError("want_map needs a height-map subject")
    points = capi.dsm_points(subject, sub_frame)[0] if is_map else subject
    registration = None
    if register is not None:
        if not kw.get("mesh", True):
            raise ValueError("register needs the mesh of the reference (mesh=True)")
        register = dict(register)
        search = register.pop("search", None)
        if search is None:
            registration = surface_register(points, reference, frame, max_jump=kw.get("max_jump"), **register)
        else:
            registration = surface_register_coarse(points, reference, frame, search, max_jump=kw.get("max_jump"), **register)
        points = transform_cloud(points, registration["pose"])
    diff = surface_difference(points, reference, frame, **kw)
    signed = difference_stats(diff, quantiles=(5000,))
    nan = float("nan")
    if signed["finite"]:
        bias = signed["quantiles"][0]
        mad = difference_stats(diff, center=bias, absolute=True, quantiles=(5000,))["quantiles"][0]
        le = difference_stats(diff, absolute=True, quantiles=(6827, 9000, 9500))["quantiles"]
    else:
        bias, mad, le = nan, nan, [nan, nan, nan]
    n = signed["n"]
    out = {"n": n, "coverage": signed["finite"] / n if n else nan, "bias": bias, "nmad": float(np.float64(1.4826) * np.float64(mad)),
           "mean": signed["mean"], "rms": signed["rms"], "le68": le[0], "le90": le[1], "le95": le[2], "min": signed["min"], "max": signed["max"],
           "diff": diff}
    if want_map:
        error_map = torch.full(subject.shape, capi.STEREO_INVALID_BITS, dtype=torch.int32, device=subject.device)
        error_map[subject.view(torch.int32) != capi.STEREO_INVALID_BITS] = diff.view(torch.int32)   # dsm_points numbers the valid cells in raster order
        out["error_map"] = error_map.view(torch.float32)
    if registration is not None:
        out["pose"], out["registration"] = registration["pose"], registration
    return out


def exchange_features(local, num_images):
    world, _ = _world()
    if world == 1:
        return [local[v] for v in range(num_images)]
    return sd.exchange_keyed(local, num_images, sd.image_owner)


def match_pairs(features, cameras, seed_features=None, epsilon=25.0, delta=5.0, rel=0.6, absolute=200.0 * 200.0, mode=1,
                ws=None, owners=None, ratio=None, mutual=False):
    """Exhaustive matching (generateMatchesExhaustive; GEO_ORBIT double-constrained for mode 1, brute force for mode 0)
    of the pairs this rank owns (`owners`: rank per pair index, default dist.assign_pairs).  features: list of uint8 CUDA
    tensors (all images).  Every pair is queued -- match, validation / compaction with the count left on the device --
    and the stream is synchronised once for all the counts.  Returns {pair index: validated uint2_pair bytes}.
    ratio (Lowe's ratio test against the second nearest target, 0 < ratio <= 1) and / or mutual (cross check): every pair
    goes through capi.match_ratio instead -- brute force only (mode 0), no seed image."""
    ws = ws or Workspace()
    if ratio is not None or mutual:
        if seed_features is not None and ratio is not None:
            raise ValueError("match_pairs: the ratio test against the second neighbour replaces the seed-image ratio; pass one of them")
        if seed_features is not None:
            raise ValueError("match_pairs: the mutual check has no seed-image form")
        if mode != 0:
            raise ValueError("match_pairs: ratio / mutual need the brute-force matcher (mode 0), got mode %d" % mode)
        return _match_pairs_ratio(features, 0.0 if ratio is None else float(ratio), bool(mutual), absolute, ws, owners)
    world, rank = _world()
    num_images = len(features)
    pairs = sd.pair_list(num_images)
    if owners is None:
        owners = sd.assign_pairs([f.numel() // FEATURE_BYTES for f in features], world)
    seed_d = ws.seed_features(seed_features)
    mine = [p for p in range(len(pairs)) if owners[p] == rank]
    counts = torch.zeros(max(len(mine), 1), dtype=torch.int32, device="cuda")
    bufs = {}
    seed_cache = {}
    shapes = []
    for p in mine:
        qi, ti = pairs[p]
        nq, nt = features[qi].numel() // FEATURE_BYTES, features[ti].numel() // FEATURE_BYTES
        shapes.append((nq, nt))
        if seed_features is not None:
            shapes.append((nq, len(seed_features)))
    mws = ws.matcher(shapes, 16)[0] if shapes else None
    for k, p in enumerate(mine):
        qi, ti = pairs[p]
        nq, nt = features[qi].numel() // FEATURE_BYTES, features[ti].numel() // FEATURE_BYTES
        sdist = None
        if seed_d is not None:
            if qi not in seed_cache:  # recomputed per query image upstream (src/MatchFactory.cu:925)
                seed_cache[qi] = capi.seed_distances(features[qi], nq, seed_d, len(seed_features), workspace=mws)
            sdist = seed_cache[qi]
        proj = capi.projection_matrix(cameras[ti:ti + 1]) if mode == 1 else None
        params = capi.make_match_params(mode, qi, ti, epsilon, delta, rel, absolute,
                                        cameras[qi:qi + 1] if mode == 1 else None, proj)
        bufs[p] = capi.dev_bytes(nq * 16)
        capi.match(features[qi], nq, features[ti], nt, params, capi.OUT_UINT2_PAIR, seed_d=sdist, workspace=mws, out=bufs[p])
        capi.compact_matches_async(capi.OUT_UINT2_PAIR, bufs[p], nq, mws, counts[k:k + 1])
    n = counts.cpu().tolist()  # the one synchronisation
    return {p: bufs[p][: n[k] * 16] for k, p in enumerate(mine)}


def _match_pairs_ratio(features, ratio, mutual, absolute, ws, owners):
    """match_pairs through the two-nearest matcher: per owned pair match_ratio + compaction on the same workspace, all
    queued, one synchronisation for the counts."""
    world, rank = _world()
    pairs = sd.pair_list(len(features))
    if owners is None:
        owners = sd.assign_pairs([f.numel() // FEATURE_BYTES for f in features], world)
    mine = [p for p in range(len(pairs)) if owners[p] == rank]
    counts = torch.zeros(max(len(mine), 1), dtype=torch.int32, device="cuda")
    shapes = [(features[pairs[p][0]].numel() // FEATURE_BYTES, features[pairs[p][1]].numel() // FEATURE_BYTES) for p in mine]
    need = max([capi.LIB.ssrlcv_hip_match2_workspace_bytes(capi.c_u32(nq), capi.c_u32(nt)) for nq, nt in shapes] or [1])
    if ws.match2_ws is None or ws.match2_ws.numel() < need:
        ws.match2_ws = capi.dev_bytes(need)
    bufs = {}
    for k, p in enumerate(mine):
        qi, ti = pairs[p]
        nq, nt = shapes[k]
        params = capi.make_ratio_params(qi, ti, ratio=ratio, absolute=absolute, mutual=mutual)
        bufs[p] = capi.dev_bytes(nq * 16)
        capi.match_ratio(features[qi], nq, features[ti], nt, params, capi.OUT_UINT2_PAIR, workspace=ws.match2_ws, out=bufs[p])
        capi.compact_matches_async(capi.OUT_UINT2_PAIR, bufs[p], nq, ws.match2_ws, counts[k:k + 1])
    n = counts.cpu().tolist()  # the one synchronisation
    return {p: bufs[p][: n[k] * 16] for k, p in enumerate(mine)}


def two_view_uncalibrated(feat_q, feat_t, ratio=0.8, samples=2048, threshold=1.0, epsilon=2.0, seed=0, absolute=3.0e9):
    """Two views without trusted cameras: ratio + mutual brute-force matches -> 7-point RANSAC for F -> the F-constrained
    matcher (mode 2, band `epsilon` px around the epipolar line) with the F found.  feat_q, feat_t: feature bytes on the
    device.  The putative matches are validated (compacted) before the RANSAC: a sample that draws a flagged entry yields
    no candidate, and two of three entries are flagged.  F comes to the host because mode 2 takes it from there.
    -> dict(F [3, 3] float32, inliers, putative (validated Match bytes), num_putative, matches (validated DMatch bytes),
    count).  No F (fewer than 7 putative matches, or no candidate with an inlier): inliers 0, no matches."""
    nq, nt = feat_q.numel() // FEATURE_BYTES, feat_t.numel() // FEATURE_BYTES
    ws2 = capi.match2_workspace(nq, nt)
    putative = capi.match_ratio(feat_q, nq, feat_t, nt, capi.make_ratio_params(0, 1, ratio=ratio, absolute=absolute, mutual=True),
                                capi.OUT_MATCH, workspace=ws2)
    n_put = capi.compact_matches(capi.OUT_MATCH, putative, nq, ws2)
    putative = putative[: n_put * 40]
    r = capi.fmatrix_ransac(putative, n_put, samples, threshold, seed=seed)
    out = {"F": r["F"], "inliers": r["count"], "putative": putative, "num_putative": n_put,
           "matches": capi.dev_bytes(0)[:0], "count": 0}
    if r["count"] == 0:
        return out
    params = capi.make_match_params(2, 0, 1, epsilon=epsilon, absolute=absolute, fundamental=r["F"])
    mws = capi.match_workspace(nq, nt)
    dm = capi.match(feat_q, nq, feat_t, nt, params, capi.OUT_DMATCH, workspace=mws)
    out["count"] = capi.compact_matches(capi.OUT_DMATCH, dm, nq, mws)
    out["matches"] = dm[: out["count"] * 48]
    return out


def exchange_pairs(local, num_pairs, owners=None):
    world, _ = _world()
    if world == 1:
        return [local[p] for p in range(num_pairs)]
    owner_fn = sd.pair_owner if owners is None else (lambda p, _world_size: owners[p])
    return sd.exchange_keyed(local, num_pairs, owner_fn)


def _pinned_copy(t_d, nbytes, slot):
    """D2H through a pinned staging buffer kept between calls (pageable, 16 MB took 5.6 ms) -> uint8 numpy view of the
    staging buffer (valid until the next call with the same slot)."""
    stages = build_match_set.__dict__.setdefault("_stages", {})
    if slot not in stages or stages[slot].numel() < nbytes:
        stages[slot] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    stage = stages[slot][:nbytes]
    stage.copy_(t_d[:nbytes])
    return stage.numpy()


def _pool_probe():
    """How sys.getrefcount reads for a pooled array nobody else refers to, measured with the very loop _result_buffer runs
    (the pool's list, the loop variable, getrefcount's argument: 3 on CPython 3.10; interpreters that borrow references
    read lower), and checked: one outstanding view must read exactly one more.  None = the count cannot be trusted on this
    interpreter, and the pool is not used (every result gets a fresh array)."""
    pool = [np.empty(16, np.uint8)]
    free = held = None
    for buf in pool:
        free = sys.getrefcount(buf)
    view = pool[0][:8].view(np.uint16)   # what a caller holds: a view whose base is the pooled buffer
    for buf in pool:
        held = sys.getrefcount(buf)
    del view
    for buf in pool:
        again = sys.getrefcount(buf)
    return free if (held == free + 1 and again == free) else None


_POOL_FREE_COUNT = _pool_probe()


def _result_buffer(nbytes, slot):
    """A host byte array for a result the caller will own.  Fresh arrays of this size (12 MB of key points per step of the
    4 x 4096^2 flow) are mmap'ed and page-faulted by every call, and now and then that stalls for 25-30 ms (seen in bench.py's
    N-view leg: one `merge` stage in five).  So the arrays are pooled per slot and handed out again once nobody outside the
    pool refers to them any more: a result array, and every slice or view a caller takes of it, is a view whose base is the
    pooled buffer, so the buffer's reference count tells -- against the free reading calibrated by _pool_probe() on this
    interpreter, not a constant."""
    if _POOL_FREE_COUNT is None:
        return np.empty(max(nbytes, 1 << 16), np.uint8)
    pool = build_match_set.__dict__.setdefault("_results", {}).setdefault(slot, [])
    for buf in pool:
        if buf.size >= nbytes and sys.getrefcount(buf) == _POOL_FREE_COUNT:
            return buf
    buf = np.empty(max(nbytes, 1 << 16), np.uint8)
    if len(pool) >= 4:
        pool.pop(0)
    pool.append(buf)
    return buf


def _host_records(t_d, count, dtype, slot):
    """`count` records of a device byte tensor as a structured numpy array the caller owns.  The copy out of the staging
    buffer is a plain byte copy: `view(dtype).copy()` on a structured dtype went element by element and took 5 of the
    merge stage's 7 ms for 0.7 M key points."""
    nbytes = count * dtype.itemsize
    raw = _result_buffer(nbytes, slot)[:nbytes]
    if count:
        np.copyto(raw, _pinned_copy(t_d, nbytes, slot))
    return raw.view(dtype)


def build_match_set(features, pair_tensors, dev=None):
    """Replicated merge -> (MultiMatch numpy, KeyPoint numpy).  The merge (src/MatchFactory.cu:943-1020) and the KeyPoint
    table (image, location of every member, :1007-1020) are built on the device (csrc/merge.hip, every rank from the same
    all-gathered pairs: deterministic); `dev` (a dict) receives the device copies so that the triangulation does not upload
    them again.  SSRLCV_MERGE_HOST=1 (or more than 32 images) takes the host merge (csrc/host_merge.cpp) instead."""
    num_features = [f.numel() // FEATURE_BYTES for f in features]
    counts = [t.numel() // 16 for t in pair_tensors]
    use_host = bool(os.environ.get("SSRLCV_MERGE_HOST")) or len(features) > 32
    if not use_host:
        live = [t.reshape(-1) for t in pair_tensors if t.numel()]
        pairs_d = torch.cat(live) if live else torch.zeros(16, dtype=torch.uint8, device="cuda")
        try:
            mm_d, mem_d, n_mm, n_mem, rounds, build_match_set._ws = capi.merge_matches_device(
                num_features, counts, pairs_d, getattr(build_match_set, "_ws", None))
        except capi.MalformedPairList:
            use_host = True   # e.g. a query matched twice in one pair: only upstream's host walk defines a result for it
    if use_host:
        mm, mem = sd.merge_matches(num_features, pair_tensors)
        kp = np.zeros(len(mem), KEYPOINT)
        if len(mem):
            mem_d = capi.to_dev(np.ascontiguousarray(mem, np.uint32))
            kp_d = capi.keypoints_from_members(mem_d, len(mem), features)
            kp = _host_records(kp_d, len(mem), KEYPOINT, "kp")   # padding bytes are zeros (k_keypoints_from_members)
            if dev is not None:
                dev["keypoints"] = kp_d
        return mm, kp
    mm = np.zeros(0, MULTIMATCH)
    kp = np.zeros(0, KEYPOINT)
    if n_mem:
        kp_d = capi.keypoints_from_members(mem_d, n_mem, features)
        mm = _host_records(mm_d, n_mm, MULTIMATCH, "mm")
        kp = _host_records(kp_d, n_mem, KEYPOINT, "kp")   # padding bytes are zeros (k_keypoints_from_members)
        if dev is not None:
            dev["keypoints"] = kp_d
            dev["matches"] = mm_d
    return mm, kp


def triangulate(mm, kp, cameras, nview, pushbroom=None, dev=None):
    """Bundle-range partitioned triangulation; every rank ends with the full cloud.  `pushbroom`: PushbroomCamera array
    (config[4]): bundles then come from generatePushbroomBundle (src/PointCloudFactory.cu:875-903).  `dev`: device copies
    left by build_match_set."""
    world, rank = _world()
    lo, hi = sd.bundle_range(len(mm), world, rank)
    n = hi - lo
    pts = torch.zeros(0, dtype=torch.float32, device="cuda")
    if n:
        kp_d = dev["keypoints"] if dev and "keypoints" in dev else capi.to_dev(kp)
        sub_d = dev["matches"][8 * lo: 8 * hi] if dev and "matches" in dev else capi.to_dev(mm[lo:hi].copy())
        if pushbroom is not None:
            b_d, l_d = capi.generate_pushbroom_bundles(sub_d, kp_d, n, capi.to_dev(pushbroom),
                                                       len(pushbroom), len(kp))
        else:
            b_d, l_d = capi.generate_bundles(sub_d, kp_d, n, capi.to_dev(cameras), len(cameras), len(kp))
        pts, _, _ = capi.triangulate(l_d, b_d, n, nview=nview)
    if world == 1:
        return pts.view(-1, 3)
    parts = sd.all_gather_bytes(pts.view(torch.uint8).reshape(-1).contiguous())
    return torch.cat([p.view(torch.float32) for p in parts]).view(-1, 3)


def filter_match_set(mm_d, kp_d, n, n_kp, cameras, kind, cutoff=None, sigma=3.0, sample_size=0.1, pushbroom=None):
    """PointCloudFactory::linearCutoffFilter (kind "linear", src/PointCloudFactory.cu:3500-3644) or
    deterministicStatisticalFilter (kind "statistical", :3070-3275) on a MatchSet that lives on the device (MultiMatch /
    KeyPoint byte tensors): bundles, the error triangulation, the statistical cutoff, the cutoff triangulation and the
    rebuild of the MatchSet are queued back to back, the two counts come back in one small copy.
    -> (mm_d, kp_d, n, n_kp) after the filter (the inputs themselves when upstream would leave the MatchSet alone)."""
    if n == 0:
        return mm_d, kp_d, n, n_kp
    nview = len(cameras if pushbroom is None else pushbroom) > 2
    if pushbroom is not None:
        b_d, l_d = capi.generate_pushbroom_bundles(mm_d, kp_d, n, capi.to_dev(pushbroom), len(pushbroom), n_kp)
    else:
        b_d, l_d = capi.generate_bundles(mm_d, kp_d, n, capi.to_dev(cameras), len(cameras), n_kp)
    if kind == "linear":
        if cutoff < 0.0:
            return mm_d, kp_d, n, n_kp
        capi.triangulate(l_d, b_d, n, nview=nview, want_errors=True, cutoff=float(cutoff))
        only_if_bad = True
    else:
        if sample_size > 1.0 or sample_size < 0.0:
            return mm_d, kp_d, n, n_kp
        _, err_d, _ = capi.triangulate(l_d, b_d, n, nview=nview, want_errors=True, cutoff=0.0)
        cut_d = capi.error_sample_cutoff(err_d, n, int(1 / sample_size), sigma)
        capi.triangulate(l_d, b_d, n, nview=nview, want_errors=True, cutoff=cut_d)
        only_if_bad = nview
    mm_o, kp_o, counts = capi.filter_matchset(b_d, kp_d, n, n_kp)
    kept, kept_kp, _ = [int(x) for x in counts.cpu().tolist()]
    if (only_if_bad and kept == n) or kept == 0 or (nview and kept_kp == 0):
        return mm_d, kp_d, n, n_kp   # nothing to remove, or "filtering is too aggressive": the MatchSet stays as it is
    return mm_o[: 8 * kept], kp_o[: 16 * kept_kp], kept, kept_kp


def filter_cloud(points, k=16, sigma=2.0, normals=None, cell_size=0.0):
    """Statistical neighbour-distance outlier removal on a cloud (MeshFactory's neighbour filter; contract in
    include/ssrlcv_hip.h): m_i = mean distance of point i to its k nearest neighbours, kept iff m_i <= mu + sigma * std
    over the finite points.  points: (n, 3) float32 device tensor, e.g. what `reconstruct` / `triangulate` return;
    normals: optional (n, 3) float32 device tensor compacted alongside.  At world size > 1 that cloud is already
    replicated on every rank, so no collective is needed: every rank computes the same result.
    -> dict(points (m, 3), index int64 (m,) original row of each kept point, in input order, mean_distance (n,),
    stats (mu, std, t) floats, count m, normals (m, 3) or None).  One synchronisation (the count)."""
    nbr, d2, _ = capi.knn(points, k, cell_size)
    out = capi.neighbor_distance_filter(points, d2, k, sigma, normals)
    m = int(out["count"].item())
    return {"points": out["points"][:m], "index": out["index"][:m].long(), "mean_distance": out["mean"],
            "stats": tuple(float(x) for x in out["stats"].cpu().tolist()), "count": m,
            "normals": out["normals"][:m] if normals is not None else None}


def cloud_normals(points, k=16, *, viewpoint, cell_size=0.0):
    """Oriented unit normals of a cloud (MeshFactory's normal estimation; contract in include/ssrlcv_hip.h): smallest
    eigenvector of the float64 covariance of each point and its k nearest neighbours, pointing towards `viewpoint`
    (e.g. the mean camera position, in the cloud's frame).  points: (n, 3) float32 device tensor; the same on every rank
    at world size > 1 (the cloud is replicated).  -> (n, 3) float32 device tensor; (0, 0, 0) for non-finite points and
    coincident neighbourhoods.  Stream-ordered."""
    nbr, _, _ = capi.knn(points, k, cell_size, dist2=False)
    return capi.point_normals(points, nbr, k, viewpoint)


def ba_parameter_sets(cameras2, h_lin=1e-5, h_step=(1e-4, 1e-4, 1e-4, 1e-5, 1e-5, 1e-5)):
    """The K = 612 camera-parameter vectors one BundleAdjustTwoView iteration evaluates: 24 for the central-difference
    gradient (h = 1e-5, src/PointCloudFactory.cu:1061-1062) and 588 for the Hessian (h = {1e-4 x3, 1e-5 x3} per camera,
    :1261): 12 x 5 points of the diagonal stencil (:1375-1376) and 132 ordered parameter pairs x 4 points of the cross
    stencil (:1444-1445).  Layout per set: camera-major {pos.xyz, rot.xyz}.  (The exact evaluation order and the float
    drift of upstream's in-place perturbation live in the C++ mirror, host/PointCloudFactory.hpp; this builds the same
    612-point workload for the sharded sweep.)"""
    base = np.concatenate([np.concatenate([c["cam_pos"], c["cam_rot"]]) for c in cameras2]).astype(np.float32)
    hs = np.array(list(h_step) * 2, np.float32)
    sets = []
    for i in range(12):
        for s in (+1, -1):
            p = base.copy()
            p[i] += s * np.float32(h_lin)
            sets.append(p)
    for i in range(12):
        for m in (-2, -1, 0, 1, 2):
            p = base.copy()
            p[i] += m * hs[i]
            sets.append(p)
    for i in range(12):
        for j in range(12):
            if i == j:
                continue
            for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                p = base.copy()
                p[i] += si * hs[i]
                p[j] += sj * hs[j]
                sets.append(p)
    assert len(sets) == 612
    return np.stack(sets)


def _ba_subset_device(dev, n_mm, pair, world, rank):
    """The 2-view bundles of `pair` out of the device copy of the MatchSet as a 2-camera MatchSet on the device
    (ssrlcv_hip_select_pair_bundles: one library pass, the count is the only thing that comes back), and this rank's share
    of them: the MultiMatch entries index the shared KeyPoint array, so a share is a slice of the MultiMatch array.
    -> (MultiMatch bytes of the share, KeyPoint bytes, bundles of this rank, bundles of the pair)"""
    n_kp = dev["keypoints"].numel() // 16
    sub_mm, sub_kp, count = capi.select_pair_bundles(dev["matches"], dev["keypoints"], n_mm, n_kp, pair[0], pair[1])
    total = int(count.item())
    lo, hi = sd.bundle_range(total, world, rank)
    return sub_mm[8 * lo: 8 * hi], sub_kp, hi - lo, total


def ba_error_sweep(mm, kp, cameras, pair=(0, 1), params=None, dev=None):
    """f(params_k) = sum of squared skew-line gaps of the 2-view bundles of `pair`, for all K parameter sets: this rank's
    bundle range in one launch (ssrlcv_hip_ba_sweep2), then all-reduce(sum) over the ranks.  Returns a K-vector on the
    device (identical on every rank up to the float all-reduce).  `dev`: the device copies of the MatchSet left by
    build_match_set / apply_filters; with them the pair's bundles are selected on the device."""
    world, rank = _world()
    if dev and "matches" in dev and "keypoints" in dev and len(mm):
        cams2 = cameras[[pair[0], pair[1]]].copy()
        if params is None:
            params = ba_parameter_sets(cams2)
        K = len(params)
        sub_mm_d, sub_kp_d, n, total = _ba_subset_device(dev, len(mm), pair, world, rank)
        sums = torch.zeros(K, dtype=torch.float32, device="cuda")
        if n:
            sums = capi.ba_sweep2(sub_mm_d, sub_kp_d, n, capi.to_dev(cams2), 2,
                                  torch.from_numpy(np.ascontiguousarray(params, np.float32)).cuda(), K)
        if world > 1:
            sd.all_reduce_sum(sums)
        return sums, total
    two = np.nonzero(mm["numKeyPoints"] == 2)[0]
    if len(two):
        first = kp["parentId"][mm["index"][two]]
        second = kp["parentId"][mm["index"][two] + 1]
        two = two[(first == pair[0]) & (second == pair[1])]
    cams2 = cameras[[pair[0], pair[1]]].copy()
    if params is None:
        params = ba_parameter_sets(cams2)
    K = len(params)
    lo, hi = sd.bundle_range(len(two), world, rank)
    sums = torch.zeros(K, dtype=torch.float32, device="cuda")
    if hi > lo:
        idx = mm["index"][two[lo:hi]]
        sub_kp = np.zeros(2 * (hi - lo), KEYPOINT)
        sub_kp["parentId"][0::2], sub_kp["parentId"][1::2] = 0, 1
        sub_kp["loc"][0::2], sub_kp["loc"][1::2] = kp["loc"][idx], kp["loc"][idx + 1]
        sub_mm = np.zeros(hi - lo, MULTIMATCH)
        sub_mm["numKeyPoints"], sub_mm["index"] = 2, 2 * np.arange(hi - lo)
        sums = capi.ba_sweep2(capi.to_dev(sub_mm), capi.to_dev(sub_kp), hi - lo, capi.to_dev(cams2), 2,
                              torch.from_numpy(np.ascontiguousarray(params, np.float32)).cuda(), K)
    if world > 1:
        sd.all_reduce_sum(sums)
    return sums, len(two)


REFERENCE_FILTERS = "reference"   # doFiltering's own sequence (src/Pipeline.cu:305-340)


def apply_filters(mm, kp, dev, cameras, filters, pushbroom=None):
    """The filtering stage on the device copies of the MatchSet (dev["matches"], dev["keypoints"]; uploaded if the merge ran
    on the host).  filters: REFERENCE_FILTERS = what doFiltering runs -- the 100 km linear cutoff then the 3 sigma / 10 %
    statistical filter for two views, the statistical filter alone otherwise -- or a list of ("linear", cutoff) /
    ("statistical", sigma, sample_size) steps.  Every rank filters the same replicated MatchSet (deterministic).
    -> (MultiMatch numpy, KeyPoint numpy) after the filters; dev holds the filtered device copies."""
    views = len(cameras if pushbroom is None else pushbroom)
    if filters == REFERENCE_FILTERS:
        filters = ([("linear", 100.0)] if views == 2 else []) + [("statistical", 3.0, 0.1)]
    n, n_kp = len(mm), len(kp)
    if n == 0 or not filters:
        return mm, kp
    mm_d = dev["matches"] if "matches" in dev else capi.to_dev(mm)
    kp_d = dev["keypoints"] if "keypoints" in dev else capi.to_dev(kp)
    changed = False
    for f in filters:
        if f[0] == "linear":
            out = filter_match_set(mm_d, kp_d, n, n_kp, cameras, "linear", cutoff=f[1], pushbroom=pushbroom)
        else:
            out = filter_match_set(mm_d, kp_d, n, n_kp, cameras, "statistical", sigma=f[1], sample_size=f[2], pushbroom=pushbroom)
        changed = changed or out[2] != n
        mm_d, kp_d, n, n_kp = out
    dev["matches"], dev["keypoints"] = mm_d, kp_d
    if changed:
        mm = _host_records(mm_d, n, MULTIMATCH, "mm")
        kp = _host_records(kp_d, n_kp, KEYPOINT, "kp")
    return mm, kp


def reconstruct(pixel_tensors_all, cameras, seed_features=None, epsilon=25.0, delta=5.0, mode=1, ws=None, pushbroom=None,
                ba=False, filters=None):
    """Full flow.  pixel_tensors_all: list of u8 CUDA tensors (only the owner rank's entries are used).  `ws`: a
    Workspace kept by the caller between calls; its `times` dict accumulates the wall time of every stage.
    `filters` (None, REFERENCE_FILTERS or a list, see apply_filters): the filtering stage between the MatchSet and the
    cloud, like doFiltering upstream; the result's matches / keypoints / points are then the filtered ones and
    "matches_unfiltered" says how many multi-matches went in."""
    ws = ws or Workspace()
    world, rank = _world()
    num_images = len(pixel_tensors_all)
    mine = {v: pixel_tensors_all[v] for v in range(num_images) if sd.image_owner(v, world) == rank}
    t = time.perf_counter()
    local = extract_features(mine, ws)
    ws.tick("sift", t)
    t = time.perf_counter()
    feats = exchange_features(local, num_images)
    ws.tick("exchange_features", t)
    t = time.perf_counter()
    owners = sd.assign_pairs([f.numel() // FEATURE_BYTES for f in feats], world)
    pair_local = match_pairs(feats, cameras, seed_features, epsilon, delta, mode=mode, ws=ws, owners=owners)
    ws.tick("match", t)
    t = time.perf_counter()
    pair_all = exchange_pairs(pair_local, len(sd.pair_list(num_images)), owners)
    ws.tick("exchange_pairs", t)
    t = time.perf_counter()
    dev = {}
    mm, kp = build_match_set(feats, pair_all, dev)
    ws.tick("merge", t)
    unfiltered = len(mm)
    if filters:
        t = time.perf_counter()
        mm, kp = apply_filters(mm, kp, dev, cameras, filters, pushbroom)
        ws.tick("filter", t)
    t = time.perf_counter()
    cloud = triangulate(mm, kp, cameras, nview=num_images > 2, pushbroom=pushbroom, dev=dev)
    torch.cuda.synchronize()
    ws.tick("triangulate", t)
    out = {"features": feats, "pairs": pair_all, "matches": mm, "keypoints": kp, "points": cloud, "matches_unfiltered": unfiltered,
           "device": dev}   # device copies of the MatchSet ("matches", "keypoints"), e.g. for further apply_filters steps
    if ba and pushbroom is None:
        t = time.perf_counter()
        out["ba_sums"], out["ba_bundles"] = ba_error_sweep(mm, kp, cameras, dev=dev)
        torch.cuda.synchronize()
        ws.tick("ba_sweep", t)
    return out
