#!/usr/bin/env python
"""Developer tool: the disparity mesh (include/ssrlcv_hip.h "disparity mesh") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the block-matching call and a plain
device copy of the same run are the yardsticks, the spread of identical repeats is the noise.

At size^2 (4096 by default), at step 1 and step 4, max_jump = step.  The map is the chain's: the pair of tools/bench_stereo.py
matched by ssrlcv_hip_stereo_sad_u8 at radius 2, D = 64 from 0, left-right tolerance 1, sub-pixel step, then the speckle filter
(maxDiff 1, maxSpeckleSize 200) and the fill (paths 0xFF, maxGap 32, minHits 5, MIN).  Every buffer is allocated beforehand, one
warm-up and `repeats` timed runs between stream events, medians with min and max.  Four calls a step:
  disparity_mesh   ssrlcv_hip_disparity_mesh: the two maps and the vertex count
  mesh_triangles   ssrlcv_hip_mesh_triangles at full capacity
  mesh_normals     ssrlcv_hip_mesh_normals over ssrlcv_hip_stereo_points of the records
  mesh_select      ssrlcv_hip_mesh_select keeping a random 90 % of the vertices, on a fresh copy of the maps every run (the copy is
                   outside the timed window)
Beside each time the bytes the call must move at least, with N nodes, C cells, V vertices, T triangles, M kept vertices --
  disparity_mesh   4 N read (one disparity a node) + 4 N + C written
  mesh_triangles   4 N + C read + 12 T written
  mesh_normals     4 N + C + 12 V read + 12 V written
  mesh_select      4 M read + 4 N + C read and written
(the tables of the compactions, the old -> new table, the neighbours' re-reads and, at a step above 1, the rest of every cache
line of the map are the calls' own doing and not counted) -- the time of a plain device-to-device copy moving as many bytes in
the same run, and the ratio to the block-matching call.  Last, ssrlcv_amd.pipeline.cloud_normals (exact k-NN, k = 16, and the
covariance normals) on the same cloud, the path mesh_normals replaces for a dense cloud: at step 4, and at step 1 with --knn-all.

usage: bench_mesh.py [repeats] [--size N] [--knn-all] [--out FILE]      (defaults 9, 4096, profiles/mesh_bench.txt)"""
import ctypes
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi, pipeline  # noqa: E402
from bench_stereo import commit, make_pair, take, timed  # noqa: E402

RADIUS, D = 2, 64
MAX_DIFF, MAX_SIZE = 1.0, 200
PATHS, MAX_GAP, MIN_HITS = 0xFF, 32, 5
CAMERA = dict(foc=3000.0, baseline=0.2, doffset=8.0)
KNN_K = 16


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "mesh_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    knn_all = "--knn-all" in args
    if knn_all:
        args.remove("--knn-all")
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_mesh.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    res = dict(tool="bench_mesh", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, radius=RADIUS, numDisparities=D, knn_k=KNN_K)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_mesh %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    # ---- the chain that makes the map: block matching, the speckle filter, the fill
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws
    capi.stereo_filter_speckles(disp, cost, MAX_SIZE, MAX_DIFF)
    disp = capi.stereo_fill_holes(disp, PATHS, MAX_GAP, MIN_HITS, capi.FILL_MIN)[0]
    del cost, left, right
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f)" % (RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"]))

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    def report(key, label, s, nbytes):
        c = copy_of(nbytes)
        s.update(bytes=int(nbytes), copy_ms=c["ms"], over_copy=round(s["ms"] / c["ms"], 2), over_block_matching=round(s["ms"] / sad["ms"], 4))
        res[key] = s
        say("  %-16s %8.4f ms (%.4f .. %.4f); at least %7.1f MB, whose copy takes %.4f ms: %6.2f x the copy, %.4f x block matching" % (
            label, s["ms"], s["min_ms"], s["max_ms"], nbytes / 1e6, c["ms"], s["over_copy"], s["over_block_matching"]))

    for step in (1, 4):
        mp = capi.MeshParams(step, float(step))
        gw, gh = capi.mesh_grid(w, h, step)
        n_nodes, n_cells = gw * gh, (gw - 1) * (gh - 1)
        vi = torch.empty((gh, gw), dtype=torch.int32, device="cuda")
        cells = torch.empty((gh - 1, gw - 1), dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = capi.dev_bytes(int(LIB.ssrlcv_hip_disparity_mesh_workspace_bytes(u32(w), u32(h), ctypes.byref(mp))))
        mesh = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_disparity_mesh(capi.ptr(disp), u32(w), u32(h), ctypes.byref(mp), capi.ptr(vi), capi.ptr(cells),
                                                                              capi.ptr(count), capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
        v = int(count.item())
        records, n = capi.stereo_matches(disp, step)
        assert n == v
        points = capi.stereo_points(records, n, cx=w / 2.0, cy=h / 2.0, **CAMERA)
        del records

        tws = capi.dev_bytes(int(LIB.ssrlcv_hip_mesh_triangles_workspace_bytes(u32(gw), u32(gh))))
        faces = torch.empty((2 * n_cells, 3), dtype=torch.int32, device="cuda")
        tri = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_mesh_triangles(capi.ptr(vi), capi.ptr(cells), u32(gw), u32(gh), capi.ptr(faces), u32(2 * n_cells),
                                                                             capi.ptr(count), capi.ptr(tws), capi.c_sz(tws.numel()), capi.stream_ptr())), repeats))
        t = int(count.item())
        del faces, tws

        normals = torch.zeros((v, 3), dtype=torch.float32, device="cuda")
        nrm = summary(timed(lambda: capi.mesh_normals(points, vi, cells, out=normals), repeats))

        kept = torch.nonzero(torch.rand(v, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.9).view(-1).to(torch.int32)
        m = int(kept.numel())
        sws = capi.dev_bytes(int(LIB.ssrlcv_hip_mesh_select_workspace_bytes(u32(v))))
        vi2, cells2 = torch.empty_like(vi), torch.empty_like(cells)
        times = []
        for r in range(repeats + 1):
            vi2.copy_(vi)
            cells2.copy_(cells)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(LIB.ssrlcv_hip_mesh_select(capi.ptr(vi2), capi.ptr(cells2), u32(gw), u32(gh), u32(v), capi.ptr(kept), u32(m), capi.ptr(sws),
                                                  capi.c_sz(sws.numel()), capi.stream_ptr()))
            e1.record()
            torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1))
        sel = summary(times)
        t2 = int(capi.mesh_triangles(vi2, cells2, capacity=0)[1])
        del vi2, cells2, sws

        say("step %d: %d x %d nodes, %d vertices, %d triangles; select keeps %d vertices and %d triangles" % (step, gw, gh, v, t, m, t2))
        res["step_%d" % step] = dict(nodes=n_nodes, cells=n_cells, vertices=v, triangles=t, kept=m, kept_triangles=t2)
        report("step_%d_disparity_mesh" % step, "disparity_mesh", mesh, 8 * n_nodes + n_cells)
        report("step_%d_mesh_triangles" % step, "mesh_triangles", tri, 4 * n_nodes + n_cells + 12 * t)
        report("step_%d_mesh_normals" % step, "mesh_normals", nrm, 4 * n_nodes + n_cells + 24 * v)
        report("step_%d_mesh_select" % step, "mesh_select", sel, 4 * m + 2 * (4 * n_nodes + n_cells))
        if step == 4 or knn_all:
            knn = summary(timed(lambda: pipeline.cloud_normals(points, k=KNN_K, viewpoint=(0.0, 0.0, 0.0)), min(repeats, 3)))
            knn["over_mesh_normals"] = round(knn["ms"] / nrm["ms"], 1)
            res["step_%d_cloud_normals" % step] = knn
            say("  cloud_normals    %8.4f ms (%.4f .. %.4f): exact k-NN, k = %d, and covariance normals of the same %d points: %.1f x mesh_normals" % (
                knn["ms"], knn["min_ms"], knn["max_ms"], KNN_K, v, knn["over_mesh_normals"]))
        del vi, cells, points, normals, kept, ws

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
