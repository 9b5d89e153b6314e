#!/usr/bin/env python
"""Developer tool: the surface simplification (include/ssrlcv_hip.h "surface simplification") on the library ssrlcv_amd/_lib.py
loads (release by default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: a plain device copy and
the grid mesh's own calls in the same run are the yardsticks, the spread of identical repeats is the noise.

Four height maps: `scene`, the fused map of the chain -- the pair of tools/bench_stereo.py matched by ssrlcv_hip_stereo_sad_u8,
its cloud and two copies shifted by +-0.01 rasterised at one point a cell and fused as tools/bench_dsm.py does (about size^2
cells, holes included) -- and a plane, white noise and a smooth relief with 5 % holes at size^2 (4096 by default).  Every buffer
is allocated beforehand, one warm-up and `repeats` timed runs between stream events, medians with min and max.  Per map:
  errors       ssrlcv_hip_dsm_simplify_errors, beside a device copy of its 8 bytes a node (4 read, 4 written)
  lab          tools/simplify_lab.hip on the same map in a child process: its fused form (the two finest levels of a tile in LDS)
               against the shipped error pass, one launch a half-level, and whether the two maps are bit-equal
  grid mesh    ssrlcv_hip_disparity_mesh + ssrlcv_hip_mesh_triangles of the map at step 1: what the extraction is compared with
  extraction   ssrlcv_hip_dsm_simplify_mesh at full capacity at three tolerances: -1 (every triangle), and the smallest ones found
               by bisection that leave at most 10 % and 1 % of them; vertices, triangles, the largest vertical distance of a covered
               node from its triangle's plane (float64, measured here with torch) and the header's bound 2L (tol + 2^-22 max|h|)

usage: bench_simplify.py [repeats] [--size N] [--out FILE]      (defaults 9, 4096, profiles/simplify_bench.txt)"""
import ctypes
import datetime
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssrlcv_amd import _lib, capi, pipeline  # noqa: E402
from bench_stereo import commit, make_pair, take, timed  # noqa: E402

RADIUS, D = 2, 64
CAMERA = dict(foc=3000.0, baseline=0.2, doffset=8.0)
UP = (0.0, 0.0, -1.0)
INVALID = capi.STEREO_INVALID_BITS
LAB = os.path.join(ROOT, "tools", "_build", "simplify_lab")


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def levels(w, h):
    m, L = max(w - 1, h - 1, 1), 0
    while (1 << L) < m:
        L += 1
    return L


def max_deviation(height, corners, budget=1 << 24):
    """the largest |h(n) - plane(n)| over the nodes n the triangles cover, float64.  height: float32 (h, w) tensor; corners: int64
    (T, 3, 2) tensor of (x, y).  Triangles are taken by the side of their bounding box, `budget` box nodes at a time; a leaf
    (side 1) covers its corners alone and is skipped."""
    h, w = height.shape
    side = (corners.amax(1) - corners.amin(1)).amax(1)
    worst = 0.0
    z = height.to(torch.float64)
    for s in torch.unique(side).tolist():
        if s <= 1:
            continue
        tris = corners[side == s]
        oy, ox = torch.meshgrid(torch.arange(s + 1, device=height.device), torch.arange(s + 1, device=height.device), indexing="ij")
        step = max(1, budget // ((s + 1) * (s + 1)))
        for at in range(0, tris.shape[0], step):
            t = tris[at:at + step]
            lo = t.amin(1)
            px, py = lo[:, 0, None, None] + ox, lo[:, 1, None, None] + oy
            (x0, y0), (x1, y1), (x2, y2) = ((t[:, k, 0, None, None], t[:, k, 1, None, None]) for k in range(3))
            det = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            l1 = ((px - x0) * (y2 - y0) - (py - y0) * (x2 - x0)) * det.sign()
            l2 = ((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)) * det.sign()
            l0 = det.abs() - l1 - l2
            inside = (l0 >= 0) & (l1 >= 0) & (l2 >= 0) & (px < w) & (py < h)
            zc = [z[t[:, k, 1], t[:, k, 0]][:, None, None] for k in range(3)]
            plane = (l0 * zc[0] + l1 * zc[1] + l2 * zc[2]) / det.abs()
            dev = (z[py.clamp(max=h - 1), px.clamp(max=w - 1)] - plane).abs()
            dev = torch.where(inside, dev, torch.zeros_like(dev))
            worst = max(worst, float(torch.nan_to_num(dev, nan=float("inf")).max()))
    return worst


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "simplify_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_simplify.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    res = dict(tool="bench_simplify", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, rows={})
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_simplify %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    # ---- the maps
    left, right, _ = make_pair(size)
    disp = torch.empty((size, size), dtype=torch.float32, device="cuda")
    cost = torch.empty((size, size), dtype=torch.int32, device="cuda")
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(size, size, p)
    capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(size), u32(size), ctypes.byref(p), capi.ptr(sad_ws),
                                            capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost), capi.stream_ptr()))
    records, n = capi.stereo_matches(disp, 1)
    raster = capi.stereo_points(records, n, cx=size / 2.0, cy=size / 2.0, **CAMERA)
    del sad_ws, cost, left, right, records, disp
    box = pipeline.dsm_frame(raster, UP, 1.0, ex=(1, 0, 0))
    fr = pipeline.dsm_frame(raster, UP, float(np.sqrt(float(box.w) * float(box.h) / n)), ex=(1, 0, 0))
    shift = torch.tensor([0.0, 0.0, 0.01], device="cuda")
    scene = pipeline.surface_model([raster, raster + shift, raster - shift], fr, fuse=dict(min_views=2, max_spread=1.0, rule="median"))["height"]
    del raster
    gen = torch.Generator("cuda").manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(size, device="cuda", dtype=torch.float32), torch.arange(size, device="cuda", dtype=torch.float32), indexing="ij")
    relief = 20.0 * torch.sin(xx * 0.01) * torch.cos(yy * 0.013) + 2.0 * torch.sin(xx * 0.11 + yy * 0.07)
    holes = relief.clone()
    holes.view(torch.int32)[torch.rand((size, size), device="cuda", generator=gen) < 0.05] = INVALID
    maps = [("scene", scene.contiguous()), ("plane", (0.5 * xx - 0.25 * yy).contiguous()),
            ("noise", torch.rand((size, size), device="cuda", generator=gen)), ("holes", holes)]
    del xx, yy, relief

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    for name, height in maps:
        h, w = height.shape
        nodes, L = w * h, levels(w, h)
        row = dict(w=w, h=h, L=L, valid=int((height.view(torch.int32) != INVALID).sum()))
        say("%s: %d x %d nodes, %d valid, L = %d" % (name, w, h, row["valid"], L))
        err = torch.empty((h, w), dtype=torch.float32, device="cuda")
        e = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_simplify_errors(capi.ptr(height), u32(w), u32(h), capi.ptr(err), capi.stream_ptr())), repeats))
        c = copy_of(8 * nodes)
        e.update(copy_ms=c["ms"], over_copy=round(e["ms"] / c["ms"], 2))
        row["errors"] = e
        say("  errors           %8.4f ms (%.4f .. %.4f); its 8 B a node are %6.1f MB, whose copy takes %.4f ms: %5.2f x the copy" % (
            e["ms"], e["min_ms"], e["max_ms"], 8 * nodes / 1e6, c["ms"], e["over_copy"]))
        if os.path.exists(LAB):
            with tempfile.NamedTemporaryFile(suffix=".raw") as f:
                height.cpu().numpy().tofile(f.name)
                lab = subprocess.run([LAB, str(w), str(h), f.name, str(repeats)], capture_output=True, text=True, timeout=600)
            text = lab.stdout.strip().split(": ", 1)[-1] if lab.returncode == 0 else "failed (%d): %s" % (lab.returncode, lab.stderr.strip()[-200:])
            row["lab"] = text
            say("  lab              %s" % text)
        # the grid mesh of the same map
        mp = capi.MeshParams(1, float("inf"))
        vi = torch.empty((h, w), dtype=torch.int32, device="cuda")
        cells = torch.empty((h - 1, w - 1), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        cap = 2 * (w - 1) * (h - 1)
        faces = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
        ws = capi.dev_bytes(max(int(LIB.ssrlcv_hip_disparity_mesh_workspace_bytes(u32(w), u32(h), ctypes.byref(mp))),
                                int(LIB.ssrlcv_hip_mesh_triangles_workspace_bytes(u32(w), u32(h))),
                                int(LIB.ssrlcv_hip_dsm_simplify_mesh_workspace_bytes(u32(w), u32(h)))))

        def grid_mesh():
            capi.check(LIB.ssrlcv_hip_disparity_mesh(capi.ptr(height), u32(w), u32(h), ctypes.byref(mp), capi.ptr(vi), capi.ptr(cells), capi.ptr(counts),
                                                     capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr()))
            capi.check(LIB.ssrlcv_hip_mesh_triangles(capi.ptr(vi), capi.ptr(cells), u32(w), u32(h), capi.ptr(faces), u32(cap), capi.ptr(counts),
                                                     capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr()))
        g = summary(timed(grid_mesh, repeats))
        g["triangles"] = int(counts[0].item())
        row["grid_mesh"] = g
        say("  grid mesh        %8.4f ms (%.4f .. %.4f): disparity_mesh + mesh_triangles, %d triangles" % (g["ms"], g["min_ms"], g["max_ms"], g["triangles"]))
        kept = torch.empty(nodes, dtype=torch.int32, device="cuda")

        def extract(tol, capacity=cap, kept_capacity=nodes):
            capi.check(LIB.ssrlcv_hip_dsm_simplify_mesh(capi.ptr(height), capi.ptr(err), u32(w), u32(h), capi.c_f32(tol), capi.c_vp(0), capi.ptr(vi),
                                                        capi.ptr(faces) if capacity else capi.c_vp(0), u32(capacity), capi.c_vp(counts.data_ptr()),
                                                        capi.ptr(kept) if kept_capacity else capi.c_vp(0), u32(kept_capacity),
                                                        capi.c_vp(counts.data_ptr() + 4), capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr()))

        def count_at(tol):
            extract(tol, 0, 0)
            return int(counts[0].item())
        full = count_at(-1.0)
        finite = err[torch.isfinite(err)]
        top = float(finite.max()) if finite.numel() else 0.0
        hmax = float(torch.nan_to_num(height[height.view(torch.int32) != INVALID].abs(), nan=0.0, posinf=0.0).max()) if row["valid"] else 0.0
        row["extraction"] = []
        for share in (1.0, 0.1, 0.01):
            tol = -1.0
            if share < 1.0:
                lo, hi = 0.0, top
                for _ in range(40):  # the smallest float32 tolerance that leaves at most `share` of the triangles
                    mid = float(np.float32(0.5 * (lo + hi)))
                    if mid in (lo, hi):
                        break
                    lo, hi = (lo, mid) if count_at(mid) <= share * full else (mid, hi)
                tol = hi if count_at(lo) > share * full else lo
            x = summary(timed(lambda: extract(tol), repeats))
            t, v = (int(k) for k in counts.cpu().tolist())
            corner = kept[:v].to(torch.int64)[faces[:t].to(torch.int64)]
            dev = max_deviation(height, torch.stack([corner % w, corner // w], 2)) if t else 0.0
            x.update(tolerance=tol, triangles=t, vertices=v, share=round(t / max(full, 1), 4), over_grid_mesh=round(x["ms"] / g["ms"], 2),
                     deviation=dev, bound=2 * L * (max(tol, 0.0) + 2.0 ** -22 * hmax))
            row["extraction"].append(x)
            say("  extraction %5.1f %% %8.4f ms (%.4f .. %.4f): %5.2f x the grid mesh; tolerance %.6g leaves %d vertices and %d triangles (%.2f %%); "
                "largest deviation %.6g, bound %.6g" % (100 * share, x["ms"], x["min_ms"], x["max_ms"], x["over_grid_mesh"], tol, v, t, 100.0 * t / max(full, 1),
                                                        dev, x["bound"]))
        res["rows"][name] = row
        del err, vi, cells, faces, kept, ws

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
