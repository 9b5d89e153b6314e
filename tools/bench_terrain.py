#!/usr/bin/env python
"""Developer tool: the terrain filter (include/ssrlcv_hip.h "terrain filter") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: a plain device copy of the bytes a
call must move at least, measured in the same run, is the yardstick, and the spread of identical repeats is the noise.

Four height maps at size^2 (4096 by default): white noise, a constant map, noise with 5 % holes, and `scene`, the fused map of
the chain as tools/bench_simplify.py builds it (about size^2 cells, holes included).  Every buffer is allocated beforehand, one
warm-up and `repeats` timed runs between stream events, medians with min and max.  Per map:
  ERODE, OPEN    ssrlcv_hip_dsm_morphology at radii 1, 2, 8, 32, 128 and 512, beside a device copy of 8 bytes a cell
  lab            tools/terrain_lab.hip on the same map in a child process: the erosion's direct form (a tile and its halo in LDS, both passes in
                 one launch; shipped for radii 1 to 8) against its running minima (shipped above 8), and whether they are bit-equal
  terrain        ssrlcv_hip_dsm_terrain on terrain_schedule's default 8 levels up to radius 128 (level and terrain written),
                 beside a copy of its 9 bytes a cell
  subtract       ssrlcv_hip_dsm_subtract, beside a copy of its 12 bytes a cell
  surface_terrain  the whole pipeline call: filter, fill, subtract
Every row also as a multiple of the 2.31 ms matching call the README measures every stage against.

usage: bench_terrain.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096, profiles/terrain_bench.txt)"""
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
LAB = os.path.join(ROOT, "tools", "_build", "terrain_lab")
RADII = (1, 2, 8, 32, 128, 512)
MATCH_MS = 2.31


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def scene_map(size):
    """the chain's fused map, as tools/bench_simplify.py builds it"""
    u32, LIB = capi.c_u32, capi.LIB
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
    height = pipeline.surface_model([raster, raster + shift, raster - shift], fr, fuse=dict(min_views=2, max_spread=1.0, rule="median"))["height"]
    return height.contiguous(), fr


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "terrain_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_terrain.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    res = dict(tool="bench_terrain", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, match_ms=MATCH_MS, rows={})
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_terrain %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    scene, scene_frame = scene_map(size)
    gen = torch.Generator("cuda").manual_seed(7)
    noise = torch.rand((size, size), device="cuda", generator=gen)
    holes = noise.clone()
    holes.view(torch.int32)[torch.rand((size, size), device="cuda", generator=gen) < 0.05] = INVALID
    maps = [("noise", noise), ("constant", torch.full((size, size), 1.25, device="cuda")), ("holes", holes), ("scene", scene)]

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    def row_text(name, t, nbytes, c):
        return "  %-16s %8.4f ms (%.4f .. %.4f); its %2d B a cell copy in %.4f ms: %6.2f x the copy, %5.2f x the matching call" % (
            name, t["ms"], t["min_ms"], t["max_ms"], nbytes, c["ms"], t["ms"] / c["ms"], t["ms"] / MATCH_MS)

    for name, height in maps:
        h, w = height.shape
        cells = w * h
        row = dict(w=w, h=h, valid=int((height.view(torch.int32) != INVALID).sum()), morphology=[])
        say("%s: %d x %d cells, %d valid" % (name, w, h, row["valid"]))
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        ws = capi.dev_bytes(int(LIB.ssrlcv_hip_dsm_terrain_workspace_bytes(u32(w), u32(h))))
        c8 = copy_of(8 * cells)
        for op, op_name in ((capi.MORPH_ERODE, "ERODE"), (capi.MORPH_OPEN, "OPEN")):
            for radius in RADII:
                t = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_morphology(capi.ptr(height), capi.ptr(out), u32(w), u32(h), u32(radius), u32(op),
                                                                                   capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
                t.update(op=op_name, radius=radius, copy_ms=c8["ms"], over_copy=round(t["ms"] / c8["ms"], 2), over_match=round(t["ms"] / MATCH_MS, 2))
                row["morphology"].append(t)
                say(row_text("%s r %d" % (op_name, radius), t, 8, c8))
        if os.path.exists(LAB):
            with tempfile.NamedTemporaryFile(suffix=".raw") as f:
                height.cpu().numpy().tofile(f.name)
                lab = subprocess.run([LAB, str(w), str(h), f.name, str(repeats)], capture_output=True, text=True, timeout=600)
            texts = [ln.split(" x ", 1)[-1].split(" ", 1)[-1] for ln in lab.stdout.strip().splitlines()] if lab.returncode == 0 else [
                "failed (%d): %s" % (lab.returncode, (lab.stdout + lab.stderr).strip()[-300:])]
            row["lab"] = texts
            for text in texts:
                say("  lab              %s" % text)
        radii, thresholds = pipeline.terrain_schedule(1.0, 128, 0.3, 0.5, 3.0)
        p = capi.TerrainParams(len(radii), (u32 * 8)(*radii), (capi.c_f32 * 8)(*thresholds))
        terrain = torch.empty((h, w), dtype=torch.float32, device="cuda")
        level = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        t = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_terrain(capi.ptr(height), u32(w), u32(h), ctypes.byref(p), capi.ptr(terrain), capi.ptr(level),
                                                                        capi.c_vp(0), capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
        c9 = copy_of(9 * cells)
        t.update(radii=radii, copy_ms=c9["ms"], over_copy=round(t["ms"] / c9["ms"], 2), over_match=round(t["ms"] / MATCH_MS, 2),
                 flagged=int(((level != 0) & (level != 255)).sum()))
        row["terrain"] = t
        say(row_text("terrain 8 levels", t, 9, c9) + "; %d cells flagged" % t["flagged"])
        t = summary(timed(lambda: capi.dsm_subtract(height, terrain, out=out), repeats))
        c12 = copy_of(12 * cells)
        t.update(copy_ms=c12["ms"], over_copy=round(t["ms"] / c12["ms"], 2), over_match=round(t["ms"] / MATCH_MS, 2))
        row["subtract"] = t
        say(row_text("subtract", t, 12, c12))
        del out, ws, terrain, level
        if name == "scene":
            t = summary(timed(lambda: pipeline.surface_terrain(height, scene_frame, 128, 0.3, 0.5, 3.0), repeats))
            t.update(over_match=round(t["ms"] / MATCH_MS, 2))
            row["surface_terrain"] = t
            say("  surface_terrain  %8.4f ms (%.4f .. %.4f): the filter up to radius 128, the fill and the subtraction, allocations included; %5.2f x the matching call"
                % (t["ms"], t["min_ms"], t["max_ms"], t["over_match"]))
        res["rows"][name] = row

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
