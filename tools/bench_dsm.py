#!/usr/bin/env python
"""Developer tool: the surface model (include/ssrlcv_hip.h "surface model") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the block-matching call and a plain
device copy of the same run are the yardsticks, the spread of identical repeats is the noise.

The cloud is the dense cloud of a size^2 pair (4096 by default: 16.7 M points in the raster order of the image), the pair of
tools/bench_stereo.py matched by ssrlcv_hip_stereo_sad_u8 at radius 2, D = 64, through ssrlcv_hip_stereo_matches and
ssrlcv_hip_stereo_points; and the same points shuffled, the unorganised case.  Every buffer is allocated beforehand, one warm-up
and `repeats` timed runs between stream events, medians with min and max.
  dsm_rasterize   at cells of about 1, 16 and 256 points and on the one-cell grid, with source and count and without count
  dsm_fuse        m = 3 and 8 maps of size^2
  dsm_points      a size^2 map
  surface         pipeline.surface_model + surface_mesh of three clouds (the raster cloud and two shifted copies)
Beside each time the bytes the call must move at least -- rasterize: 12 B a point read, 8 B a cell cleared, 8 B a cell read, and
the maps written; fuse: 4 m + 5 B a cell; points: 4 B a cell and 12 B a vertex -- the time of a plain device-to-device copy moving
as many bytes in the same run, and the ratio to the block-matching call.

--form NAME labels the run (the A/B of the scatter kernel's forms: a library built aside with -DSSRLCV_DSM_SCATTER=1 or 2 and
loaded through SSRLCV_HIP_LIB); --scatter-only stops behind the rasterize rows; --append adds to the file instead of replacing it.

usage: bench_dsm.py [repeats] [--size N] [--form NAME] [--scatter-only] [--append] [--out FILE]   (defaults 9, 4096, profiles/dsm_bench.txt)"""
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
CAMERA = dict(foc=3000.0, baseline=0.2, doffset=8.0)
UP = (0.0, 0.0, -1.0)   # the camera looks along +Z: heights grow towards it; with ex = X, (ex, ey, -ez) = (X, Y, Z) is right-handed


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "dsm_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    form = take(args, "--form", "shipped", str)
    scatter_only, append = "--scatter-only" in args, "--append" in args
    args = [a for a in args if a not in ("--scatter-only", "--append")]
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_dsm.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    res = dict(tool="bench_dsm", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(), form=form,
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, radius=RADIUS, numDisparities=D)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_dsm %s commit %s library %s (scatter form: %s) on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], form, res["device"], size, repeats))

    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws, cost, left, right
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f)" % (RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"]))
    records, n = capi.stereo_matches(disp, 1)
    raster = capi.stereo_points(records, n, cx=w / 2.0, cy=h / 2.0, **CAMERA)
    del records, disp
    shuffled = raster[torch.randperm(n, device="cuda", generator=torch.Generator("cuda").manual_seed(1))].contiguous()
    box = pipeline.dsm_frame(raster, UP, 1.0, ex=(1, 0, 0))          # cells of 1 world unit: w and h are the extent
    spacing = float(np.sqrt(float(box.w) * float(box.h) / n))
    say("cloud: %d points, extent %d x %d world units, mean spacing %.4f" % (n, box.w, box.h, spacing))

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    def report(key, label, s, nbytes):
        c = copy_of(nbytes)
        s.update(bytes=int(nbytes), copy_ms=c["ms"], over_copy=round(s["ms"] / c["ms"], 2), over_block_matching=round(s["ms"] / sad["ms"], 4))
        res[key] = s
        say("  %-44s %9.4f ms (%.4f .. %.4f); at least %7.1f MB, whose copy takes %.4f ms: %7.2f x the copy, %.4f x block matching" % (
            label, s["ms"], s["min_ms"], s["max_ms"], nbytes / 1e6, c["ms"], s["over_copy"], s["over_block_matching"]))

    grids = [("%d/cell" % k, pipeline.dsm_frame(raster, UP, spacing * np.sqrt(k), ex=(1, 0, 0))) for k in (1, 16, 256)]
    grids.append(("one cell", pipeline.dsm_frame(raster, UP, float(max(box.w, box.h)) + 1.0, ex=(1, 0, 0))))
    for label, fr in grids:
        cells = int(fr.w) * int(fr.h)
        ws = capi.dev_bytes(int(LIB.ssrlcv_hip_dsm_rasterize_workspace_bytes(u32(fr.w), u32(fr.h))))
        height = torch.empty((fr.h, fr.w), dtype=torch.float32, device="cuda")
        source, count = torch.empty((fr.h, fr.w), dtype=torch.int32, device="cuda"), torch.empty((fr.h, fr.w), dtype=torch.int32, device="cuda")
        for cloud_name, cloud in (("raster", raster), ("shuffled", shuffled)):
            for with_count in (True, False):
                s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_rasterize(capi.ptr(cloud), u32(n), ctypes.byref(fr), u32(0), capi.ptr(height),
                                                                                  capi.ptr(source), capi.ptr(count) if with_count else capi.c_vp(0),
                                                                                  capi.ptr(ws), capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
                report("rasterize/%s/%s/%s" % (label, cloud_name, "count" if with_count else "no_count"),
                       "rasterize %s %dx%d %s %s" % (label, fr.w, fr.h, cloud_name, "with count" if with_count else "no count"), s,
                       12 * n + (8 + 8 + 4 + 4 + (4 if with_count else 0)) * cells)
        del ws, height, source, count

    if not scatter_only:
        maps = [torch.randn((h, w), device="cuda", generator=torch.Generator("cuda").manual_seed(k)) for k in range(8)]
        for m in (3, 8):
            out, views = torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.uint8, device="cuda")
            arr = (capi.c_vp * m)(*[x.data_ptr() for x in maps[:m]])
            s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_fuse(arr, u32(m), u32(w), u32(h), u32(2), capi.c_f32(1.0), u32(1), capi.ptr(out),
                                                                         capi.ptr(views), capi.stream_ptr())), repeats))
            report("fuse/m%d" % m, "fuse m = %d, %d^2" % (m, size), s, (4 * m + 5) * w * h)
        fr = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 0.5, w, h)
        s = summary(timed(lambda: capi.dsm_points(maps[0], fr), repeats))
        report("points", "points %d^2 (with the count's synchronisation)" % size, s, 16 * w * h)
        del maps
        fr = grids[1][1]
        clouds = [raster, raster + torch.tensor([0.0, 0.0, 0.01], device="cuda"), raster - torch.tensor([0.0, 0.0, 0.01], device="cuda")]

        def whole():
            model = pipeline.surface_model(clouds, fr, fuse=dict(min_views=2, max_spread=1.0, rule="median"))
            return pipeline.surface_mesh(model, fr, 1.0)
        s = summary(timed(whole, min(repeats, 5)))
        s["over_block_matching"] = round(s["ms"] / sad["ms"], 4)
        res["surface"] = s
        say("  surface_model + surface_mesh, 3 clouds, %dx%d  %9.4f ms (%.4f .. %.4f): %.4f x block matching (host allocations and two "
            "synchronisations included)" % (fr.w, fr.h, s["ms"], s["min_ms"], s["max_ms"], s["over_block_matching"]))

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
