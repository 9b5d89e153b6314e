#!/usr/bin/env python
"""Developer tool: surface accuracy (include/ssrlcv_hip.h "surface accuracy") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the block-matching call and a plain
device copy of the same run are the yardsticks, the spread of identical repeats is the noise.

The reference is the terrain of tools/scene.py's scene at the centres of a size^2 grid (4096 by default); the subject is that
terrain plus noise of a twentieth of a cell with 5 % holes, its valid cells as points through ssrlcv_hip_dsm_points (16 M points in
raster order), and the same points shuffled, the unorganised case.  Every buffer is allocated beforehand, one warm-up and `repeats`
timed runs between stream events, medians with min and max.
  dsm_difference     CELL and MESH mode, on the raster and on the shuffled cloud
  difference_stats   1 and 8 quantiles, on the MESH differences of the scene, on a constant input (every value in one bin of every
                     pass) and on uniformly random bits
Beside each time the bytes the call must move at least -- difference: 12 B a point read, 4 B a point written, the map once (and a
byte a cell in MESH mode); stats: 4 B a value, read once -- the time of a plain device-to-device copy moving as many bytes in the
same run, and the ratio to the block-matching call.

--form NAME labels the run (the A/B of the radix select's digit width: a library built aside with the other
digits and loaded through SSRLCV_HIP_LIB); --stats-only skips the difference rows; --append adds to the file instead of replacing it.

usage: bench_accuracy.py [repeats] [--size N] [--form NAME] [--stats-only] [--append] [--out FILE]   (defaults 9, 4096, profiles/accuracy_bench.txt)"""
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
from ssrlcv_amd import _lib, capi  # noqa: E402
from bench_stereo import commit, make_pair, take, timed  # noqa: E402

RADIUS, D = 2, 64
EIGHT = (0, 10000, 5000, 2500, 7500, 6827, 9000, 9500)


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "accuracy_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    form = take(args, "--form", "shipped", str)
    stats_only, append = "--stats-only" in args, "--append" in args
    args = [a for a in args if a not in ("--stats-only", "--append")]
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_accuracy.py needs a GPU"
    torch.cuda.set_device(0)
    u32, LIB = capi.c_u32, capi.LIB
    w = h = size
    res = dict(tool="bench_accuracy", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(), form=form,
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_accuracy %s commit %s library %s (digits: %s) on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], form, res["device"], size, repeats))

    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws, cost, left, right, disp
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f)" % (RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"]))

    # the scene's terrain over the patch, a cell of one world unit
    import scene
    gsd = scene.PATCH_KM / size
    jj, ii = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    terrain = scene.Scene(64, gsd, torch.device("cuda")).height((ii + 0.5 - w / 2) * gsd, (jj + 0.5 - h / 2) * gsd)   # the terrain needs no texture
    truth = (terrain / gsd).contiguous()                                 # heights in cells
    del terrain, ii, jj
    gen = torch.Generator("cuda").manual_seed(1)
    subject = truth + 0.05 * torch.randn((h, w), device="cuda", generator=gen)
    subject.view(torch.int32)[torch.rand((h, w), device="cuda", generator=gen) < 0.05] = capi.STEREO_INVALID_BITS
    fr = capi.DsmFrame.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, w, h)
    raster, n = capi.dsm_points(subject, fr)
    raster = raster.contiguous()
    shuffled = raster[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    cells = capi.disparity_mesh(truth, 1, float("inf"))[1]
    say("reference: %d x %d terrain, relief %.1f cells; subject: %d points, noise 0.05 cells" % (w, h, float(truth.max() - truth.min()), n))

    def copy_of(nbytes):
        a, b = capi.dev_bytes(nbytes // 2), capi.dev_bytes(nbytes // 2)
        return summary(timed(lambda: b.copy_(a), repeats))

    def report(key, label, s, nbytes):
        c = copy_of(nbytes)
        s.update(bytes=int(nbytes), copy_ms=c["ms"], over_copy=round(s["ms"] / c["ms"], 2), over_block_matching=round(s["ms"] / sad["ms"], 4))
        res[key] = s
        say("  %-44s %9.4f ms (%.4f .. %.4f); at least %7.1f MB, whose copy takes %.4f ms: %7.2f x the copy, %.4f x block matching" % (
            label, s["ms"], s["min_ms"], s["max_ms"], nbytes / 1e6, c["ms"], s["over_copy"], s["over_block_matching"]))

    diff = torch.empty((n,), dtype=torch.float32, device="cuda")
    if not stats_only:
        for cloud_name, cloud in (("raster", raster), ("shuffled", shuffled)):
            for mode, c in (("CELL", None), ("MESH", cells)):
                s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_dsm_difference(capi.ptr(cloud), u32(n), capi.ptr(truth), ctypes.byref(fr), capi.ptr(c),
                                                                                   capi.ptr(diff), capi.stream_ptr())), repeats))
                report("difference/%s/%s" % (mode, cloud_name), "difference %s %s" % (mode, cloud_name), s, 16 * n + 4 * w * h + (cells.numel() if c is not None else 0))
    capi.dsm_difference(raster, truth, fr, cells, out=diff)
    del shuffled, subject
    inputs = [("scene", diff), ("constant", torch.full((n,), 0.25, dtype=torch.float32, device="cuda")),
              ("random bits", torch.randint(-2 ** 31, 2 ** 31, (n,), device="cuda", dtype=torch.int64, generator=gen).to(torch.int32).view(torch.float32))]
    out = torch.empty(72, dtype=torch.uint8, device="cuda")
    for name, values in inputs:
        for quantiles in ((5000,), EIGHT):
            prm = capi.DiffStatsParams(0.0, 0, len(quantiles), (u32 * 8)(*quantiles))
            ws = capi.dev_bytes(int(LIB.ssrlcv_hip_difference_stats_workspace_bytes(u32(n), ctypes.byref(prm))))
            s = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_difference_stats(capi.ptr(values), u32(n), ctypes.byref(prm), capi.ptr(out), capi.ptr(ws),
                                                                                 capi.c_sz(ws.numel()), capi.stream_ptr())), repeats))
            rec = capi.DiffStats.from_buffer_copy(out.cpu().numpy().tobytes())
            s.update(finite=int(rec.finite), median=float(rec.quantile[0]) if len(quantiles) == 1 else float(rec.quantile[2]))
            report("stats/%s/q%d" % (name, len(quantiles)), "stats %s, %d quantile%s" % (name, len(quantiles), "" if len(quantiles) == 1 else "s"), s, 4 * n)

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
