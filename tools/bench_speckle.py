#!/usr/bin/env python
"""Developer tool: the disparity post-filters (include/ssrlcv_hip.h "disparity post-filters") on the map of the block matching
they follow, on the library ssrlcv_amd/_lib.py loads (release by default).  Not part of the driver contract (bench.py).
Nothing is gated on these numbers: the block-matching call and a plain device copy of the same run are the yardsticks.

At size^2 (4096 by default): the pair of tools/bench_stereo.py, matched by ssrlcv_hip_stereo_sad_u8 at radius 2, D = 64 from 0,
left-right tolerance 1, sub-pixel step.  Every buffer allocated beforehand, one warm-up and `repeats` timed runs between stream
events, medians with min and max.  The speckle filter works in place, so the map is restored from a copy before every run,
outside the timed interval.
  block matching   the call that made the map: what the filters are an addition to
  components       ssrlcv_hip_disparity_components with sizes
  speckles         ssrlcv_hip_stereo_filter_speckles, the whole call, maxDiff 1, maxSpeckleSize 200, with the cost map: on that
                   map, and on an all-valid constant map -- one component of size^2 pixels, every tile adding its count to one
                   counter: the worst case for the counts
  median           ssrlcv_hip_stereo_filter_median at radius 1 and 2
Beside each time the bytes the call must move at least, and the time of a plain device-to-device copy moving as many bytes
(read + written) in the same run.  What is counted, per pixel:
  median           4 read + 4 written = 8 B
  labelling        4 (the map read by the tile pass) + 4 + 4 (labels and counts written) + 4 + 4 (both read by the flatten pass)
                   + 4 (labels rewritten) = 24 B; the seam pass touches 1 / 16 + 1 / 64 of the pixels and is not counted
  components       labelling + 4 (labels read) + 4 (sizes written) = 32 B; the gather of counts[label] is not counted
  speckles         labelling + 4 (labels read) = 28 B; the gather and the writes to removed pixels are not counted

usage: bench_speckle.py [repeats] [--size N] [--out FILE]      (defaults 7, 4096, profiles/speckle_bench.txt)"""
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
MAX_DIFF, MAX_SIZE = 1.0, 200
BYTES = dict(median=8, components=32, speckles=28)


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def timed_restored(restore, fn, repeats):
    """like bench_stereo.timed, with restore() before every run and outside the events"""
    restore()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "speckle_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 7
    assert torch.cuda.is_available(), "bench_speckle.py needs a GPU"
    torch.cuda.set_device(0)
    u32, f32, LIB = capi.c_u32, capi.c_f32, capi.LIB
    w = h = size
    px = w * h
    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    work = torch.empty_like(disp)
    work_cost = torch.empty_like(cost)
    out = torch.empty_like(disp)
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    sizes = torch.empty((h, w), dtype=torch.int32, device="cuda")
    constant = torch.full((h, w), 20.0, dtype=torch.float32, device="cuda")
    ws = capi.dev_bytes(int(LIB.ssrlcv_hip_stereo_filter_speckles_workspace_bytes(u32(w), u32(h))))
    res = dict(tool="bench_speckle", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, radius=RADIUS, numDisparities=D, maxDiff=MAX_DIFF,
               maxSpeckleSize=MAX_SIZE, bytes_per_pixel=BYTES)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_speckle %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    # ---- the block matching that makes the map
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws
    sad["valid_share"] = round(float((disp.view(torch.int32) != capi.STEREO_INVALID_BITS).float().mean()), 4)
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f), valid %.3f" % (
        RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"], sad["valid_share"]))

    # ---- a plain copy of as many bytes as each call must move: n bytes read + n written = 2 n moved
    def copy_ms(bytes_per_pixel):
        n = px * bytes_per_pixel // 2
        a, b = capi.dev_bytes(n), capi.dev_bytes(n)
        s = summary(timed(lambda: b.copy_(a), repeats))
        del a, b
        return s

    copies = {k: copy_ms(v) for k, v in BYTES.items()}
    res["copy"] = copies

    def row(key, label, kind, s):
        s["copy_ms"] = copies[kind]["ms"]
        s["min_bytes"] = px * BYTES[kind]
        res[key] = s
        say("%-52s %8.4f ms (%.4f .. %.4f); %2d B/pixel = %6.1f MB at least; a copy of as many: %.4f ms (%.2f x)" % (
            label, s["ms"], s["min_ms"], s["max_ms"], BYTES[kind], s["min_bytes"] / 1e6, s["copy_ms"], s["ms"] / s["copy_ms"]))

    def components():
        capi.check(LIB.ssrlcv_hip_disparity_components(capi.ptr(disp), u32(w), u32(h), f32(MAX_DIFF), capi.ptr(labels), capi.ptr(sizes), capi.ptr(ws),
                                                       capi.c_sz(ws.numel()), capi.stream_ptr()))

    row("components", "components with sizes, the block-matching map", "components", summary(timed(components, repeats)))
    res["components"]["count"] = int((labels.view(-1) == torch.arange(px, dtype=torch.int32, device="cuda")).sum())
    res["components"]["largest"] = int(sizes.max())
    say("    %d components, the largest of %d pixels" % (res["components"]["count"], res["components"]["largest"]))

    def speckles():
        capi.check(LIB.ssrlcv_hip_stereo_filter_speckles(capi.ptr(work), capi.ptr(work_cost), u32(w), u32(h), f32(MAX_DIFF), u32(MAX_SIZE), capi.ptr(ws),
                                                         capi.c_sz(ws.numel()), capi.stream_ptr()))

    def restore_real():
        work.copy_(disp)
        work_cost.copy_(cost)

    def restore_constant():
        work.copy_(constant)
        work_cost.copy_(cost)

    row("speckles_real", "speckles, whole call, the block-matching map", "speckles", summary(timed_restored(restore_real, speckles, repeats)))
    removed = int((work.view(torch.int32) == capi.STEREO_INVALID_BITS).sum()) - int((disp.view(torch.int32) == capi.STEREO_INVALID_BITS).sum())
    res["speckles_real"]["removed_pixels"] = removed
    say("    %d pixels removed; %.3f x the block-matching call" % (removed, res["speckles_real"]["ms"] / sad["ms"]))
    row("speckles_constant", "speckles, whole call, an all-valid constant map", "speckles", summary(timed_restored(restore_constant, speckles, repeats)))
    res["speckles_constant"]["over_real"] = round(res["speckles_constant"]["ms"] / res["speckles_real"]["ms"], 3)
    say("    %.3f x the block-matching map's time (every tile adds its count to ONE counter)" % res["speckles_constant"]["over_real"])

    for m in (1, 2):
        def median():
            capi.check(LIB.ssrlcv_hip_stereo_filter_median(capi.ptr(disp), capi.ptr(out), u32(w), u32(h), u32(m), capi.stream_ptr()))
        row("median%d" % m, "median, radius %d, the block-matching map" % m, "median", summary(timed(median, repeats)))
    res["speckles_over_block_matching"] = round(res["speckles_real"]["ms"] / sad["ms"], 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
