#!/usr/bin/env python
"""Developer tool: hole filling (include/ssrlcv_hip.h "hole filling") on the library ssrlcv_amd/_lib.py loads (release by
default).  Not part of the driver contract (bench.py).  Nothing is gated on these numbers: the block-matching call and a plain
device copy of the same run are the yardsticks, the spread of identical repeats is the noise.

At size^2 (4096 by default), paths 0xFF, minHits 5, rule MIN, maxGap 32 unless said otherwise, with the mask.  Every buffer is
allocated beforehand, one warm-up and `repeats` timed runs between stream events, medians with min and max.  The call is out of
place, so nothing is restored between runs.  Four maps:
  post-speckle     the pair of tools/bench_stereo.py matched by ssrlcv_hip_stereo_sad_u8 at radius 2, D = 64 from 0, left-right
                   tolerance 1, sub-pixel step, then the speckle filter (maxDiff 1, maxSpeckleSize 200): the map of
                   profiles/speckle_bench.txt, the one the call follows in the chain
  all valid        nothing to fill: the floor of the carry passes, which read the map once per direction whatever it holds
  half hole        the left half of the map is one hole: size / 2 steps of carry, and every hit map entry of that half stored
                   and read
  checkerboard     a one-pixel checkerboard of holes: a store at every other pixel of every hit map; minHits 4, because the
                   diagonal rays of a hole meet holes only
Beside each time the bytes the call must move at least -- 4 read + 4 written per pixel; the mask byte, the hit maps and the
re-reads per direction are the call's own doing and not counted -- the time of a plain device-to-device copy moving as many
bytes in the same run, and the ratio to the block-matching call.
The half-hole map is then run at maxGap 4 and at UINT32_MAX: the design claim is that no loop depends on the gap, so the two
must agree within the noise.  Last, the half-hole map with the horizontal directions alone (0x03) and with the six others
(0xFC): which pass the time belongs to.

usage: bench_fill.py [repeats] [--size N] [--out FILE]      (defaults 9, 4096, profiles/fill_bench.txt)"""
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
PATHS, MAX_GAP, MIN_HITS = 0xFF, 32, 5
BYTES = 8


def summary(times):
    return dict(ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", os.path.join(ROOT, "profiles", "fill_bench.txt"), str)
    size = take(args, "--size", 4096, int)
    repeats = max(3, int(args[0])) if args else 9
    assert torch.cuda.is_available(), "bench_fill.py needs a GPU"
    torch.cuda.set_device(0)
    u32, f32, LIB = capi.c_u32, capi.c_f32, capi.LIB
    w = h = size
    px = w * h
    left, right, _ = make_pair(size)
    disp = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.int32, device="cuda")
    out = torch.empty_like(disp)
    mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    invalid = torch.tensor([capi.STEREO_INVALID_BITS], dtype=torch.int32, device="cuda").view(torch.float32)[0]
    res = dict(tool="bench_fill", date=datetime.date.today().isoformat(), commit=commit(), library=_lib.flavour(),
               device=torch.cuda.get_device_name(0), repeats=repeats, size=size, radius=RADIUS, numDisparities=D, paths=PATHS, maxGap=MAX_GAP,
               minHits=MIN_HITS, rule="min", bytes_per_pixel=BYTES)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("bench_fill %s commit %s library %s on %s: %d^2, median (min .. max) of %d runs after one warm-up" % (
        res["date"], res["commit"], res["library"], res["device"], size, repeats))

    # ---- the block matching that makes the map, then the speckle filter
    p = capi.StereoParams(RADIUS, 0, D, capi.STEREO_NO_LIMIT, 1, 1)
    sad_ws = capi.stereo_workspace(w, h, p)
    sad = summary(timed(lambda: capi.check(LIB.ssrlcv_hip_stereo_sad_u8(capi.ptr(left), capi.ptr(right), u32(w), u32(h), ctypes.byref(p),
                                                                        capi.ptr(sad_ws), capi.c_sz(sad_ws.numel()), capi.ptr(disp), capi.ptr(cost),
                                                                        capi.stream_ptr())), repeats))
    del sad_ws
    capi.stereo_filter_speckles(disp, cost, MAX_SIZE, MAX_DIFF)
    res["block_matching"] = sad
    say("block matching, SAD radius %d, D %d, LR 1, sub-pixel   %8.4f ms (%.4f .. %.4f)" % (RADIUS, D, sad["ms"], sad["min_ms"], sad["max_ms"]))

    a, b = capi.dev_bytes(px * BYTES // 2), capi.dev_bytes(px * BYTES // 2)
    copy = summary(timed(lambda: b.copy_(a), repeats))
    del a, b
    res["copy"] = copy
    say("a device copy of %d B/pixel = %.1f MB moved            %8.4f ms (%.4f .. %.4f)" % (BYTES, px * BYTES / 1e6, copy["ms"], copy["min_ms"], copy["max_ms"]))

    ws = capi.dev_bytes(8 * ((4 * px + 255) // 256 * 256))

    def run(key, label, src, paths=PATHS, max_gap=MAX_GAP, min_hits=MIN_HITS):
        fp = capi.FillParams(paths, max_gap, min_hits, capi.FILL_MIN)

        def call():
            capi.check(LIB.ssrlcv_hip_stereo_fill_holes(capi.ptr(src), capi.ptr(out), capi.ptr(mask), u32(w), u32(h), ctypes.byref(fp), capi.ptr(ws),
                                                        capi.c_sz(ws.numel()), capi.stream_ptr()))

        s = summary(timed(call, repeats))
        s["holes"] = int((src.view(torch.int32) == capi.STEREO_INVALID_BITS).sum())
        s["filled"] = int(mask.sum())
        s["over_copy"] = round(s["ms"] / copy["ms"], 2)
        s["over_block_matching"] = round(s["ms"] / sad["ms"], 4)
        res[key] = s
        say("%-52s %8.4f ms (%.4f .. %.4f); %9d holes, %9d filled; %6.2f x the copy, %.3f x block matching" % (
            label, s["ms"], s["min_ms"], s["max_ms"], s["holes"], s["filled"], s["over_copy"], s["over_block_matching"]))
        return s

    run("post_speckle", "the post-speckle block-matching map", disp)
    valid = torch.full((h, w), 20.0, dtype=torch.float32, device="cuda")
    run("all_valid", "an all-valid map (the floor of the carry passes)", valid)
    half = valid.clone()
    half[:, : w // 2] = invalid
    run("half_hole", "the left half one hole", half, min_hits=1)
    checker = valid.clone()
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    checker[(xs + ys) % 2 == 1] = invalid
    del ys, xs
    run("checkerboard", "a one-pixel checkerboard, minHits 4", checker, min_hits=4)   # a hole's diagonal rays meet holes only

    near = run("half_hole_gap4", "the left half one hole, maxGap 4", half, max_gap=4, min_hits=1)
    far = run("half_hole_unlimited", "the left half one hole, maxGap UINT32_MAX", half, max_gap=0xFFFFFFFF, min_hits=1)
    noise = max(near["max_ms"] - near["min_ms"], far["max_ms"] - far["min_ms"])
    res["gap_difference_ms"] = round(abs(near["ms"] - far["ms"]), 4)
    res["gap_noise_ms"] = round(noise, 4)
    say("    maxGap 4 against UINT32_MAX: the medians differ by %.4f ms; the spread of identical repeats is %.4f ms" % (
        res["gap_difference_ms"], res["gap_noise_ms"]))
    run("half_hole_rows", "the left half one hole, paths 0x03 (rows)", half, paths=0x03, min_hits=1)
    run("half_hole_march", "the left half one hole, paths 0xFC (the six others)", half, paths=0xFC, min_hits=1)

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
